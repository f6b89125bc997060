"""Designed inputs of the relaxation kernels (codlad_relax, codlad_relax_energy) and the conditioning rule they are held to.

The rule (rule 1 of tests/test_relax_fp64_parity.py), per structure, everything in float64 from the float32 inputs the device
is handed: relax_ref.conditioning gives every atom a scale_a = 2^-24 (S_a + K_a) and every energy a scale_E; with
r_a = max_c |g[a, c] - g64[a, c]| / scale_a and E_ref = the largest r_a of the numpy float32 restatement on that structure,
  free atoms   r_a(device) <= 4 max(E_ref, 0.25)            fixed atoms   gradient exactly 0
  energies     |e - e64| <= 4 scale_E each; a class with no member (scale_E == 0) is exactly 0.0
An atom no term touches has scale 0: its gradient must be exactly 0.  Nothing here is taken from the device.

The cases (CASES, each -> dict: radius, bonds, quads, fixed, xyz0, xyz float32 [S, n, 3], T, refs[s] = the float64 references
a structure may be held to - one, or two where ONE quad is undecided at the weight threshold):
  tiny_*             1, 2 and 3 atoms; n = 1 has no pair, no quad, n_pairs == 0
  start              x == x0 on test_relax.case(257): both restraint energies and every contact-free gradient exactly 0
  far                case(257) on the 2^-13 A grid, translated by (+500, -800, +1200): exact in float32 (see far())
  coincident         free pairs at distance 0, 1e-4 and 1e-3 A inside a 40-atom chain
  many_quads_*       100 atoms, one row block, 255 / 256 / 257 / 513 / 0 quads: relax_prep_kernel's second and third pass
  weight_threshold   quads whose flatter start-structure bond angle has |sin| = 0.1 (1 +- 2^-10), and one within 2 ulp of 0.1
  batch              40 atoms x 130 structures (sliced to 64, 65, 130): the second and third block of relax_finish_kernel
"""
import functools

import numpy as np

from tests import relax_ref as rr

F32 = np.float32
FACTOR, FLOOR = 4.0, 0.25
MARGIN = 1e-4                       # no free pair within this of its sigma, as tests/test_relax.py
ULP_01 = float(np.spacing(F32(0.1)))
R_C = 0.68


# ------------------------------------------------------------------------------------------------------------ the rule
def _ratio(err, scale):
    """err / scale with 0 / 0 = 0 and x / 0 = inf."""
    err, scale = np.asarray(err, dtype=np.float64), np.asarray(scale, dtype=np.float64)
    out = np.where(err > 0, np.inf, 0.0)
    pos = scale > 0
    out[pos] = err[pos] / scale[pos]
    return out


def grad_ratios(g, ref):
    """r_a [n]; a fixed atom reads 0 when its gradient is exactly 0 and inf otherwise."""
    err = np.abs(np.asarray(g, dtype=np.float64) - ref["g"]).max(-1)
    r = _ratio(err, ref["scale"])
    fx = ref["fixed"]
    r[fx] = np.where(np.asarray(g)[fx].any(-1), np.inf, 0.0)
    return r


def energy_ratios(e, ref):
    return _ratio(np.abs(np.asarray(e, dtype=np.float64) - ref["e"]), ref["scale_E"])


def structure_ref(x, x0, T, fixed, w=None, e64g64=None, e32g32=None, **k):
    """The float64 reference of one structure with its scales and the float32 restatement's figures: e [3], g [n, 3],
    conditioning's fields, fixed, E_ref, r32 [n], e32_ratio [3], bound [n] = 4 max(E_ref, 0.25) scale_a."""
    fixed = np.zeros(T["n"], dtype=bool) if fixed is None else np.asarray(fixed, dtype=bool)
    e64, g64 = e64g64 if e64g64 is not None else rr.energy(x, x0, T, fixed, w=w, **k)[:2]
    e32, g32 = e32g32 if e32g32 is not None else rr.energy(x, x0, T, fixed, dtype=F32, w=w, **k)[:2]
    ref = dict(rr.conditioning(x, x0, T, w=w, **k), e=e64, g=g64, fixed=fixed)
    ref["r32"] = grad_ratios(g32, ref)
    ref["E_ref"] = float(ref["r32"].max(initial=0.0))
    ref["e32_ratio"] = energy_ratios(e32, ref)
    ref["bound"] = FACTOR * max(ref["E_ref"], FLOOR) * ref["scale"]
    return ref


def judge(ref, e, g):
    """-> (worst r_a / max(E_ref, 0.25) over the atoms: bound FACTOR; |e - e64| / scale_E [3]: bound FACTOR)."""
    return float(grad_ratios(g, ref).max(initial=0.0)) / max(ref["E_ref"], FLOOR), energy_ratios(e, ref)


def passes(figures):
    return figures[0] <= FACTOR and bool((figures[1] <= FACTOR).all())


def judge_any(refs, e, g):
    """The figures against the first reference that is kept, else against the first."""
    figs = [judge(r, e, g) for r in refs]
    return next((f for f in figs if passes(f)), figs[0])


# ---------------------------------------------------------------------------------------------------------- building
def chain_xyz(n, angle, torsion, bond=1.5):
    """n atoms placed one after the other from bond lengths, bond angles and torsions (degrees; scalars or [n]), float64."""
    angle, torsion = np.deg2rad(np.broadcast_to(angle, n)), np.deg2rad(np.broadcast_to(torsion, n))
    bond = np.broadcast_to(bond, n)
    x = np.zeros((n, 3))
    if n > 1:
        x[1] = [bond[1], 0, 0]
    if n > 2:
        x[2] = x[1] + bond[2] * np.array([-np.cos(angle[2]), np.sin(angle[2]), 0])
    for k in range(3, n):
        a, b, c = x[k - 3], x[k - 2], x[k - 1]
        bc = (c - b) / np.linalg.norm(c - b)
        nrm = np.cross(b - a, bc)
        nrm /= np.linalg.norm(nrm)
        m = np.cross(nrm, bc)
        th, ta = angle[k], torsion[k]
        x[k] = c + bond[k] * (-np.cos(th) * bc + np.sin(th) * np.cos(ta) * m + np.sin(th) * np.sin(ta) * nrm)
    return x


def chain_bonds(n):
    return np.array([(k, k + 1) for k in range(n - 1)], dtype=np.int64).reshape(-1, 2)


def sigma_gap(x, T):
    """d - sigma of every free pair of one structure, float64, d with the kernel's 1e-7 under the root."""
    d = rr._dist(np.asarray(x, dtype=np.float64), T["free_i"], T["free_j"], np.float64)[1]
    return d - (T["radius"][T["free_i"]] + T["radius"][T["free_j"]]) * rr.DEFAULTS["contact_scale"]


def off_sigma(xyz, T, rng, keep=(), step=0.01):
    """Moves, in place, one atom of every free pair within MARGIN of its sigma (never an atom of `keep`)."""
    keep = np.asarray(sorted(keep), dtype=np.int64)
    for s in range(len(xyz)):
        for _ in range(100):
            near = np.nonzero(np.abs(sigma_gap(xyz[s], T)) < MARGIN)[0]
            if not len(near):
                break
            j = T["free_j"][near]
            j = np.where(np.isin(j, keep), T["free_i"][near], j)
            atoms = np.setdiff1d(np.unique(j), keep)
            xyz[s, atoms] += (np.round(rng.normal(0, step, (len(atoms), 3)) * 8192) / 8192).astype(F32)
        else:
            raise ValueError("a free pair stays on its sigma")
    return xyz


def make(radius, bonds, quads, xyz0, xyz, fixed=None, alternatives=None):
    """alternatives[s]: None, or the index of the ONE quad of structure s that may take either weight."""
    radius = np.asarray(radius, dtype=F32)
    bonds = np.asarray(bonds, dtype=np.int64).reshape(-1, 2)
    quads = np.asarray(quads, dtype=np.int64).reshape(-1, 4)
    xyz0, xyz = np.ascontiguousarray(xyz0, dtype=F32), np.ascontiguousarray(xyz, dtype=F32)
    n = len(radius)
    fixed = np.zeros(n, dtype=bool) if fixed is None else np.asarray(fixed, dtype=bool)
    T = rr.tables(radius, bonds, quads)
    refs = []
    for s in range(len(xyz)):
        und = None if alternatives is None else alternatives[s]
        if und is None:
            refs.append([structure_ref(xyz[s], xyz0[s], T, fixed)])
        else:
            w = rr.start_constants(xyz0[s], T)[3]
            refs.append([structure_ref(xyz[s], xyz0[s], T, fixed, w=np.where(np.arange(len(quads)) == und, v, w))
                         for v in (False, True)])
    return dict(radius=radius, bonds=bonds, quads=quads, xyz0=xyz0, xyz=xyz, fixed=fixed, T=T, refs=refs,
                undecided=alternatives)


# --------------------------------------------------------------------------------------------------------------- tiny
def tiny(n, fixed0=False):
    """A straight piece of chain, its atoms and its place jittered.  A structure of one or two terms has a float32 restatement
    that can be right by luck; seed 3100 is the first of 3100, 3101, ... at which it reads E_ref >= 0.1 on all three
    structures of n = 2 and n = 3 (the restatement's figure, asserted on the CPU; nothing of the device's)."""
    rng = np.random.default_rng(3100)
    x0 = np.stack([chain_xyz(n, 111.0, 180.0) + rng.normal(0, 0.05, (n, 3)) + rng.normal(0, 3.0, 3) for _ in range(3)])
    x = x0 + rng.normal(0, 0.1, x0.shape)
    fixed = np.zeros(n, dtype=bool)
    fixed[0] = fixed0
    return make(np.full(n, R_C), chain_bonds(n), np.zeros((0, 4)), x0, x, fixed)


# ---------------------------------------------------------------------------------------------- start, far: case(257)
def _case257():
    from tests import test_relax as tr
    return tr.case(257)


def start():
    """x == x0: the start structures of case(257) as they are (their free pairs keep MARGIN from sigma: asserted on the CPU)."""
    c = _case257()
    return make(c["radius"], c["bonds"], c["quads"], c["xyz0"], c["xyz0"], c["fixed"])


FAR_SHIFT = np.array([500.0, -800.0, 1200.0])
FAR_GRID = 2.0 ** -13                         # the spacing of float32 in [1024, 2048)


def far_base():
    """case(257) with every coordinate rounded to the 2^-13 A grid, pairs moved off sigma again (on the grid).  A float32
    translation of arbitrary coordinates to 1200 A rounds each by up to 6e-5 A - that is another structure, whose
    energies differ from the untranslated one's by 5 to 97 scale_E (test_relax_cases_host.py holds the figure above 1); on the
    grid the translation is exact, so the translated and the untranslated input are the same structure to float64 and the
    case asks the one thing a translation can: that the kernel forms differences of coordinates before anything else."""
    c = _case257()
    rng = np.random.default_rng(3257)
    snap = lambda a: (np.round(a.astype(np.float64) / FAR_GRID) * FAR_GRID).astype(F32)                       # noqa: E731
    xyz0, xyz = snap(c["xyz0"]), snap(c["xyz"])
    T = rr.tables(c["radius"], c["bonds"], c["quads"])
    off_sigma(xyz, T, rng)
    return c, xyz0, xyz


def far():
    c, xyz0, xyz = far_base()
    shift = FAR_SHIFT.astype(F32)
    return make(c["radius"], c["bonds"], c["quads"], xyz0 + shift, xyz + shift, c["fixed"])


# --------------------------------------------------------------------------------------------------------- coincident
COINCIDENT_PAIRS = ((4, 20, 0.0), (9, 30, 1e-4), (14, 36, 1e-3))


def coincident():
    """A 40-atom chain, x = x0 + N(0, 0.05 A), then atom b of each pair put at atom a + delta along an axis that differs by
    structure (in float32: a + 0 is a's bits, so the first pair's distance is exactly 0)."""
    n = 40
    rng = np.random.default_rng(3400)
    bonds = chain_bonds(n)
    quads = np.array([(k - 1, k, k + 1, k + 2) for k in range(1, n - 2, 3)], dtype=np.int64)
    T = rr.tables(np.full(n, R_C), bonds, quads)
    x0 = np.stack([chain_xyz(n, 111.0 + rng.normal(0, 3, n), rng.choice(rr.ROTAMERS, n) + rng.normal(0, 10, n))
                   for _ in range(3)]).astype(F32)
    x = (x0 + rng.normal(0, 0.05, x0.shape)).astype(F32)
    for s in range(3):
        for a, b, delta in COINCIDENT_PAIRS:
            x[s, b] = x[s, a]
            x[s, b, s] = x[s, a, s] + F32(delta)
    off_sigma(x, T, rng, keep={p for a, b, _d in COINCIDENT_PAIRS for p in (a, b)})
    return make(np.full(n, R_C), bonds, quads, x0, x)


# --------------------------------------------------------------------------------------------------------- many_quads
MANY_N, MANY_COUNTS = 100, (255, 256, 257, 513, 0)


def many_graph():
    """The ternary tree over 100 atoms (the parent of k is (k - 1) // 3) and every directed 3-path a - b - c - d of it, in
    lexicographic order of (b, c, a, d): 558 rows, the path and its reverse being two rows (two terms)."""
    n = MANY_N
    bonds = np.array(sorted(((k - 1) // 3, k) for k in range(1, n)), dtype=np.int64)
    adj = [set() for _ in range(n)]
    for i, j in bonds.tolist():
        adj[i].add(j), adj[j].add(i)
    paths = [(a, b, c, d) for b in range(n) for c in sorted(adj[b]) for a in sorted(adj[b] - {c}) for d in sorted(adj[c] - {b})]
    return bonds, np.array(paths, dtype=np.int64)


@functools.lru_cache(maxsize=None)
def _many_xyz():
    """Start structures in which every bond angle at every atom has |sin| >= 0.3 (so every quad has weight 1), drawn child by
    child; x = x0 + N(0, 0.08 A), off sigma."""
    n = MANY_N
    rng = np.random.default_rng(3500)
    bonds, paths = many_graph()
    T = rr.tables(np.full(n, R_C), bonds, paths)
    parent = [(k - 1) // 3 for k in range(n)]
    x0 = np.zeros((3, n, 3))
    for s in range(3):
        dirs = {}                                               # atom -> the unit vectors of its bonds so far
        for k in range(1, n):
            p = parent[k]
            for _ in range(10000):
                u = rng.normal(0, 1, 3)
                u /= np.linalg.norm(u)
                if all(np.linalg.norm(np.cross(u, v)) >= 0.5 and u @ v < 0.5 for v in dirs.get(p, [])):
                    break
            else:
                raise ValueError("no direction left")
            dirs.setdefault(p, []).append(u)
            dirs.setdefault(k, []).append(-u)
            x0[s, k] = x0[s, p] + 1.5 * u
    x0 = x0.astype(F32)
    x = (x0 + rng.normal(0, 0.08, x0.shape)).astype(F32)
    off_sigma(x, T, rng)
    return x0, x


def many_quads(count):
    bonds, paths = many_graph()
    x0, x = _many_xyz()
    return make(np.full(MANY_N, R_C), bonds, paths[:count], x0, x)


# --------------------------------------------------------------------------------------------------- weight_threshold
WT_N = 16
WT_QUADS = np.array([(4 * k, 4 * k + 1, 4 * k + 2, 4 * k + 3) for k in range(4)], dtype=np.int64)
WT_ABOVE, WT_BELOW = 0.1 * (1 + 2.0 ** -10), 0.1 * (1 - 2.0 ** -10)
# per structure the target of the first bond angle's |sin| of quads 0 .. 3: a number, or "hi" / "lo" = the float32 input
# whose float64 sine is the closest to 0.1 from above / from below (the undecided quad)
WT_TARGETS = ((WT_ABOVE, WT_BELOW, "hi", None), (WT_BELOW, WT_ABOVE, "lo", None), (WT_BELOW, None, WT_ABOVE, WT_ABOVE))
WT_UNDECIDED = (2, 2, None)


def _tune(x, q, target):
    """Moves atom 4 q (the quad's first atom, part of no other quad) of the float32 structure x, in place: the bond angle at
    atom 4 q + 1 is opened until its float64 |sin| is `target`; "hi" / "lo": then one float32 step at a time."""
    a, b, c = 4 * q, 4 * q + 1, 4 * q + 2
    xb, xc = x[b].astype(np.float64), x[c].astype(np.float64)
    e = (xc - xb) / np.linalg.norm(xc - xb)
    perp = np.cross(e, [0.3, -0.5, 0.8])
    perp /= np.linalg.norm(perp)
    want = 0.1 if isinstance(target, str) else target
    th = np.arcsin(want)
    x[a] = (xb + 1.5 * (-np.cos(th) * e + np.sin(th) * perp)).astype(F32)      # nearly straight: the angle is 180 - 5.7 degrees
    if not isinstance(target, str):
        return
    # the float32 neighbours of that position, up to 12 places off in each coordinate: their float64 sines lie a few 1e-9 apart
    offs = np.arange(-12, 13)
    cand = [(np.float64(x[a, k]) + offs * np.float64(np.spacing(x[a, k]))).astype(F32).astype(np.float64) for k in range(3)]
    pa = np.stack(np.meshgrid(*cand, indexing="ij"), -1).reshape(-1, 3)
    b1, b2 = xb - pa, xc - xb
    sines = np.linalg.norm(np.cross(b1, b2), axis=-1) / (np.linalg.norm(b1, axis=-1) * np.linalg.norm(b2))
    gap = sines - 0.1 if target == "hi" else 0.1 - sines
    ok = np.nonzero((gap > 0) & (gap <= 2 * ULP_01))[0]
    if not len(ok):
        raise ValueError("no float32 input within 2 ulp of the threshold")
    x[a] = pa[ok[np.argmin(gap[ok])]].astype(F32)


def weight_threshold():
    rng = np.random.default_rng(3600)
    n = WT_N
    x0 = np.stack([chain_xyz(n, 111.0 + rng.normal(0, 3, n), rng.choice(rr.ROTAMERS, n) + rng.normal(0, 10, n))
                   for _ in range(3)]).astype(F32)
    for s in range(3):
        for q, target in enumerate(WT_TARGETS[s]):
            if target is not None:
                _tune(x0[s], q, target)
    x = (x0 + rng.normal(0, 0.03, x0.shape)).astype(F32)
    T = rr.tables(np.full(n, R_C), chain_bonds(n), WT_QUADS)
    off_sigma(x, T, rng)
    return make(np.full(n, R_C), chain_bonds(n), WT_QUADS, x0, x, alternatives=WT_UNDECIDED)


# -------------------------------------------------------------------------------------------------------------- batch
BATCH_N, BATCH_S, BATCH_SIZES = 40, 130, (64, 65, 130)
BATCH_PLANTED = (0, 17, 63, 64, 65, 100, 129)                  # the structures with a planted clash
BATCH_ALONE = lambda S: (0, 63, 64, S - 1) if S > 64 else (0, 63)                                                # noqa: E731
BATCH_ITER = 8


def batch():
    """Jittered copies (N(0, 0.03 A)) of one all-trans 40-atom chain - no free pair under sigma - as the start structures;
    in BATCH_PLANTED atom 14 is put 1.0 A from atom 10.  xyz_loop: the input of the loop (its own start structure), xyz: the
    same displaced by N(0, 0.05 A), for the single evaluation against xyz0 = xyz_loop."""
    n, S = BATCH_N, BATCH_S
    rng = np.random.default_rng(3700)
    base = chain_xyz(n, 111.0, 180.0, bond=1.53)
    x0 = (base[None] + rng.normal(0, 0.03, (S, n, 3))).astype(F32)
    for s in BATCH_PLANTED:
        u = x0[s, 14] - x0[s, 10]
        x0[s, 14] = x0[s, 10] + u / np.linalg.norm(u)
    quads = np.array([(k - 1, k, k + 1, k + 2) for k in range(1, n - 2, 2)], dtype=np.int64)
    T = rr.tables(np.full(n, R_C), chain_bonds(n), quads)
    off_sigma(x0, T, rng)
    x = (x0 + rng.normal(0, 0.05, x0.shape)).astype(F32)
    off_sigma(x, T, rng)
    c = make(np.full(n, R_C), chain_bonds(n), quads, x0, x)
    c["xyz_loop"] = x0
    return c


CASES = {"tiny_n1": lambda: tiny(1), "tiny_n2": lambda: tiny(2), "tiny_n3": lambda: tiny(3),
         "tiny_n2_fixed0": lambda: tiny(2, True), "start": start, "far": far, "coincident": coincident,
         **{f"many_quads_{c}": functools.partial(many_quads, c) for c in MANY_COUNTS},
         "weight_threshold": weight_threshold, "batch": batch}


@functools.lru_cache(maxsize=None)
def get(name):
    return CASES[name]()


@functools.lru_cache(maxsize=None)
def existing(n):
    """test_relax.case(n) with the references of rule 1 beside its own (the cached float64 and float32 evaluations reused)."""
    from tests import test_relax as tr
    c = tr.case(n)
    refs = [[structure_ref(c["xyz"][s], c["xyz0"][s], c["T"], c["fixed"], e64g64=c["ref64"][s][:2], e32g32=c["ref32"][s][:2])]
            for s in range(3)]
    return dict(c, refs=refs)


# ----------------------------------------------------------------------------------------------------------- the loop
LOOP_K = 24
# h0 = h_max of the second run.  At 0.1 the float64 loop rejects 0, 0 and 1 of the first 24 trials of the three structures; at
# 0.2 it rejects 2, 6 and 6 (both asserted by tests/test_relax_cases_host.py).
LOOP_H = 0.2


def loop_runs():
    """name -> dict(T, fixed, xyz float32 [S, n, 3], constants): the two runs of the per-step test."""
    from tests import test_relax as tr
    p, c = rr.planted_case("r32"), tr.case(257)
    return {"r32": dict(T=p["T"], fixed=p["fixed"], xyz=p["xyz"][None], constants={}, planted=p),
            "c257": dict(T=c["T"], fixed=c["fixed"], xyz=c["xyz"], constants=dict(h0=LOOP_H, h_max=LOOP_H), case=c)}
