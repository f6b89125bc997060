"""Float64 reference of the restrained clash relaxation (metrics.relax / relax_energy, codlad_relax).

Tables, the energy with its analytic gradient, and the minimiser, in numpy, sharing no code with metrics.relax_tables or
the kernel: the restrained pairs come from dataset_builder.high_order_edges (the dense construction), the free pairs from
its complement, the quads from an enumeration over the adjacency MATRIX, the ring bonds from a list by residue name.
`dtype` switches the arithmetic of the energy terms and of the gradient to float32 (one rounding per operation, the
formulas in the kernel's form); the energies are sums of those terms in float64 in both, as on the device.  The
difference of the two evaluations on the same inputs is ref_dev, the deviation the device is allowed four times over -
pooled over all cases in tests/test_relax.py, per atom and per term against `conditioning`'s scales in
tests/test_relax_fp64_parity.py.

The energy (per structure, A, no hydrogens), d = sqrt(|xi - xj|^2 + 1e-7):
  distance   k_r (d - d0)^2 over the pairs within 2 bonds, d0 from the start structure
  torsion    k_t w (1 - cos phi cos phi0 - sin phi sin phi0) over the quads, (cos, sin) = (n1.n2, |b2| b1.n2) normalised,
             evaluated as k_t w ((cos - cos0)^2 + (sin - sin0)^2) / 2 - the same function of two unit vectors, exactly 0 at
             the start structure; w = 0 where a bond angle of the quad has |sin| < 0.1 in the start structure
  repulsion  k_c (sigma - d)^2 over the pairs more than `order` bonds apart with d < sigma = (r_i + r_j) contact_scale
"""
import numpy as np
import torch

from codlad_amd.utils import dataset_builder as db

EPS = 1e-7
MIN_SIN = 0.1
DEFAULTS = dict(k_r=100.0, k_t=50.0, k_c=30.0, contact_scale=1.6, h0=0.01, h_max=0.1)

# the ring bonds of the residue templates, by name
RING_BONDS = {
    "PRO": "N-CA CA-CB CB-CG CG-CD CD-N",
    "PHE": "CG-CD1 CD1-CE1 CE1-CZ CZ-CE2 CE2-CD2 CD2-CG",
    "TYR": "CG-CD1 CD1-CE1 CE1-CZ CZ-CE2 CE2-CD2 CD2-CG",
    "HIS": "CG-ND1 ND1-CE1 CE1-NE2 NE2-CD2 CD2-CG",
    "TRP": "CG-CD1 CD1-NE1 NE1-CE2 CE2-CD2 CD2-CG CE2-CZ2 CZ2-CH2 CH2-CZ3 CZ3-CE3 CE3-CD2",
}


# ------------------------------------------------------------------------------------------------------------ tables
def expected_rigid_bonds(top):
    """(ring bonds by residue name, peptide bonds, ARG NE - CZ) as sets of (i, j), i < j."""
    ring, peptide, arg = set(), set(), set()
    for r, nm in enumerate(top.res_names):
        for bond in RING_BONDS.get(nm, "").split():
            a, b = (top.atom(r, x) for x in bond.split("-"))
            ring.add((min(a, b), max(a, b)))
        if r + 1 < top.n_residues and top.chain_ids[r + 1] == top.chain_ids[r]:
            peptide.add((top.atom(r, "C"), top.atom(r + 1, "N")))
        if nm == "ARG":
            a, b = top.atom(r, "NE"), top.atom(r, "CZ")
            arg.add((min(a, b), max(a, b)))
    return ring, peptide, arg


def brute_quads(bonds, rigid, n):
    """Every (a, b, c, d) over the rigid bonds b < c with a bonded to b, d bonded to c, a != c, d != b, a != d: from the
    adjacency matrix, in lexicographic order of (b, c, a, d)."""
    adj = np.zeros((n, n), dtype=bool)
    bonds = np.asarray(bonds, dtype=np.int64).reshape(-1, 2)
    adj[bonds[:, 0], bonds[:, 1]] = adj[bonds[:, 1], bonds[:, 0]] = True
    out = []
    for b, c in sorted((min(p), max(p)) for p in rigid):
        for a in range(n):
            for d in range(n):
                if adj[a, b] and adj[c, d] and a != c and d != b and a != d:
                    out.append((a, b, c, d))
    return np.array(out, dtype=np.int64).reshape(-1, 4)


def tables(radius, bonds, quads, order=2):
    """-> dict: n, radius float64, pairs int64 [P, 2] (i < j within 2 bonds), free bool [n, n] (more than `order` bonds
    apart, i != j) and the same as lists free_i < free_j, quads int64 [Q, 4]."""
    radius = np.asarray(radius, dtype=np.float64)
    n = len(radius)
    bonds = np.asarray(bonds, dtype=np.int64).reshape(-1, 2)

    def within(k):
        if not len(bonds):
            return np.zeros((0, 2), dtype=np.int64)
        return db.high_order_edges(torch.as_tensor(bonds), k, n).numpy().reshape(-1, 2)
    free = np.ones((n, n), dtype=bool)
    e = within(order)
    free[e[:, 0], e[:, 1]] = free[e[:, 1], e[:, 0]] = False
    np.fill_diagonal(free, False)
    iu, ju = np.triu_indices(n, 1)
    keep = free[iu, ju]
    return dict(n=n, radius=radius, pairs=within(2), free=free, free_i=iu[keep], free_j=ju[keep],
                quads=np.asarray(quads, dtype=np.int64).reshape(-1, 4))


# ------------------------------------------------------------------------------------------------------------- energy
def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _dist(x, i, j, dt):
    r = x[i] - x[j]
    return r, np.sqrt(_dot(r, r) + dt(EPS))


def torsion_parts(x, quads):
    """-> dict of the kernel's intermediate quantities of every quad, in x's dtype."""
    p0, p1, p2, p3 = (x[quads[:, k]] for k in range(4))
    b1, b2, b3 = p1 - p0, p2 - p1, p3 - p2
    n1, n2 = _cross(b1, b2), _cross(b2, b3)
    lb2 = np.sqrt(_dot(b2, b2))
    xx, yy = _dot(n1, n2), lb2 * _dot(b1, n2)
    with np.errstate(all="ignore"):
        r = np.sqrt(xx * xx + yy * yy)
        return dict(b1=b1, b2=b2, b3=b3, n1=n1, n2=n2, lb2=lb2, cos=xx / r, sin=yy / r)


def quad_angles(x, quads):
    """The two bond angles of every quad in degrees [Q, 2], float64."""
    x = np.asarray(x, dtype=np.float64)
    out = []
    for k in (0, 1):
        u, v = x[quads[:, k]] - x[quads[:, k + 1]], x[quads[:, k + 2]] - x[quads[:, k + 1]]
        c = (u * v).sum(-1) / np.sqrt((u * u).sum(-1) * (v * v).sum(-1))
        out.append(np.rad2deg(np.arccos(np.clip(c, -1, 1))))
    return np.stack(out, -1)


def angle_sines(x, quads):
    """|sin| of the two bond angles of every quad [Q, 2]."""
    t = torsion_parts(x, quads)
    with np.errstate(all="ignore"):
        s1 = np.sqrt(_dot(t["n1"], t["n1"])) / (np.sqrt(_dot(t["b1"], t["b1"])) * t["lb2"])
        s2 = np.sqrt(_dot(t["n2"], t["n2"])) / (t["lb2"] * np.sqrt(_dot(t["b3"], t["b3"])))
    return np.stack([s1, s2], -1)


def start_constants(x0, T, dtype=np.float64):
    """(d0 [P], cos0 [Q], sin0 [Q], w [Q]) of the start structure, in `dtype`."""
    dt = np.dtype(dtype).type
    x0 = np.asarray(x0).astype(dtype)
    d0 = _dist(x0, T["pairs"][:, 0], T["pairs"][:, 1], dt)[1]
    t = torsion_parts(x0, T["quads"])
    with np.errstate(invalid="ignore"):
        w = (angle_sines(x0, T["quads"]) >= dt(MIN_SIN)).all(-1)
    return d0, t["cos"], t["sin"], w


def energy(x, x0, T, fixed=None, dtype=np.float64, k_r=100.0, k_t=50.0, k_c=30.0, contact_scale=1.6, w=None, **_unused):
    """One structure x [n, 3] against the start structure x0 -> (energy float64 [3], grad [n, 3] in `dtype`, gmax).  The
    terms and the gradient are computed in `dtype` from the coordinates cast to it; the energies are float64 sums.
    w bool [Q]: the quad weights to use instead of the start structure's own (a quad AT the weight threshold)."""
    dt = np.dtype(dtype).type
    x = np.asarray(x).astype(dtype)
    n = T["n"]
    d0, c0, s0, w_own = start_constants(x0, T, dtype)
    w = w_own if w is None else np.asarray(w, dtype=bool)
    g = np.zeros((n, 3), dtype=dtype)
    k_r, k_t, k_c, cs = dt(k_r), dt(k_t), dt(k_c), dt(contact_scale)
    two = dt(2.0)
    # distance restraints
    i, j = T["pairs"][:, 0], T["pairs"][:, 1]
    r, d = _dist(x, i, j, dt)
    t = d - d0
    e_r = float((k_r * (t * t)).astype(np.float64).sum())
    f = (((two * k_r) * t) / d)[:, None] * r
    np.add.at(g, i, f)
    np.add.at(g, j, -f)
    # torsion restraints
    q = T["quads"][w]
    e_t = 0.0
    if len(q):
        c0, s0 = c0[w], s0[w]
        p = torsion_parts(x, q)
        dc, ds = p["cos"] - c0, p["sin"] - s0                                 # 1 - cos(phi - phi0) = |u - u0|^2 / 2
        e_t = float((k_t * (dt(0.5) * (dc * dc + ds * ds))).astype(np.float64).sum())
        de = k_t * (p["sin"] * c0 - p["cos"] * s0)
        bb = _dot(p["b2"], p["b2"])
        f0, f3 = -p["lb2"] / _dot(p["n1"], p["n1"]), p["lb2"] / _dot(p["n2"], p["n2"])
        u, v = _dot(p["b1"], p["b2"]) / bb, _dot(p["b3"], p["b2"]) / bb
        coef = [(f0, 0 * f0), (-f0 - u * f0, v * f3), (u * f0, -f3 - v * f3), (0 * f3, f3)]
        for k, (a1, a2) in enumerate(coef):
            np.add.at(g, q[:, k], de[:, None] * (a1[:, None] * p["n1"] + a2[:, None] * p["n2"]))
    # repulsion
    iu, ju = T["free_i"], T["free_j"]
    r, d = _dist(x, iu, ju, dt)
    sig = (T["radius"].astype(dtype)[iu] + T["radius"].astype(dtype)[ju]) * cs
    hit = d < sig
    r, d, sig, iu, ju = r[hit], d[hit], sig[hit], iu[hit], ju[hit]
    t = sig - d
    e_c = float((k_c * (t * t)).astype(np.float64).sum())
    f = (((two * k_c) * t) / d)[:, None] * r
    np.add.at(g, iu, -f)
    np.add.at(g, ju, f)
    if fixed is not None:
        g[np.asarray(fixed, dtype=bool)] = 0
    return np.array([e_r, e_t, e_c]), g, float(np.abs(g).max()) if g.size else 0.0


def conditioning(x, x0, T, w=None, k_r=100.0, k_t=50.0, k_c=30.0, contact_scale=1.6, **_unused):
    """What one float32 rounding can do to the gradient of every atom and to each energy, in float64 from the inputs as
    given -> dict: S, K float64 [n] (the force magnitudes and the stiffness x length of the terms touching an atom),
    scale [n] = 2^-24 (S + K), scale_E [3] per energy, contact bool [n] (the atom has a contact inside sigma), members
    int [3] (the terms of each class that are counted: pairs, quads of weight 1, contacts inside sigma).
      pair (i, j), t = d - d0             S += |2 k_r t|       K += 2 k_r (d + d0)       E: k_r t^2 + |2 k_r t| (d + d0)
      contact, t = sigma - d > 0          S += 2 k_c t         K += 2 k_c (d + sigma)    E: k_c t^2 + 2 k_c t (d + sigma)
      quad of weight 1, atom at `pos`     S += |dE/dphi| G     K += (k_t + |dE/dphi|) G / min(s1, s2)
        with G = |a1| |n1| + |a2| |n2| (a1, a2: the kernel's coefficients of dphi/dp[pos]) and s1, s2 the |sin| of the quad's
        bond angles at x;                 E: E_t + k_t chord / min(s1, s2 at x and at x0), chord = |(cos, sin) - (cos0, sin0)|
    A difference t is formed from two roots that are each off by half a place of their own size, hence (d + d0); the
    torsion's unit vector is off by a few places over the sine of the flatter bond angle."""
    x, x0 = np.asarray(x, dtype=np.float64), np.asarray(x0, dtype=np.float64)
    n = T["n"]
    d0, c0, s0, w_own = start_constants(x0, T)
    w = w_own if w is None else np.asarray(w, dtype=bool)
    S, K, sE = np.zeros(n), np.zeros(n), np.zeros(3)
    contact = np.zeros(n, dtype=bool)

    def both(i, j, s, k):
        for a in (i, j):
            np.add.at(S, a, s)
            np.add.at(K, a, k)
    i, j = T["pairs"][:, 0], T["pairs"][:, 1]
    d = _dist(x, i, j, np.float64)[1]
    t = d - d0
    f = np.abs(2 * k_r * t)
    both(i, j, f, 2 * k_r * (d + d0))
    sE[0] = (k_r * t * t + f * (d + d0)).sum()
    q = T["quads"][w]
    if len(q):
        c0, s0 = c0[w], s0[w]
        p = torsion_parts(x, q)
        de = np.abs(k_t * (p["sin"] * c0 - p["cos"] * s0))
        bb = _dot(p["b2"], p["b2"])
        n1, n2 = np.sqrt(_dot(p["n1"], p["n1"])), np.sqrt(_dot(p["n2"], p["n2"]))
        f0, f3 = -p["lb2"] / (n1 * n1), p["lb2"] / (n2 * n2)
        u, v = _dot(p["b1"], p["b2"]) / bb, _dot(p["b3"], p["b2"]) / bb
        flat, flat0 = angle_sines(x, q).min(-1), angle_sines(x0, q).min(-1)
        for k, (a1, a2) in enumerate([(f0, 0 * f0), (-f0 - u * f0, v * f3), (u * f0, -f3 - v * f3), (0 * f3, f3)]):
            G = np.abs(a1) * n1 + np.abs(a2) * n2
            np.add.at(S, q[:, k], de * G)
            np.add.at(K, q[:, k], (k_t + de) * G / flat)
        dc, ds = p["cos"] - c0, p["sin"] - s0
        chord2 = dc * dc + ds * ds
        sE[1] = (k_t * 0.5 * chord2 + k_t * np.sqrt(chord2) / np.minimum(flat, flat0)).sum()
    iu, ju = T["free_i"], T["free_j"]
    d = _dist(x, iu, ju, np.float64)[1]
    sig = (T["radius"][iu] + T["radius"][ju]) * contact_scale
    hit = d < sig
    iu, ju, d, sig = iu[hit], ju[hit], d[hit], sig[hit]
    t = sig - d
    both(iu, ju, 2 * k_c * t, 2 * k_c * (d + sig))
    sE[2] = (k_c * t * t + 2 * k_c * t * (d + sig)).sum()
    contact[iu] = contact[ju] = True
    return dict(S=S, K=K, scale=2.0 ** -24 * (S + K), scale_E=2.0 ** -24 * sE, contact=contact,
                members=np.array([len(i), len(q), int(hit.sum())]))


def sigma_margin(x, T, contact_scale=1.6):
    """Smallest |d - sigma| over the free pairs of one structure (float64), inf if there is none."""
    x = np.asarray(x, dtype=np.float64)
    iu, ju = T["free_i"], T["free_j"]
    if not len(iu):
        return np.inf
    d = _dist(x, iu, ju, np.float64)[1]
    return float(np.abs(d - (T["radius"][iu] + T["radius"][ju]) * contact_scale).min())


def free_pair_distances(x, T):
    """Plain distances (no EPS) of the free pairs i < j of one structure, float64."""
    x = np.asarray(x, dtype=np.float64)
    return np.sqrt(((x[T["free_i"]] - x[T["free_j"]]) ** 2).sum(-1))


def clashes(x, T, clash=1.2):
    """The geometry check's clash count over free pairs: sqrt(d^2 + 1e-7) < clash, float64."""
    d = free_pair_distances(x, T)
    return int((np.sqrt(d * d + EPS) < clash).sum())


# ----------------------------------------------------------------------------------------------------------- minimiser
def minimise(x, T, n_iter, fixed=None, h0=0.01, h_max=0.1, watch=None, **k):
    """Steepest descent with the rule of codlad_relax in float64 (the step lengths in float32, as on the device) -> dict:
    xyz, energy [n_iter + 1], trial_energy, step, accepted, gmax [n_iter], converged.  watch(x): called on every accepted
    state, the input included."""
    x0 = np.asarray(x, dtype=np.float64)
    x = x0.copy()
    e3, g, gmax = energy(x, x0, T, fixed, **k)
    e = float((e3[0] + e3[1]) + e3[2])
    h = np.float32(h0)
    out = dict(energy=[e], trial_energy=[], step=[], accepted=[], gmax=[])
    if watch is not None:
        watch(x)
    for _ in range(n_iter):
        xt = x - (float(h) / gmax) * g if gmax > 0 else x.copy()
        e3t, gt, gmaxt = energy(xt, x0, T, fixed, **k)
        et = float((e3t[0] + e3t[1]) + e3t[2])
        acc = et < e
        out["trial_energy"].append(et), out["step"].append(float(h)), out["accepted"].append(acc), out["gmax"].append(gmax)
        if acc:
            x, e, g, gmax = xt, et, gt, gmaxt
            h = min(h * np.float32(1.2), np.float32(h_max))
            if watch is not None:
                watch(x)
        else:
            h = h * np.float32(0.5)
        out["energy"].append(e)
    out = {k_: np.array(v) for k_, v in out.items()}
    out.update(xyz=x, converged=gmax == 0)
    return out


# ------------------------------------------------------------------------------------------------- planted clash inputs
ROTAMERS = (-60.0, 180.0, 60.0)
# the templates stereo_ref.build_chain builds with sane geometry: the side-chain atoms beyond the chi path of HIS, PHE, TRP,
# TYR, TPO and SEP are placed off their last three atoms, on top of their own residue, and no ring is closed (PRO's neither,
# which leaves the bond angles at its N to chance).  The quads of these chains are the peptide bonds' and ARG NE - CZ's.
PLANT_RES = "ALA ARG ASN ASP CYS GLN GLU GLY ILE LEU LYS MET SER THR VAL".split()
CLASH, CLEAN = 1.2, 1.4                     # the check's clash distance, and what a relaxed structure must keep: 1.2 + 0.2


def search_planted(n_res, seed, n_planted=4):
    """The search behind tests/golden/relax_planted.npz (slow: run by `python -m tests.relax_ref`, not by the tests).  A
    chain with sane backbone (phi -63 +/- 10, psi -43 +/- 10: a helix, omega 180, all L), chi from the rotamers, redrawn
    until NO free pair is under sigma + 0.05; then `n_planted` residues, at least 3 apart, whose chi1 is rotated until an atom
    of their side chain comes within 1.1 A of an atom it is free to clash with.  -> dict of the angles for build_chain:
    seq, phi, psi, chi (clean), chi_planted, residues.  Raises if the draw finds no clean baseline or cannot plant."""
    from tests import stereo_ref as sr
    rng = np.random.default_rng(seed)
    seq = [PLANT_RES[int(k)] for k in rng.integers(0, len(PLANT_RES), n_res)]
    phi, psi = -63.0 + rng.uniform(-10, 10, n_res), -43.0 + rng.uniform(-10, 10, n_res)
    omega = np.full(n_res, 180.0)
    chi = rng.choice(ROTAMERS, (n_res, 4))
    top, xyz = sr.build_chain(seq, phi, psi, omega, chi)
    T = case_tables(top)[1]
    res_of = top.residue_of_atom
    sig = (T["radius"][T["free_i"]] + T["radius"][T["free_j"]]) * DEFAULTS["contact_scale"]

    def under(x, cut):
        return np.nonzero(free_pair_distances(x.astype(np.float32), T) < cut)[0]

    for _ in range(300):                                   # redraw the chi of the residues of a pair under sigma
        bad = under(xyz, sig + 0.05)
        if not len(bad):
            break
        for r in set(res_of[T["free_i"][bad]].tolist()) | set(res_of[T["free_j"][bad]].tolist()):
            chi[r] = rng.choice(ROTAMERS, 4) + rng.uniform(-25, 25, 4)
        xyz = sr.build_chain(seq, phi, psi, omega, chi)[1]
    else:
        raise ValueError("no clean baseline")
    residues, chi_p = [], chi.copy()
    for r in rng.permutation(np.arange(1, n_res - 1)):
        if len(residues) == n_planted:
            break
        if sr.N_CHI[seq[r]] < 2 or any(abs(r - q) < 3 for q in residues):
            continue
        for c1 in rng.permutation(np.arange(-180.0, 180.0, 10.0)):
            trial = chi_p.copy()
            trial[r, 0] = c1
            hit = under(sr.build_chain(seq, phi, psi, omega, trial)[1], CLASH - 0.1)
            new = [h for h in hit if r in (res_of[T["free_i"][h]], res_of[T["free_j"][h]])]
            if len(new) and len(hit) <= len(residues) * 3 + 3:
                chi_p = trial
                residues.append(int(r))
                break
    if len(residues) < n_planted:
        raise ValueError("could not plant")
    return dict(seq=np.array(seq), phi=phi, psi=psi, chi=chi, chi_planted=chi_p, residues=np.array(residues))


def case_tables(top):
    """(metrics.relax_tables(top), the reference's tables over the same quads)."""
    from codlad_amd import metrics
    tab = metrics.relax_tables(top)
    return tab, tables(tab["radius"].numpy(), db.standard_bonds(top).numpy(), tab["quads"].numpy())


# name -> (residues, seed, planted residues, iterations of the test): about 32 and 60 residues, and one over 1 024 atoms (two
# column tiles, five row blocks).  Seeds: the first for which search_planted succeeds AND the float64 reference run meets the
# conditions of tests/test_relax_host.py.
PLANTED = {"r32": (32, 3, 4, 200), "r60": (60, 1, 6, 200), "r140": (140, 0, 8, 200)}
GOLDEN = "relax_planted.npz"


def golden_path():
    import os
    return os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", GOLDEN)


_CASES = {}


def planted_case(key):
    """-> dict: top, xyz0 (clean) and xyz (planted) float32 [n, 3], residues, tab, T, fixed, n_iter - built by
    stereo_ref.build_chain from the angles stored in tests/golden/relax_planted.npz."""
    from tests import stereo_ref as sr
    if key not in _CASES:
        z = np.load(golden_path())
        g = {k: z[f"{key}_{k}"] for k in ("seq", "phi", "psi", "chi", "chi_planted", "residues")}
        seq, n = [str(a) for a in g["seq"]], len(g["seq"])
        top, clean = sr.build_chain(seq, g["phi"], g["psi"], np.full(n, 180.0), g["chi"])
        planted = sr.build_chain(seq, g["phi"], g["psi"], np.full(n, 180.0), g["chi_planted"])[1]
        tab, T = case_tables(top)
        _CASES[key] = dict(top=top, xyz0=clean.astype(np.float32), xyz=planted.astype(np.float32), tab=tab, T=T,
                           residues=g["residues"].tolist(), fixed=tab["fixed"].numpy(), n_iter=PLANTED[key][3])
    return _CASES[key]


if __name__ == "__main__":
    out = {}
    for name, (n_res, seed, n_planted, _n_iter) in PLANTED.items():
        for k, v in search_planted(n_res, seed, n_planted).items():
            out[f"{name}_{k}"] = v
    np.savez_compressed(golden_path(), **out)
    print(golden_path())
