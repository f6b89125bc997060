"""Reference of the secondary-structure assignment (metrics.hbonds / metrics.dssp, codlad_dssp_hbonds / codlad_dssp_assign).

`stage1` states the first stage - links, amide hydrogens, the Kabsch-Sander energy of every eligible pair, bends - in numpy,
in the operation order the header fixes.  In float64 it is the reference; with dtype=np.float32 it is the float32 restatement
of the same order (one rounding per operation), and the difference of the two on the same inputs is the deviation the
device is allowed four times over.  `assign` is the pattern stage as plain loops over residues, straight from the rule in
include/codlad_hip.h: no bitmaps, no shifts - it shares nothing with the kernel's word arithmetic.

The planted cases are built by `stereo_ref.build_chain` from chosen backbone torsions, so their labels are known by hand:
ideal helices, two strands docked into a ladder by a frozen rigid transform (found by tools/dssp_dock_search.py against
this reference), a stretched link, a PRO, a chain start and an absent O inside a helix.
"""
import functools

import numpy as np

from codlad_amd.utils.cg_input import template_topology
from codlad_amd.utils.dataset_builder import Topology
from tests import stereo_ref as sr

CODES = " HBEGITS"
LOOP, H, B, E, G, I, T, S = range(8)
UNDEFINED = 255
MAX_RES = 4096                                   # CODLAD_DSSP_MAX_RES
KIND_PRO, KIND_CHAIN_START = 1, 2
GEOM_LINK, GEOM_BEND = 1, 2
KS_Q, E_MIN, E_BOND, R_MIN, LINK_MAX, BEND_ABOVE = 27.888, -9.9, -0.5, 0.5, 2.5, 70.0


# ---------------------------------------------------------------------------------------------------------- stage 1
def tables(top):
    """(bb int64 [R, 4] = N, CA, C, O by atom NAME, -1 where the residue lists none; kind uint8 [R]) of a Topology."""
    R = top.n_residues
    bb = np.array([[top.atom(r, a) for a in ("N", "CA", "C", "O")] for r in range(R)], dtype=np.int64).reshape(R, 4)
    kind = np.array([(KIND_PRO if top.res_names[r] == "PRO" else 0) |
                     (KIND_CHAIN_START if r == 0 or top.chain_ids[r - 1] != top.chain_ids[r] else 0) for r in range(R)],
                    dtype=np.uint8)
    return bb, kind


def _dist(a, b):
    d = a - b
    return np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def stage1(xyz, bb, kind, dtype=np.float64):
    """xyz [S, n_atoms, 3] (or [n_atoms, 3]) -> dict, the arithmetic in `dtype` from the coordinates cast to it:
      energy [S, R, R]     E(i -> j), C=O of i with N-H of j; NaN where the pair is not eligible
      eligible, hb [S, R, R] bool;  link, bend [S, R] bool;  d_link [S, R] |C_r - N_{r+1}| where both exist, else NaN
      kappa [S, R];  geom uint8 [S, R];  finite bool [S]
      e_best [S, R, 2], partner int64 [S, R, 2], gap [S, R, 2] (second-lowest minus lowest energy, inf with fewer than two)
    A structure with a non-finite coordinate of a named atom has hb / geom 0, NaN energies and kappa, partners -1."""
    dt = np.dtype(dtype).type
    x_in = np.asarray(xyz)
    x_in = x_in.reshape(-1, x_in.shape[-2], 3)
    n_atoms, R = x_in.shape[1], bb.shape[0]
    present = (bb >= 0) & (bb < n_atoms)
    idx = np.where(present, bb, 0)
    named = np.unique(bb[present])
    finite = np.isfinite(x_in[:, named].astype(np.float64)).all(axis=(1, 2))
    x = x_in.astype(dtype)
    pN, pCA, pC, pO = (x[:, idx[:, k]] for k in range(4))                       # [S, R, 3]
    hasN, hasCA, hasC, hasO = (present[:, k] for k in range(4))
    pro, start = (kind & KIND_PRO) > 0, (kind & KIND_CHAIN_START) > 0
    S_ = x.shape[0]
    with np.errstate(all="ignore"):
        d_link = np.full((S_, R), np.nan, dtype=dtype)
        can = np.zeros(R, bool)
        can[:-1] = ~start[1:] & hasC[:-1] & hasN[1:]
        d_link[:, :-1] = _dist(pC[:, :-1], pN[:, 1:])
        d_link[:, ~can] = np.nan
        link = can[None] & (d_link <= dt(LINK_MAX))
        has_h = np.zeros((S_, R), bool)
        has_h[:, 1:] = link[:, :-1] & (~pro[1:] & hasN[1:] & hasC[:-1] & hasO[:-1])[None]
        pH = np.zeros_like(pN)
        dv = pC[:, :-1] - pO[:, :-1]
        ln = np.sqrt(_dot(dv, dv))
        pH[:, 1:] = pN[:, 1:] + dv / ln[..., None]
        r_on = _dist(pO[:, :, None], pN[:, None, :])
        r_ch = _dist(pC[:, :, None], pH[:, None, :])
        r_oh = _dist(pO[:, :, None], pH[:, None, :])
        r_cn = _dist(pC[:, :, None], pN[:, None, :])
        one = dt(1.0)
        en = dt(KS_Q) * (((one / r_on + one / r_ch) - one / r_oh) - one / r_cn)
        en = np.where(en < dt(E_MIN), dt(E_MIN), en)
        close = (r_on < dt(R_MIN)) | (r_ch < dt(R_MIN)) | (r_oh < dt(R_MIN)) | (r_cn < dt(R_MIN))
        en = np.where(close, dt(E_MIN), en)
        ii, jj = np.arange(R)[:, None], np.arange(R)[None, :]
        eligible = (ii != jj)[None] & (hasC & hasO)[None, :, None] & has_h[:, None, :] & \
            ~((jj == ii + 1)[None] & link[:, :, None])
        eligible &= finite[:, None, None]
        energy = np.where(eligible, en, dt(np.nan))
        hb = eligible & (energy < dt(E_BOND))
        # bends
        kappa = np.full((S_, R), np.nan, dtype=dtype)
        if R >= 5:
            u, v = pCA[:, 2:-2] - pCA[:, :-4], pCA[:, 4:] - pCA[:, 2:-2]
            cs = _dot(u, v) / np.sqrt(_dot(u, u) * _dot(v, v))
            cs = np.where(cs > one, one, np.where(cs < -one, -one, cs))
            k = np.arccos(cs) * dt(180.0 / np.pi)
            ok = link[:, :-4] & link[:, 1:-3] & link[:, 2:-2] & link[:, 3:-1] & (hasCA[:-4] & hasCA[2:-2] & hasCA[4:])[None]
            kappa[:, 2:-2] = np.where(ok, k, dt(np.nan))
        kappa[~finite] = np.nan
        link = link & finite[:, None]
        bend = kappa > dt(BEND_ABOVE)
    geom = (GEOM_LINK * link + GEOM_BEND * bend).astype(np.uint8)
    e_best, partner, gap = (np.zeros((S_, R, 2), dtype=dtype), np.full((S_, R, 2), -1, dtype=np.int64),
                            np.full((S_, R, 2), np.inf))
    for col, mat in ((0, energy), (1, energy.transpose(0, 2, 1))):
        m = np.where(np.isnan(mat), np.inf, mat.astype(np.float64))
        best = m.argmin(-1)                                                       # the first minimum: the lowest j
        val = np.take_along_axis(m, best[..., None], -1)[..., 0]
        have = np.isfinite(val)
        partner[..., col] = np.where(have, best, -1)
        e_best[..., col] = np.where(have, np.take_along_axis(mat, best[..., None], -1)[..., 0], dt(0.0))
        if R >= 2:
            two = np.sort(m, -1)[..., :2]
            with np.errstate(invalid="ignore"):
                gap[..., col] = np.where(np.isfinite(two[..., 1]), two[..., 1] - two[..., 0], np.inf)
    e_best[~finite] = np.nan
    partner[~finite] = -1
    return dict(energy=energy, eligible=eligible, hb=hb, link=link, bend=bend, d_link=d_link, kappa=kappa, geom=geom,
                finite=finite, e_best=e_best, partner=partner, gap=gap)


def pack_bits(hb):
    """hb bool [..., R, R] -> (acc, don) uint64 [..., R, W]: bit j of row i of acc is hb[i, j], of don hb[j, i]."""
    hb = np.asarray(hb, bool)
    R = hb.shape[-1]
    W = (R + 63) // 64

    def pack(m):
        pad = np.zeros(m.shape[:-1] + (W * 64,), bool)
        pad[..., :R] = m
        weights = np.uint64(1) << np.arange(64, dtype=np.uint64)
        return (pad.reshape(m.shape[:-1] + (W, 64)).astype(np.uint64) * weights).sum(-1, dtype=np.uint64)

    return pack(hb), pack(np.swapaxes(hb, -1, -2))


def unpack_bits(words, R):
    """uint64 [..., R, W] -> bool [..., R, R]."""
    words = np.asarray(words).astype(np.uint64)
    bits = (words[..., None] >> np.arange(64, dtype=np.uint64)) & np.uint64(1)
    return bits.reshape(words.shape[:-1] + (-1,))[..., :R].astype(bool)


# ---------------------------------------------------------------------------------------------------------- stage 2
def assign(hb, link, bend, sparse=False):
    """hb bool [R, R] (hb[i, j] = Hbond(i -> j)), link bool [R] (r to r+1), bend bool [R] -> (ss uint8 [R], bridge int32
    [R, 2], counts int32 [8]).  Plain loops, in the order of the rule.  sparse: the bridge loop of residue i visits only
    the j that can pass its test - every term of Bridge(i, j) is a bond between one of i - 1, i, i + 1 and one of j - 1, j,
    j + 1 - which makes R = 4096 a matter of seconds; tests/test_size_limits_host.py holds it to the full loop."""
    hb, link, bend = np.asarray(hb, bool), np.asarray(link, bool), np.asarray(bend, bool)
    R = hb.shape[0]

    def partners(i):
        if not sparse:
            return range(R)
        rows = slice(max(i - 1, 0), i + 2)
        near = np.nonzero(hb[rows].any(0) | hb[:, rows].any(1))[0]
        return sorted({int(j) + d for j in near for d in (-1, 0, 1) if 0 <= j + d < R})

    def bond(i, j):
        return 0 <= i < R and 0 <= j < R and bool(hb[i, j])

    def lk(r):
        return 0 <= r < R - 1 and bool(link[r])

    turn = {n: [bond(i, i + n) and all(lk(i + q) for q in range(n)) for i in range(R)] for n in (3, 4, 5)}
    ss = [LOOP] * R
    for i in range(1, R):
        if turn[4][i - 1] and turn[4][i]:
            for q in range(4):
                ss[i + q] = H
    par, anti = [set() for _ in range(R)], [set() for _ in range(R)]
    for i in range(R):
        if not (lk(i - 1) and lk(i)):
            continue
        for j in partners(i):
            if abs(i - j) < 3 or not (lk(j - 1) and lk(j)):
                continue
            if (bond(i - 1, j) and bond(j, i + 1)) or (bond(j - 1, i) and bond(i, j + 1)):
                par[i].add(j)
            if (bond(i, j) and bond(j, i)) or (bond(i - 1, j + 1) and bond(j - 1, i + 1)):
                anti[i].add(j)

    def has(sets, i, j):
        return 0 <= i < R and j in sets[i]

    for i in range(R):
        cont = any(has(par, i - 1, j - 1) or has(par, i + 1, j + 1) for j in par[i]) or \
            any(has(anti, i - 1, j + 1) or has(anti, i + 1, j - 1) for j in anti[i])
        if ss[i] != H:
            if cont:
                ss[i] = E
            elif par[i] or anti[i]:
                ss[i] = B
    for n, code in ((3, G), (5, I)):
        for i in range(1, R):
            if turn[n][i - 1] and turn[n][i] and all(ss[i + q] in (LOOP, code) for q in range(n)):
                for q in range(n):
                    ss[i + q] = code
    for i in range(R):
        if ss[i] == LOOP and any(turn[n][i - k] for n in (3, 4, 5) for k in range(1, n) if i - k >= 0):
            ss[i] = T
    for i in range(R):
        if ss[i] == LOOP and bend[i]:
            ss[i] = S
    bridge = np.array([[min(par[i]) if par[i] else -1, min(anti[i]) if anti[i] else -1] for i in range(R)], dtype=np.int32)
    ss = np.array(ss, dtype=np.uint8)
    return ss, bridge.reshape(R, 2), np.bincount(ss, minlength=8).astype(np.int32)


def assign_batch(hb, geom, finite, sparse=False):
    """The pattern stage for S structures from bitmaps-as-matrices hb [S, R, R], geom [S, R], finite [S]."""
    S_, R = geom.shape
    ss, bridge, counts = (np.full((S_, R), UNDEFINED, np.uint8), np.full((S_, R, 2), -1, np.int32),
                          np.full((S_, 8), -1, np.int32))
    for s in range(S_):
        if finite[s]:
            ss[s], bridge[s], counts[s] = assign(hb[s], (geom[s] & GEOM_LINK) > 0, (geom[s] & GEOM_BEND) > 0, sparse)
    return ss, bridge, counts


def labels(ss):
    return "".join(CODES[c] if c < 8 else "?" for c in ss)


def reference(xyz, top, dtype=np.float64):
    """Both stages -> stage1's dict plus ss [S, R], bridge, counts, ss_string."""
    bb, kind = tables(top)
    out = stage1(xyz, bb, kind, dtype)
    out["ss"], out["bridge"], out["counts"] = assign_batch(out["hb"], out["geom"], out["finite"])
    out["ss_string"] = [labels(s) for s in out["ss"]]
    return out


# ---------------------------------------------------------------------------------------------------- planted cases
HELIX = {"alpha": (-57.0, -47.0), "310": (-49.0, -26.0), "pi": (-57.0, -70.0)}
STRAND = {"anti": (-139.0, 135.0), "par": (-119.0, 113.0)}
# the rigid transform x' = rot(rotvec) x + shift of the second strand (as build_chain leaves it, 40 A away) that docks it
# onto the first: found by tools/dssp_dock_search.py, a hill climb on the clipped Kabsch-Sander energy of the wanted bonds
DOCK = {
    # smallest |E + 0.5| over all eligible pairs 0.1364 (anti) and 0.0439 (par: the strand's own i -> i + 2 pairs at -0.5439,
    # bonds that are no turn and no bridge)
    "anti": ((1.2101552157043491, -1.692315360560959, -2.3544747417333256),
             (34.379208011836766, 32.05865503822696, -34.006039264098725)),
    "par": ((-0.009451565891383594, 0.02048108886871499, -0.054873216403683506),
            (-3.3046737484870268, -37.707700724889015, -4.0398322671405005)),
}
DOCK_BONDS = {"anti": ((0, 13), (2, 11), (4, 9), (7, 6), (9, 4), (11, 2)),
              "par": ((0, 8), (2, 10), (4, 12), (8, 2), (10, 4), (12, 6))}


def rotation(rotvec):
    v = np.asarray(rotvec, dtype=np.float64)
    t = np.linalg.norm(v)
    if t == 0:
        return np.eye(3)
    k = v / t
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(t) * K + (1 - np.cos(t)) * (K @ K)


def chain(seq, phi, psi, chain_breaks=()):
    n = len(seq)
    phi = np.broadcast_to(np.asarray(phi, np.float64), (n,))
    psi = np.broadcast_to(np.asarray(psi, np.float64), (n,))
    return sr.build_chain(list(seq), phi, psi, np.full(n, 180.0), np.full((n, 4), 180.0), chain_breaks=chain_breaks)


def helix(kind, n=14, seq=None):
    phi, psi = HELIX[kind]
    return chain(seq or ["ALA"] * n, phi, psi)


def strands(kind, dock=None, n=7):
    """Two n-residue strands as two chains, the second moved by the rigid transform `dock` (default: the frozen one)."""
    phi, psi = STRAND[kind]
    top, x = chain(["ALA"] * (2 * n), phi, psi, chain_breaks=(n,))
    rotvec, shift = DOCK[kind] if dock is None else dock
    a = int(top.first_atom[n])
    x = x.copy()
    x[a:] = x[a:] @ rotation(rotvec).T + np.asarray(shift, np.float64)
    return top, x


def stretched(top, x, r, length=3.0):
    """Residues r .. move rigidly along C_{r-1} -> N_r until |C_{r-1} - N_r| = length."""
    c, n = x[top.atom(r - 1, "C")], x[top.atom(r, "N")]
    d = n - c
    x = x.copy()
    x[int(top.first_atom[r]):] += d / np.linalg.norm(d) * (length - np.linalg.norm(d))
    return x


def without_atom(top, x, r, name):
    """The topology and coordinates with atom `name` of residue r taken out."""
    names = [list(a) for a in top.atom_names]
    names[r].remove(name)
    keep = np.ones(top.n_atoms, bool)
    keep[top.atom(r, name)] = False
    return Topology(top.res_names, names, top.res_seqs, top.chain_ids), x[keep]


@functools.lru_cache(maxsize=None)
def planted():
    """name -> (Topology, xyz float32 [n_atoms, 3], the hand-derived label string)."""
    out = {}
    helix14 = " " + "H" * 12 + " "
    for kind, code in (("alpha", "H"), ("310", "G"), ("pi", "I")):
        top, x = helix(kind)
        out["helix_" + kind] = (top, x, " " + code * 12 + " ")
    for kind in ("anti", "par"):
        top, x = strands(kind)
        out["sheet_" + kind] = (top, x, " EEEEE  EEEEE ")
    # helix - break - helix: 4-turns 0 .. 10 and 15 .. 25, the link 14 -> 15 stretched to 3 A
    top, x = helix("alpha", 30)
    out["helix_break_helix"] = (top, stretched(top, x, 15), " " + "H" * 13 + "  " + "H" * 13 + " ")
    # a PRO at 7 has no amide H: turn_4(3) goes, the two consecutive pairs around it still cover 1 .. 12
    top, x = helix("alpha", 14, ["ALA"] * 7 + ["PRO"] + ["ALA"] * 6)
    out["helix_pro"] = (top, x, helix14)
    # a chain start at 7 inside an unbroken helix: 4-turns 0 .. 2 and 7 .. 9 only
    top, x = helix("alpha")
    out["helix_chain_start"] = (template_topology(top.res_names, chain_ids=[0] * 7 + [1] * 7), x, " HHHHH  HHHHH ")
    # no O in residue 5: no C=O of 5 and no H of 6, turn_4(5) and turn_4(2) go, the remaining pairs still cover 1 .. 12
    top, x = helix("alpha")
    top, x = without_atom(top, x, 5, "O")
    out["helix_no_o"] = (top, x, helix14)
    return {k: (t, np.ascontiguousarray(x, dtype=np.float32), s) for k, (t, x, s) in out.items()}


# cases by size: what the first stage is held to on the device
SIZES = (5, 63, 64, 65, 130)
NOISE, NOISE_COPIES = 0.3, 4
SIZED_SEED = {5: 1, 63: 1, 64: 1, 65: 1, 130: 1, 257: 1, 513: 1, 1025: 1, 4096: 1}
# beyond one trip of the kernels' per-residue loops (256 threads), and CODLAD_DSSP_MAX_RES itself (tests/test_size_limits.py):
# size -> noisy copies beside the planted structure.  4096 takes 2 GB of host memory per structure in margins()
LIMIT_SIZES = {257: NOISE_COPIES, 1025: NOISE_COPIES, 4096: 1}


@functools.lru_cache(maxsize=None)
def sized(R):
    """(Topology, xyz float32 [n_atoms, 3]) of R residues cycling through the 22 templates (PRO and GLY among them):
    alternating alpha / 3-10 / pi helices of 9-14 residues joined by two extended residues, a chain start in the middle and a
    link stretched to 3 A a quarter of the way in."""
    rng = np.random.default_rng(100 * R + SIZED_SEED[R])
    seq = [sr.RES22[(i + 3) % 22] for i in range(R)]
    phi, psi = np.empty(R), np.empty(R)
    i, k = 0, 0
    while i < R:
        n = int(rng.integers(9, 15))
        phi[i:i + n], psi[i:i + n] = HELIX[("alpha", "310", "pi")[k % 3]]
        phi[i + n:i + n + 2], psi[i + n:i + n + 2] = rng.uniform(-150, -90, 2)[:R - i - n], rng.uniform(110, 160, 2)[:R - i - n]
        i, k = i + n + 2, k + 1
    breaks = (R // 2,) if R >= 10 else ()
    top, x = chain(seq, phi, psi, chain_breaks=breaks)
    if R >= 20:
        x = _stretch_first_chain(top, x, R // 4, R // 2)
    return top, np.ascontiguousarray(x, dtype=np.float32)


def _stretch_first_chain(top, x, r, end):
    """stretched() for the residues r .. end - 1 only (the first chain; the second one stays where it is)."""
    c, n = x[top.atom(r - 1, "C")], x[top.atom(r, "N")]
    d = n - c
    x = x.copy()
    x[int(top.first_atom[r]):int(top.first_atom[end])] += d / np.linalg.norm(d) * (3.0 - np.linalg.norm(d))
    return x


def noisy(x, seed, copies=NOISE_COPIES):
    """float32 [copies, n_atoms, 3]: x + N(0, NOISE A) per coordinate."""
    rng = np.random.default_rng(seed)
    return (x[None].astype(np.float64) + rng.normal(0.0, NOISE, (copies,) + x.shape)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def limit_call(R):
    """The inputs of one call at a size of LIMIT_SIZES, with the references: (Topology, xyz [1 + copies, n_atoms, 3] read-only,
    margins).  Computed once per session."""
    top, x = sized(R)
    xyz = np.concatenate([x[None], noisy(x, 7 * R, LIMIT_SIZES[R])])
    xyz.setflags(write=False)
    return top, xyz, margins(xyz, top)


def margins(xyz, top):
    """The float64 reference, the float32 restatement and what separates them on xyz [S, n_atoms, 3] -> dict:
    r64, r32; dev_e / dev_k / dev_d = max |32 - 64| of the eligible energies, the defined kappas, the link distances;
    undecided_e [S, R, R], undecided_k, undecided_d [S, R]: within 4 x that deviation of the threshold."""
    bb, kind = tables(top)
    r64, r32 = stage1(xyz, bb, kind, np.float64), stage1(xyz, bb, kind, np.float32)
    out = dict(r64=r64, r32=r32)
    with np.errstate(invalid="ignore"):
        for key, name, thr in (("e", "energy", E_BOND), ("k", "kappa", BEND_ABOVE), ("d", "d_link", LINK_MAX)):
            a, b = r64[name], r32[name].astype(np.float64)
            both = np.isfinite(a) & np.isfinite(b)
            dev = float(np.abs(a - b)[both].max()) if both.any() else 0.0
            out["dev_" + key] = dev
            out["undecided_" + key] = np.isfinite(a) & (np.abs(a - thr) <= 4.0 * dev)
            out["min_" + key] = float(np.abs(a - thr)[np.isfinite(a)].min()) if np.isfinite(a).any() else np.inf
    return out


# ------------------------------------------------------------------------------------------ hand-written bitmaps (stage 2)
def handmade(R):
    """R = 130 or 200 -> (hb bool [R, R], link bool [R], bend bool [R], checks: {residue: label} derived by hand).
    An antiparallel and a parallel ladder whose partners straddle a word boundary (63 / 64 and 127 / 128, swapped between
    the two sizes), a bridge with |i - j| = 2, a bridge across a broken link, G next to H (and a G refused by an H), two
    overlapping I, left-over T and S."""
    b_anti, b_par = (64, 128) if R == 130 else (128, 64)
    hb = np.zeros((R, R), bool)
    link = np.ones(R, bool)
    link[R - 1] = False
    bend = np.zeros(R, bool)
    checks = {}
    # antiparallel: bridges (10 + k, b_anti + 2 - k), k = 0 .. 6; the even ones planted as mutual bonds, the odd ones follow
    for k in (0, 2, 4, 6):
        i, j = 10 + k, b_anti + 2 - k
        hb[i, j] = hb[j, i] = True
    for k in range(7):
        checks[10 + k] = checks[b_anti + 2 - k] = "E"
    checks[9] = checks[17] = checks[b_anti + 3] = checks[b_anti - 5] = " "
    # parallel: bridges (20 + k, b_par - 4 + k), k = 0 .. 4; the even ones planted as i-1 -> j, j -> i+1
    for k in (0, 2, 4):
        i, j = 20 + k, b_par - 4 + k
        hb[i - 1, j] = hb[j, i + 1] = True
    for k in range(5):
        checks[20 + k] = checks[b_par - 4 + k] = "E"
    # |i - j| = 2: refused
    hb[40, 42] = hb[42, 40] = True
    checks[40] = checks[41] = checks[42] = " "
    # across a broken link 50 -> 51: (50, 90) and (51, 89) refused, (52, 88) stands alone
    hb[50, 90] = hb[90, 50] = hb[52, 88] = hb[88, 52] = True
    link[50] = False
    checks.update({50: " ", 51: " ", 52: "B", 88: "B", 89: " ", 90: " "})
    # H from 4-turns 100 .. 103; 3-turns 106 .. 108 give G 107 .. 110 right after it; 3-turns 99, 100 are refused by the H
    for i in (100, 101, 102, 103):
        hb[i, i + 4] = True
    for i in (99, 100, 106, 107, 108):
        hb[i, i + 3] = True
    checks.update({100: "T", **{r: "H" for r in range(101, 107)}, **{r: "G" for r in range(107, 111)}})
    # 5-turns 112 .. 114: I 113 .. 117 and 114 .. 118 overlap
    for i in (112, 113, 114):
        hb[i, i + 5] = True
    checks.update({r: "I" for r in range(113, 119)})
    # left-overs: a lone 4-turn at 30 gives T 31 .. 33 (a bend inside it stays T), a lone bend at 45 gives S
    hb[30, 34] = True
    bend[32] = bend[45] = True
    checks.update({30: " ", 31: "T", 32: "T", 33: "T", 34: " ", 45: "S"})
    return hb, link, bend, checks


HIGH_KINDS = ("a", "b")


def handmade_high(R, kind):
    """R >= 4040, kind "a" or "b" -> (hb, link, bend, checks) as handmade(): the word logic at high word indices and the
    borders between the trips of the kernel's per-residue loops (256 residues a trip).
      a: an antiparallel ladder between word 0 and words 62 / 63 whose partners straddle bits 4031 / 4032, a parallel one
         whose partners straddle 255 / 256, a G run across 511 / 512, an I run across 767 / 768, an H run across 1023 / 1024
      b: the parallel ladder at 4031 / 4032 and the antiparallel one at 1279 / 1280, an H run across 255 / 256 and one across
         2047 / 2048, a G run across 511 / 512, a lone 4-turn at 767 whose T lie in the next trip (768 .. 770, a bend inside
         it stays T), a bend that gives S at 3000"""
    assert R >= 4040 and kind in HIGH_KINDS
    b_anti, b_par = (4032, 256) if kind == "a" else (1280, 4032)
    hb = np.zeros((R, R), bool)
    link = np.ones(R, bool)
    link[R - 1] = False
    bend = np.zeros(R, bool)
    checks = {}
    # the two ladders of handmade(): rows 10 .. 16 and 20 .. 24, both in word 0
    for k in (0, 2, 4, 6):
        i, j = 10 + k, b_anti + 2 - k
        hb[i, j] = hb[j, i] = True
    for k in range(7):
        checks[10 + k] = checks[b_anti + 2 - k] = "E"
    checks[9] = checks[17] = checks[b_anti + 3] = checks[b_anti - 5] = " "
    for k in (0, 2, 4):
        i, j = 20 + k, b_par - 4 + k
        hb[i - 1, j] = hb[j, i + 1] = True
    for k in range(5):
        checks[20 + k] = checks[b_par - 4 + k] = "E"
    checks[b_par - 5] = checks[b_par + 1] = " "

    def run(first, last, n, code):
        """n-turns at first .. last: the run of `code` over first + 1 .. last + n - 1, loop on both sides of the turns' reach."""
        for i in range(first, last + 1):
            hb[i, i + n] = True
        checks.update({r: code for r in range(first + 1, last + n)})
        checks[first] = " "
        checks[last + n] = " "

    if kind == "a":
        run(508, 512, 3, "G")
        run(764, 768, 5, "I")
        run(1019, 1027, 4, "H")
    else:
        run(250, 258, 4, "H")
        run(508, 512, 3, "G")
        run(2043, 2051, 4, "H")
        hb[767, 771] = True                    # a lone 4-turn: T 768 .. 770
        bend[769] = bend[3000] = True
        checks.update({767: " ", 768: "T", 769: "T", 770: "T", 771: " ", 3000: "S"})
    return hb, link, bend, checks


def random_maps(R, seed):
    """Random bitmaps: bonds i -> i + 3 / 4 / 5 in runs, a sprinkling of long-range bonds dense enough to make ladders, a
    few broken links and bends."""
    rng = np.random.default_rng(seed)
    hb = rng.random((R, R)) < 0.03
    for n in (3, 4, 5):
        on = rng.random(R) < 0.5
        for i in range(R - n):
            hb[i, i + n] |= on[i] or (i > 0 and on[i - 1] and rng.random() < 0.7)
    for _ in range(R // 8):                                  # short ladders at random places
        i, j, anti = int(rng.integers(1, R - 8)), int(rng.integers(1, R - 8)), bool(rng.integers(2))
        for k in range(0, 6, 2):
            if anti and j - k >= 0:
                hb[i + k, j - k] = hb[j - k, i + k] = True
            elif not anti:
                hb[i + k - 1, j + k] = hb[j + k, i + k + 1] = True
    np.fill_diagonal(hb, False)
    link = rng.random(R) > 0.05
    link[R - 1] = False
    return hb, link, rng.random(R) < 0.2
