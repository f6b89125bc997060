"""Inputs and float64 references of the ensemble observables (metrics.sasa, contact_map, radius_of_gyration;
codlad_sasa, codlad_contact_counts).

SASA.  `margins` evaluates the header's rule per test point: m = min over j != i of (|e|^2 - R_j^2) with
e = R_i u_k - (x_j - x_i); the point is buried when m < 0.  The same code runs in float64 (the reference, on the float32
inputs converted exactly) and in float32 (numpy: one rounding per operation in the header's order - the sign of a rounded
difference is the sign of the exact one, so m32 < 0 is the kernel's decision).  ref_dev = the largest |m32 - m64| over all
cases; a point with |m64| <= 4 ref_dev is UNDECIDED and the device may fall on either side of it.
The minimum over j is taken over the atoms within R_i + R_j + 1 A first; an atom beyond that has a margin above
2 min(R) + 1, so only points whose minimum so far is larger (isolated ones) look at every atom.  That is the minimum
over all j, cheaper.

Inputs are built in float64 from fixed seeds, rounded to float32, and used as built and translated by SHIFT.  Every
reference is computed once per session (lru_cache) and its arrays are read-only.
"""
import functools

import numpy as np

from tests import stereo_ref as sr

VDW = np.array([1.70, 1.55, 1.52, 1.80])           # C, N, O, S
PROBE = 1.4
SHIFT = np.array([1000.0, -500.0, 250.0])
DENSITY, MIN_SEP = 0.055, 1.2                       # atoms / A^3 of a protein interior; closest pair of a ball
SIZES = (1, 2, 3, 63, 64, 65, 255, 256, 257, 600)   # at 96 points
POINTS = (1, 63, 64, 65, 96, 960, 1024)             # at the atom counts below
POINT_SIZES = (3, 65, 257)
N_STRUCT = 3
CONTACT_SIZES = (1, 2, 64, 65, 257)
CONTACT_STRUCT = 5
CUTOFF = 8.0
CONTACT_MARGIN = 1e-3                               # A^2 on d^2: see contact_case


def sphere_points(n):
    """The golden spiral of metrics.sphere_points, restated: float64, rounded once to float32."""
    k = np.arange(n, dtype=np.float64)
    z = 1.0 - (2.0 * k + 1.0) / n
    phi = k * (np.pi * (3.0 - np.sqrt(5.0)))
    rho = np.sqrt(1.0 - z * z)
    return np.stack([rho * np.cos(phi), rho * np.sin(phi), z], 1).astype(np.float32)


def ball(n, rng):
    """n points in a ball of DENSITY atoms / A^3, no two closer than MIN_SEP (sequential rejection)."""
    rad = (3.0 * n / (4.0 * np.pi * DENSITY)) ** (1.0 / 3.0)
    pts = np.zeros((0, 3))
    while len(pts) < n:
        p = rng.uniform(-rad, rad, 3)
        if p @ p <= rad * rad and (len(pts) == 0 or ((pts - p) ** 2).sum(1).min() >= MIN_SEP ** 2):
            pts = np.vstack([pts, p])
    return pts


def chain(n, seed):
    """The first n atoms of a chain of stereo_ref.build_chain (ideal bonded geometry, random torsions)."""
    n_res = n // 4 + 2                               # GLY, the smallest template, has 4 atoms
    pl = sr.planted(n_res, seed)
    _top, xyz = sr.build_chain(pl["seq"], pl["phi"], pl["psi"], pl["omega"], pl["chi"], pl["d_ca"], pl["d_side"])
    assert xyz.shape[0] >= n
    return xyz[:n]


def residue_table(n):
    """Residues of 7 atoms, a last shorter one, and (n >= 3) one empty residue."""
    cuts = sorted(set(range(0, n, 7)) | {n})
    if n >= 3:
        cuts.insert(1, cuts[1])
    return np.array(cuts, dtype=np.int32)


def margins(x, radius, dirs, dtype):
    """x [n, 3], radius [n], dirs [P, 3] (float32) -> m [n, P] in `dtype`; +inf for a single atom."""
    n, P = x.shape[0], dirs.shape[0]
    x64 = x.astype(np.float64)
    r64 = radius.astype(np.float64)
    far_floor = 2.0 * float(r64.min()) + 1.0
    xs, rs, us = x.astype(dtype), radius.astype(dtype), dirs.astype(dtype)
    rr = rs * rs
    out = np.full((n, P), np.inf, dtype=dtype)

    def over(i, js, pts):
        d = xs[js] - xs[i]                                                     # [J, 3]: the difference first
        e = pts[:, None, :] - d[None]                                          # [P', J, 3]
        return (((e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2]) - rr[js][None]).min(1)

    others = np.arange(n)
    for i in range(n):
        if n == 1:
            break
        pts = rs[i] * us                                                       # [P, 3]
        dist = np.sqrt(((x64 - x64[i]) ** 2).sum(1))
        near = others[(dist < r64[i] + r64 + 1.0) & (others != i)]
        if len(near):
            out[i] = over(i, near, pts)
        lonely = np.nonzero(out[i].astype(np.float64) > 0.5 * far_floor)[0]
        if len(lonely):
            out[i, lonely] = over(i, others[others != i], pts[lonely])
    return out


def _freeze(*arrays):
    for a in arrays:
        a.setflags(write=False)


@functools.lru_cache(maxsize=None)
def sasa_case(kind, n, n_points, shifted):
    """-> dict: x float32 [S, n, 3], vdw float64 [n], radius float32 [n] (vdw + probe), unit float32 [n], dirs float32
    [P, 3], res_ptr int32, m64 / m32 [S, n, P].  S = N_STRUCT, or 1 where n * n_points > 65 * 1024 (the CPU time of the
    reference)."""
    seed = 7919 * n + 31 * n_points + (0 if kind == "ball" else 1)
    rng = np.random.default_rng(seed)
    S = N_STRUCT if n * n_points <= 65 * 1024 else 1
    x = np.stack([ball(n, rng) if kind == "ball" else chain(n, seed + 101 * s) for s in range(S)])
    if shifted:
        x = x + SHIFT
    x = x.astype(np.float32)
    vdw = rng.choice(VDW, n)
    radius = (vdw + PROBE).astype(np.float32)
    unit = (4.0 * np.pi * radius.astype(np.float64) ** 2 / n_points).astype(np.float32)
    dirs = sphere_points(n_points)
    m64 = np.stack([margins(x[s], radius, dirs, np.float64) for s in range(S)])
    m32 = np.stack([margins(x[s], radius, dirs, np.float32) for s in range(S)])
    res_ptr = residue_table(n)
    _freeze(x, vdw, radius, unit, dirs, m64, m32, res_ptr)
    return dict(x=x, vdw=vdw, radius=radius, unit=unit, dirs=dirs, res_ptr=res_ptr, m64=m64, m32=m32)


def sasa_keys():
    """Every (kind, n_atoms, n_points, shifted) of the SASA tests: both kinds at every size at 96 points, and the other
    point counts at POINT_SIZES, kinds alternating."""
    keys = [(kind, n, 96, sh) for n in SIZES for kind in ("chain", "ball") for sh in (False, True)]
    for k, P in enumerate(p for p in POINTS if p != 96):
        keys += [(("ball", "chain")[(k + q) % 2], n, P, sh) for q, n in enumerate(POINT_SIZES) for sh in (False, True)]
    return keys


@functools.lru_cache(maxsize=None)
def ref_dev():
    """The largest |m32 - m64| over all cases (inf - inf of a single atom counts as 0)."""
    worst = 0.0
    for key in sasa_keys():
        c = sasa_case(*key)
        fin = np.isfinite(c["m64"])
        assert (fin == np.isfinite(c["m32"])).all()
        if fin.any():
            worst = max(worst, float(np.abs(c["m32"].astype(np.float64)[fin] - c["m64"][fin]).max()))
    return worst


def sasa_expected(key):
    """-> (exposed int [S, n] of the float64 reference, undecided int [S, n]: the points within 4 ref_dev of the decision)."""
    c = sasa_case(*key)
    return (c["m64"] >= 0).sum(-1), (np.abs(c["m64"]) <= 4.0 * ref_dev()).sum(-1)


# ------------------------------------------------------------------------------------------------------------ contacts
def _d2(x, dtype):
    """[S, m, m] squared distances of x [S, m, 3] in `dtype`, in the order of the kernel."""
    x = x.astype(dtype)
    d = x[:, :, None, :] - x[:, None, :, :]
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def too_close_to_the_cutoff(x):
    """Atoms with a pair whose d^2 (float64) lies within CONTACT_MARGIN of the cut-off's square, per structure."""
    d2 = _d2(x, np.float64)
    bad = np.abs(d2 - float(np.float32(CUTOFF * CUTOFF))) <= CONTACT_MARGIN
    return [np.unique(np.nonzero(b)[1]) for b in bad]


@functools.lru_cache(maxsize=None)
def contact_case(m):
    """-> dict: x float32 [5, m + 37, 3] (a blob of spread 6 A), sel int64 [m] (distinct, unsorted), counts_sel and
    counts_all int [.., ..] (the float64 reference with `sel` and over the first m atoms), dev: the largest
    |d2_32 - d2_64| over pairs below twice the cut-off.  CONTACT_MARGIN: d^2 near 64 A^2 from coordinates below 64 A carries
    a few 2^-24 * d^2 of float32 rounding (each difference of coordinates, each square and the two sums round once: below
    4e-5 A^2 up to d^2 = 256 A^2, measured as `dev`): 1e-3 is 4 x that, six times over.  Atoms with a pair inside the margin are moved."""
    rng = np.random.default_rng(5000 + m)
    n = m + 37
    x = (rng.standard_normal((CONTACT_STRUCT, n, 3)) * 6.0).astype(np.float32)
    for _ in range(50):
        bad = too_close_to_the_cutoff(x)
        if not any(len(b) for b in bad):
            break
        for s, b in enumerate(bad):
            x[s, b] += rng.normal(0, 0.05, (len(b), 3)).astype(np.float32)
    sel = rng.permutation(n)[:m].astype(np.int64)
    cut2 = float(np.float32(CUTOFF * CUTOFF))

    def count(xx):
        c = (_d2(xx, np.float64) < cut2).sum(0)
        np.fill_diagonal(c, 0)
        return c

    d64, d32 = _d2(x, np.float64), _d2(x, np.float32).astype(np.float64)
    dev = float(np.abs(d32 - d64)[d64 < 4 * cut2].max())
    out = dict(x=x, sel=sel, counts_sel=count(x[:, sel]), counts_all=count(x[:, :m]), dev=dev)
    _freeze(x, sel, out["counts_sel"], out["counts_all"])
    return out


# ------------------------------------------------------------------------------------------------- radius of gyration
def rg2(x, sel=None):
    """x [S, n, 3] -> (G / m [S], G [S]) in float64 about the unweighted centroid of `sel` (default: all atoms)."""
    x = np.asarray(x, dtype=np.float64)
    if sel is not None:
        x = x[:, np.asarray(sel)]
    g = ((x - x.mean(1, keepdims=True)) ** 2).sum((1, 2))
    return g / x.shape[1], g
