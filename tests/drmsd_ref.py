"""References for the dRMSD kernels (codlad_drmsd_matrix, codlad_drmsd_pairs), numpy only: the float32 restatement of the
pair distance (pair_hist_kernels.hip's sequence), the msd as the DIRECT sum of squared differences of those distances in
np.longdouble (never the Gram form), the kernel's pair order as a plain loop, the pools the tests run on, and the error
bounds, which are read from the macros of include/codlad_hip.h and restated from their parts (none is fitted)."""
import functools
import os
import re

import numpy as np

from tests.polymer_ref import walk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "codlad_hip.h")).read()
LD = np.longdouble
EPS = 2.220446049250313e-16                            # 2^-52, the factor of every bound macro


def macro(name):
    """The value of the plain integer macro CODLAD_DRMSD_<name>."""
    m = re.search(r"^#define CODLAD_DRMSD_" + name + r" ([0-9]+)$", HEADER, re.M)
    assert m, name
    return int(m.group(1))


def bound_macro(name, arg):
    """The text of the function macro CODLAD_DRMSD_<name>(arg)."""
    m = re.search(r"^#define CODLAD_DRMSD_" + name + r"\(" + arg + r"\) (.+)$", HEADER, re.M)
    assert m, name
    return m.group(1)


MAX_SEL, WINDOW, SLAB_TILES = macro("MAX_SEL"), macro("WINDOW"), macro("SLAB_TILES")
SPLIT_MAX_BLOCKS, SCRATCH_BUDGET = macro("SPLIT_MAX_BLOCKS"), macro("SCRATCH_BUDGET")
BLOCK = 64                                             # structures of a block: the bits of a bitmap word


def _c_value(text, var, v):
    """A bound macro's C expression at v: `/` between integers is C's integer division."""
    expr = text.replace("((m) + 63) / 64", "((m) + 63) // 64").replace("((m) + 3) / 4", "((m) + 3) // 4")
    assert re.fullmatch(r"[0-9" + var + r"()+\-*/. e]+", expr), text
    return float(eval(expr, {"__builtins__": {}}, {var: int(v)}))


def n_pairs(m, min_sep=1):
    return (m - min_sep) * (m - min_sep + 1) // 2


def matrix_bound(P):
    """|msd - exact| / ((G_i + G_j + 2 C_ij) / P): one rounding per accumulated product, two additions, the division."""
    v = _c_value(bound_macro("MATRIX_BOUND", "P"), "P", P)
    assert v == (P + 2 + 1) * EPS
    return v


def pairs_bound(m):
    """|msd - exact| / exact of the pair route: term 2, lane ceil(m / 64), butterfly 6, wave ceil(m / 4), waves 3, division 1."""
    v = _c_value(bound_macro("PAIRS_BOUND", "m"), "m", m)
    assert v == (2 + (m + 63) // 64 + 6 + (m + 3) // 4 + 3 + 1) * EPS
    return v


def position_bound(m):
    v = _c_value(bound_macro("POSITION_BOUND", "m"), "m", m)
    assert v == (2 + (m + 63) // 64 + 6 + 1) * EPS
    return v


# ------------------------------------------------------------------------------------------------- the pair order --
def pair_order(m, min_sep=1):
    """The kernel's pair order, a plain loop -> (list of (k, l), list of the slab of every pair): windows of WINDOW x WINDOW
    positions on or above the diagonal row by row, a window's slots row by row; SLAB_TILES consecutive windows a slab."""
    T = (m + WINDOW - 1) // WINDOW
    pairs, slabs, tile = [], [], 0
    for tr in range(T):
        for tc in range(tr, T):
            for k in range(tr * WINDOW, min((tr + 1) * WINDOW, m)):
                for l in range(tc * WINDOW, min((tc + 1) * WINDOW, m)):
                    if l - k >= min_sep:
                        pairs.append((k, l))
                        slabs.append(tile // SLAB_TILES)
            tile += 1
    return pairs, slabs


def n_slabs(m):
    T = (m + WINDOW - 1) // WINDOW
    return (T * (T + 1) // 2 + SLAB_TILES - 1) // SLAB_TILES


def n_blocks(Na, Nb=0):
    a, b = (Na + BLOCK - 1) // BLOCK, (Nb + BLOCK - 1) // BLOCK
    return a * b if Nb else a * (a + 1) // 2


def groups(Na, Nb, m):
    """The split rule of the header: the workgroups per block."""
    s, b = n_slabs(m), n_blocks(Na, Nb)
    return s if s > 1 and b < SPLIT_MAX_BLOCKS and b * s * BLOCK * BLOCK * 8 <= SCRATCH_BUDGET else 1


# ------------------------------------------------------------------------------------------------------ references --
def picked(x, sel):
    return x if sel is None else x[:, np.asarray(sel, dtype=np.int64)]


def distances(x, sel=None, min_sep=1):
    """x float32 [N, n, 3] -> float32 [N, P]: d = sqrt((dx*dx + dy*dy) + dz*dz) of every pair in float32, one rounding per
    operation, separation by separation (the direct sums below do not care about the order)."""
    p = np.ascontiguousarray(picked(x, sel), dtype=np.float32)
    m = p.shape[1]
    out = []
    with np.errstate(invalid="ignore", over="ignore"):
        for s in range(min_sep, m):
            d = p[:, s:] - p[:, :m - s]
            assert d.dtype == np.float32
            out.append(np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]))
    D = np.concatenate(out, 1)
    assert D.dtype == np.float32 and D.shape[1] == n_pairs(m, min_sep)
    return D


def finite_of(x, sel=None):
    return np.isfinite(picked(x, sel)).all(axis=(1, 2))


def msd_cross(Da, Db, fa=None, fb=None):
    """-> (msd, scale) longdouble [Na, Nb]: the direct sum of (d(a) - d(b))^2 / P, and sum (d(a) + d(b))^2 / P = (G_a + G_b
    + 2 C_ab) / P, what the matrix bound multiplies.  Rows / columns of structures that are not finite are NaN."""
    Na, P = Da.shape
    msd, scale = np.zeros((Na, Db.shape[0]), dtype=LD), np.zeros((Na, Db.shape[0]), dtype=LD)
    with np.errstate(invalid="ignore", over="ignore"):
        for p0 in range(0, P, 1 << 20):                    # a million pairs at a time: the tables stay small
            A, B = Da[:, p0:p0 + (1 << 20)].astype(LD), Db[:, p0:p0 + (1 << 20)].astype(LD)
            for i in range(Na):
                msd[i] += ((B - A[i]) ** 2).sum(1)
                scale[i] += ((B + A[i]) ** 2).sum(1)
        msd /= LD(P)
        scale /= LD(P)
    if fa is not None:
        msd[~fa], scale[~fa] = np.nan, np.nan
    if fb is not None:
        msd[:, ~fb], scale[:, ~fb] = np.nan, np.nan
    return msd, scale


def worst(got, msd, scale, bound):
    """The largest |got - msd| / (bound * scale) over the elements with a finite reference (0 / 0 on a diagonal counts as 0)."""
    got = np.asarray(got).astype(LD)
    ok = np.isfinite(msd)
    err, lim = np.abs(got - msd)[ok], (LD(bound) * scale)[ok]
    with np.errstate(invalid="ignore", divide="ignore"):
        f = np.where(err == 0, LD(0), err / lim)
    return float(f.max()) if f.size else 0.0


def position_ld(da_full, db_full, m, min_sep):
    """Per chain position the mean of (d_kl(a) - d_kl(b))^2 over the partners l, from the [m, m] distance tables."""
    diff2 = (da_full.astype(LD) - db_full.astype(LD)) ** 2
    k = np.arange(m)
    partner = np.abs(k[:, None] - k[None, :]) >= min_sep
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(partner, diff2, LD(0)).sum(1) / partner.sum(1).astype(LD)


def table32(xs):
    """One structure [m, 3] float32 -> its [m, m] float32 distance table, the same sequence (the sign of dx does not matter)."""
    d = xs[None, :, :] - xs[:, None, :]
    return np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])


# ----------------------------------------------------------------------------------------------------------- pools --
def rods(m):
    """float32 [3, m, 3]: beads at (k, 0, 0), (2 k, 0, 0) and (0, 3 k, 0): distances s, 2 s and 3 s, all integers."""
    x = np.zeros((3, m, 3), dtype=np.float32)
    k = np.arange(m)
    x[0, :, 0], x[1, :, 0], x[2, :, 1] = k, 2 * k, 3 * k
    return x


def rods_msd(m, min_sep=1):
    """float64 [3, 3] by hand: sum_s (m - s) s^2 / P times (1, 4, 1) for the pairs (0, 1), (0, 2), (1, 2): integers over P."""
    S = sum((m - s) * s * s for s in range(min_sep, m))
    P = n_pairs(m, min_sep)
    out = np.zeros((3, 3))
    out[0, 1] = out[1, 0] = float(S) / float(P)
    out[0, 2] = out[2, 0] = float(4 * S) / float(P)
    out[1, 2] = out[2, 1] = float(S) / float(P)
    return out


def mirrored(x):
    y = x.copy()
    y[..., 0] = -y[..., 0]
    return y


def translated(x):
    """-> (the pool on a grid of 2^-10, the same moved by a vector of that grid): coordinates below 2^10 in size on that
    grid take 20 bits, so the translation is exact in fp32 and every coordinate difference keeps its bits."""
    assert np.abs(x).max() < 512.0
    q = np.round(x * 1024.0) / 1024.0
    return q.astype(np.float32), (q + np.array([64.0, -128.0, 32.0])).astype(np.float32)


def rotations(n, seed):
    rng = np.random.default_rng(seed)
    q, _ = np.linalg.qr(rng.normal(size=(n, 3, 3)))
    q[:, :, 0] *= np.sign(np.linalg.det(q))[:, None]
    return q


def planted(m=87, copies=(9, 7, 5), seed=0, rotate=True):
    """Three conformations, `copies` noisy copies of each (fp32 noise of 0.01 A), shuffled; with rotate every copy is
    turned by a rotation of its own -> (x float32 [N, m, 3], membership int [N])."""
    rng = np.random.default_rng(seed)
    base = walk(3, m, seed=seed + 50).astype(np.float64)
    xs, member = [], []
    rots = rotations(sum(copies), seed + 1)
    for c, n in enumerate(copies):
        for _ in range(n):
            y = base[c] + rng.normal(0.0, 0.01, (m, 3))
            if rotate:
                y = y @ rots[len(xs)].T
            xs.append(y)
            member.append(c)
    order = rng.permutation(len(xs))
    return np.ascontiguousarray(np.array(xs)[order].astype(np.float32)), np.array(member)[order]


@functools.lru_cache(maxsize=None)
def case(N, m, min_sep=1, kind="all"):
    """A pool and its references, computed once and frozen: kind "all", "subset" (an ascending selection of m of m + 9
    atoms) or "descending"."""
    n_extra = 9 if kind == "subset" else 0
    x = walk(N, m, n_extra=n_extra)
    sel = None
    if kind == "subset":
        sel = np.sort(np.random.default_rng(m).permutation(m + n_extra)[:m])
    elif kind == "descending":
        sel = np.arange(m)[::-1].copy()
    D = distances(x, sel, min_sep)
    msd, scale = msd_cross(D, D)
    for a in (x, D, msd, scale):
        a.setflags(write=False)
    return dict(x=x, sel=sel, m=m, N=N, min_sep=min_sep, P=n_pairs(m, min_sep), D=D, msd=msd, scale=scale)


BITMAP_CASES = ((130, 87, 1), (65, 33, 2), (64, 17, 1))


def cutoff_of(c):
    """A cut-off (dRMSD) the bound decides for every pair: the root of the midpoint of the widest gap of the sorted msd
    values in the middle tenth of them.  The decision is taken at cutoff * cutoff, as the Python layer forms it."""
    iu = np.triu_indices(c["N"], 1)
    v = np.sort(c["msd"][iu].astype(np.float64))
    lo, hi = int(0.45 * v.size), int(0.55 * v.size) + 1
    k = lo + int(np.argmax(np.diff(v[lo:hi + 1])))
    return float(np.sqrt(0.5 * (v[k] + v[k + 1])))


def undecided(c, cut2):
    """The pairs whose decision msd <= cut2 the matrix bound does not settle."""
    lim = LD(matrix_bound(c["P"])) * c["scale"]
    return np.abs(c["msd"] - LD(cut2)) <= lim
