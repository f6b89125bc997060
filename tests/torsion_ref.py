"""References for the torsion kernels (codlad_torsion_*, codlad_feature_covariance), numpy only: the float64 restatement of
the feature sequence of include/codlad_hip.h (the device returns its bits), the same formulas in np.longdouble on the same
fp32 inputs with the quantities the feature bound multiplies, longdouble DIRECT sums for the matrix (never the Gram form),
the pairs, the resultants and the covariance, the pools the tests run on, and the error bounds, which are read from the
macros of the header and restated from their parts (none is fitted)."""
import functools
import os
import re

import numpy as np

from tests import stereo_ref as sr
from tests.drmsd_ref import rotations
from tests.polymer_ref import walk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "codlad_hip.h")).read()
LD = np.longdouble
EPS = 2.220446049250313e-16                            # 2^-52, the factor of every bound macro


def macro(name):
    """The value of the plain integer macro CODLAD_TORSION_<name>."""
    m = re.search(r"^#define CODLAD_TORSION_" + name + r" ([0-9]+)$", HEADER, re.M)
    assert m, name
    return int(m.group(1))


def macro_text(name):
    """The text of the macro CODLAD_TORSION_<name> (with its argument list, if it has one)."""
    m = re.search(r"^#define CODLAD_TORSION_" + re.escape(name) + r" (.+)$", HEADER, re.M)
    assert m, name
    return m.group(1)


MAX_T, X_OPS, Y_OPS = macro("MAX_T"), macro("X_OPS"), macro("Y_OPS")


def _c_value(text, **names):
    """A bound macro's C expression: `/` between integers is C's integer division, ?: becomes if / else."""
    expr = text.replace("((T) + 63) / 64", "((T) + 63) // 64")
    assert re.fullmatch(r"[0-9A-Za-z_()+\-*/. <?:]+", expr), text
    return float(eval(expr, {"__builtins__": {}}, names))


def chunk_max(N):
    """The structures of a chunk at most, CODLAD_TORSION_CHUNK_MAX(N)."""
    assert macro_text("CHUNK_MAX(N)") == "((N) < 16384 ? ((N) < 528 ? (N) : 528) : (N) / 32 + 16)"
    return (N if N < 528 else 528) if N < 16384 else N // 32 + 16


def chunks_of(N):
    """reduce_math.h's chunks_of, restated: (number of chunks, structures of a chunk)."""
    nch = min(32, (N + 511) // 512)
    chunk = (((N + nch - 1) // nch) + 15) // 16 * 16
    return (N + chunk - 1) // chunk, chunk


def feature_bound(r):
    """|cos - exact|, |sin - exact| for r = (X_OPS X + Y_OPS Y) / h (array)."""
    assert macro_text("FEATURE_BOUND(r)") == "(((r) + 2.0) * 2.220446049250313e-16)"
    return (r + LD(2)) * LD(EPS)


def mean_bound(N):
    """|mean - exact| / (sum w |F| / W): the chunk, the chunks, the division; for W the lane, the butterfly, the chunks."""
    assert macro_text("MEAN_BOUND(N)") == ("((CODLAD_TORSION_CHUNK_MAX(N) + CODLAD_TORSION_CHUNK_MAX(N) / 64 + 72.0) * "
                                           "2.220446049250313e-16)")
    c = chunk_max(N)
    assert chunks_of(N)[1] <= c + 15 and min(N, chunks_of(N)[1]) <= c
    return (c + 32 + 1 + (c // 64 + 1) + 6 + 32) * EPS


def matrix_bound(T):
    """|tmsd - exact| / ((G_i + G_j + 2 |C_ij|) / T): 2 T + 1 roundings per accumulated product, two additions, the division."""
    v = _c_value(macro_text("MATRIX_BOUND(T)"), T=int(T))
    assert v == (2 * T + 1 + 2) * EPS
    return v


def pairs_bound(T):
    """|tmsd - exact| / exact of the pair route: term 4, lane ceil(T / 64), butterfly 6, division 1."""
    v = _c_value(macro_text("PAIRS_BOUND(T)"), T=int(T))
    assert v == (4 + (T + 63) // 64 + 6 + 1) * EPS
    return v


def term_bound():
    assert macro_text("TERM_BOUND") == "(4.0 * 2.220446049250313e-16)"
    return 4 * EPS


COV_BOUND_EXTRA = 34                                   # the existing (N + 34) 2^-52 T_ij of codlad_pca_covariance


# -------------------------------------------------------------------------------------------------------- features --
def _cross(a, b, minus=True):
    s = -1 if minus else 1
    return np.stack([a[..., 1] * b[..., 2] + s * (a[..., 2] * b[..., 1]), a[..., 2] * b[..., 0] + s * (a[..., 0] * b[..., 2]),
                     a[..., 0] * b[..., 1] + s * (a[..., 1] * b[..., 0])], -1)


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _xyh(x, quads, dtype):
    """The header's sequence in `dtype` from the fp32 coordinates -> (x, y, h, b1, b2, b3), each [N, T(, 3)]."""
    assert x.dtype == np.float32
    q = np.asarray(quads, dtype=np.int64)
    p = x.astype(dtype)[:, q]                                                   # [N, T, 4, 3]
    b1, b2, b3 = p[:, :, 1] - p[:, :, 0], p[:, :, 2] - p[:, :, 1], p[:, :, 3] - p[:, :, 2]
    n1, n2 = _cross(b1, b2), _cross(b2, b3)
    xx = _dot(n1, n2)
    yy = np.sqrt(_dot(b2, b2)) * _dot(b1, n2)
    h = np.sqrt(xx * xx + yy * yy)
    return xx, yy, h, b1, b2, b3


def finite_of(x, quads):
    """A structure is finite when no atom a quad names has a NaN or an infinity (collinear quads are found by h == 0)."""
    named = np.unique(np.asarray(quads, dtype=np.int64))
    return np.isfinite(x[:, named]).all(axis=(1, 2))


def features64(x, quads):
    """The float64 restatement -> (F float64 [N, 2 T] laid out (cos_0, sin_0, ..), finite bool [N]): NaN rows where an atom
    of a quad is not finite or a torsion has h == 0."""
    with np.errstate(all="ignore"):
        xx, yy, h, *_ = _xyh(x, quads, np.float64)
        ok = finite_of(x, quads) & (h > 0).all(1)
        F = np.stack([xx / h, yy / h], -1).reshape(x.shape[0], -1)
    assert F.dtype == np.float64
    F[~ok] = np.nan
    return F, ok


def features_ld(x, quads):
    """The same formulas in longdouble -> (F longdouble [N, 2 T], bound [N, 2 T]): the bound of the header, with X and Y the
    values of x and y when every product is taken by its absolute value."""
    with np.errstate(all="ignore"):
        xx, yy, h, b1, b2, b3 = _xyh(x, quads, LD)
        a1, a2, a3 = np.abs(b1), np.abs(b2), np.abs(b3)
        X = _dot(_cross(a1, a2, False), _cross(a2, a3, False))
        Y = np.sqrt(_dot(b2, b2)) * _dot(a1, _cross(a2, a3, False))
        r = (LD(X_OPS) * X + LD(Y_OPS) * Y) / h
        F = np.stack([xx / h, yy / h], -1).reshape(x.shape[0], -1)
        bound = np.repeat(feature_bound(r), 2, axis=1)
    return F, bound


def angles_to_features(deg):
    """(cos, sin) of angles in degrees, longdouble [..., 2]."""
    rad = np.deg2rad(np.asarray(deg, dtype=np.float64)).astype(LD)
    return np.stack([np.cos(rad), np.sin(rad)], -1)


# ------------------------------------------------------------------------------------------------------ direct sums --
def tmsd_cross(Fa, Fb):
    """Fa [Na, 2 T], Fb [Nb, 2 T] float64 -> (tmsd, scale) longdouble [Na, Nb]: the direct sum of (f_a - f_b)^2 / T, and
    scale_exact, what the matrix bound multiplies.  NaN rows stay NaN."""
    T = LD(Fa.shape[1] // 2)
    A, B = Fa.astype(LD), Fb.astype(LD)
    out = np.zeros((A.shape[0], B.shape[0]), dtype=LD)
    with np.errstate(invalid="ignore"):
        for i in range(A.shape[0]):
            out[i] = ((B - A[i]) ** 2).sum(1)
    return out / T, scale_exact(Fa, Fb)


def scale_exact(Fa, Fb):
    """(G_a + G_b + 2 |C_ab|) / T in longdouble: what CODLAD_TORSION_MATRIX_BOUND multiplies."""
    T = LD(Fa.shape[1] // 2)
    A, B = Fa.astype(LD), Fb.astype(LD)
    with np.errstate(invalid="ignore"):
        ga, gb = (A * A).sum(1), (B * B).sum(1)
        C = np.zeros((A.shape[0], B.shape[0]), dtype=LD)
        for i in range(A.shape[0]):
            C[i] = (B * A[i]).sum(1)
        return (ga[:, None] + gb[None, :] + 2 * np.abs(C)) / T


def worst(got, want, scale, bound):
    """The largest |got - want| / (bound * scale) over the elements with a finite reference (0 / 0 counts as 0)."""
    got = np.asarray(got).astype(LD)
    ok = np.isfinite(want)
    err, lim = np.abs(got - want)[ok], (LD(bound) * scale)[ok]
    with np.errstate(invalid="ignore", divide="ignore"):
        f = np.where(err == 0, LD(0), err / lim)
    return float(f.max()) if f.size else 0.0


def mean_ld(F, finite, w=None):
    """-> (mean longdouble [2 T], scale [2 T] = sum w |F| / W, W): over the finite structures of positive weight."""
    w = np.ones(F.shape[0]) if w is None else np.asarray(w, dtype=np.float64)
    use = finite & (w > 0)
    wl, Fl = w[use].astype(LD), F[use].astype(LD)
    W = wl.sum()
    return (wl[:, None] * Fl).sum(0) / W, (wl[:, None] * np.abs(Fl)).sum(0) / W, W


def cov_ld(D, finite, w=None):
    """D float64 [N, d] (the device's deviations) -> (C, Tij) longdouble [d, d]: sum w D D^T / W and sum w |D| |D|^T / W."""
    w = np.ones(D.shape[0]) if w is None else np.asarray(w, dtype=np.float64)
    use = finite & (w > 0)
    wl, Dl = w[use].astype(LD), D[use].astype(LD)
    W = wl.sum()
    return (Dl * wl[:, None]).T @ Dl / W, (np.abs(Dl) * wl[:, None]).T @ np.abs(Dl) / W


# ----------------------------------------------------------------------------------------------------------- pools --
def chain_quads(T):
    """The quads (k, k + 1, k + 2, k + 3) of a chain of T + 3 beads."""
    k = np.arange(T, dtype=np.int32)
    return np.stack([k, k + 1, k + 2, k + 3], 1)


POOL_SIZES = (1, 2, 63, 64, 65, 130)
TORSION_COUNTS = (1, 2, 7, 8, 9, 33, 129)
CASES = tuple(dict.fromkeys([(N, 33) for N in POOL_SIZES] + [(65, T) for T in TORSION_COUNTS] + [(1473, 9), (2, 2048)]))
BITMAP_CASES = ((130, 33), (65, 9), (64, 7))


@functools.lru_cache(maxsize=None)
def case(N, T):
    """A pool of random-walk chains and its references, computed once and frozen."""
    x = walk(N, T + 3, seed=3)
    quads = chain_quads(T)
    F, finite = features64(x, quads)
    assert finite.all()
    tmsd, scale = tmsd_cross(F, F)
    for a in (x, quads, F, tmsd, scale):
        a.setflags(write=False)
    return dict(x=x, quads=quads, N=N, T=T, F=F, tmsd=tmsd, scale=scale)


def translated(x):
    """-> (the pool on a grid of 2^-10, the same moved by a vector of that grid): the translation is exact in fp32 and every
    coordinate difference keeps its bits (drmsd_ref.translated)."""
    assert np.abs(x).max() < 512.0
    q = np.round(x * 1024.0) / 1024.0
    return q.astype(np.float32), (q + np.array([64.0, -128.0, 32.0])).astype(np.float32)


def cutoff_of(c):
    """A cut-off (torsion distance) the bound decides for every pair: the root of the midpoint of the widest gap of the
    sorted tmsd values in the middle tenth of them.  The decision is taken at cutoff * cutoff, as the Python layer forms it."""
    iu = np.triu_indices(c["N"], 1)
    v = np.sort(c["tmsd"][iu].astype(np.float64))
    lo, hi = int(0.45 * v.size), int(0.55 * v.size) + 1
    k = lo + int(np.argmax(np.diff(v[lo:hi + 1])))
    return float(np.sqrt(0.5 * (v[k] + v[k + 1])))


def undecided(c, cut2):
    """The pairs whose decision tmsd <= cut2 the matrix bound does not settle."""
    return np.abs(c["tmsd"] - LD(cut2)) <= LD(matrix_bound(c["T"])) * c["scale"]


HELIX, EXTENDED, LEFT = (-60.0, -45.0), (-120.0, 130.0), (60.0, 45.0)


@functools.lru_cache(maxsize=None)
def planted(n_states=2, n_res=12, copies=40, seed=0, noise=4.0):
    """A chain of n_res ALA by stereo_ref.build_chain: the first half of the residues helical in every structure, the second
    half in one of n_states states (helical, extended, left-handed) per structure, Gaussian noise of `noise` degrees on
    every phi and psi, and a random rigid motion applied to each copy -> dict: top, x float32 [copies, n_atoms, 3], state
    int [copies], phi, psi float64 [copies, n_res] (what was planted)."""
    rng = np.random.default_rng(seed)
    states = (HELIX, EXTENDED, LEFT)[:n_states]
    state = np.arange(copies) % n_states
    rng.shuffle(state)
    rots = rotations(copies, seed + 1)
    xs, phis, psis = [], [], []
    top = None
    for s in range(copies):
        phi = np.full(n_res, HELIX[0]) + rng.normal(0.0, noise, n_res)
        psi = np.full(n_res, HELIX[1]) + rng.normal(0.0, noise, n_res)
        phi[n_res // 2:] += states[state[s]][0] - HELIX[0]
        psi[n_res // 2:] += states[state[s]][1] - HELIX[1]
        top, xyz = sr.build_chain(["ALA"] * n_res, phi, psi, np.full(n_res, 180.0), np.zeros((n_res, 4)))
        xs.append(xyz @ rots[s].T + rng.uniform(-20.0, 20.0, 3))
        phis.append(phi)
        psis.append(psi)
    return dict(top=top, x=np.ascontiguousarray(np.array(xs).astype(np.float32)), state=state, phi=np.array(phis), psi=np.array(psis))
