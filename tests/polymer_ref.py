"""References for the chain-statistics kernels (codlad_chain_sums, codlad_gyration), numpy only: every sum in
np.longdouble by plain diagonals - separation s is the s-th diagonal of the distance matrix, x[s:] against x[:m - s] - the
gyration tensor in longdouble with np.linalg.eigvalsh in float64, the chains the tests run on, and the error bounds, which
are read from the macros of include/codlad_hip.h and restated here from their parts (none is fitted)."""
import functools
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "codlad_hip.h")).read()
LD = np.longdouble
EPS = 2.220446049250313e-16                            # 2^-52, the factor of every bound macro


def macro(name):
    """The value of the plain numeric macro CODLAD_POLYMER_<name>."""
    m = re.search(r"^#define CODLAD_POLYMER_" + name + r" ([0-9.e+-]+)$", HEADER, re.M)
    assert m, name
    return float(m.group(1)) if re.search(r"[.e]", m.group(1)) else int(m.group(1))


def bound_macro(name):
    """The text of the function macro CODLAD_POLYMER_<name>(m)."""
    m = re.search(r"^#define CODLAD_POLYMER_" + name + r"\(m\) (.+)$", HEADER, re.M)
    assert m, name
    return m.group(1)


MAX_SEL, SPLIT_MAX_N, SPLIT_MIN_SEL = macro("MAX_SEL"), macro("SPLIT_MAX_N"), macro("SPLIT_MIN_SEL")
LANES, TERM_OPS, TREE_ADDS, JACOBI_STOP = macro("LANES"), macro("TERM_OPS"), macro("TREE_ADDS"), macro("JACOBI_STOP")


def _c_value(text, m):
    """A bound macro's C expression at m: `/` between the integers (m + 63) and 64 is C's integer division."""
    expr = text.replace("((m) + 63) / 64", "((m) + 63) // 64")
    assert expr != text and re.fullmatch(r"[0-9m()+\-*/. e]+", expr), text
    return float(eval(expr, {"__builtins__": {}}, {"m": int(m)}))


def sum_bound(m):
    """|sep_r2 - exact| / exact and |sep_inv - exact| / exact: the header's CODLAD_POLYMER_SUM_BOUND(m)."""
    v = _c_value(bound_macro("SUM_BOUND"), m)
    assert v == (TERM_OPS + (m + LANES - 1) // LANES + TREE_ADDS) * EPS            # the parts the header derives it from
    return v


def inv_sum_bound(m):
    v = _c_value(bound_macro("INV_SUM_BOUND"), m)
    assert v == (TERM_OPS + (m + LANES - 1) // LANES + TREE_ADDS + (m - 2)) * EPS
    return v


def tensor_bound(m):
    """|tensor - exact| / trace, element by element: CODLAD_POLYMER_TENSOR_BOUND(m)."""
    v = _c_value(bound_macro("TENSOR_BOUND"), m)
    assert v == (3 + (m + LANES - 1) // LANES + TREE_ADDS + 1) * EPS
    return v


def eig_bound(m):
    """|eig - eigvalsh(the device's tensor)| / trace: the tensor's bound and what the Jacobi stop rule may leave."""
    return tensor_bound(m) + JACOBI_STOP


def ensemble_bound(m, N):
    """A weighted ensemble value (r_rms^2, 1 / rh_mean) relative to its longdouble value: the per-structure sums carry
    inv_sum_bound(m) at most (sum_bound is smaller); on top, for N structures of positive terms and in any order, one
    product and at most N additions per term of the numerator, N additions in the sum of the weights, the product
    W (m - s), the quotient, and a square root or a reciprocal: 2 N + 4 roundings, each below 2^-52."""
    return inv_sum_bound(m) + (2 * N + 4) * EPS


# ------------------------------------------------------------------------------------------------------- chains --
def walk(N, m, seed=0, n_extra=0):
    """float32 [N, m + n_extra, 3]: random-walk chains with a step of 3.8 A in a seeded random direction, plus seeded
    noise of 0.05 A on every coordinate (so no two steps are alike in the last bits)."""
    rng = np.random.default_rng(1000 * m + 10 * N + seed)
    n = m + n_extra
    step = rng.normal(size=(N, n, 3))
    step *= 3.8 / np.linalg.norm(step, axis=-1, keepdims=True)
    x = np.cumsum(step, axis=1) + rng.normal(0.0, 0.05, (N, n, 3))
    return np.ascontiguousarray(x.astype(np.float32))


def rod(m):
    """float32 [1, m, 3]: m beads at x = 4 k on the x axis: every value below is exact in fp32 and in float64."""
    x = np.zeros((1, m, 3), dtype=np.float32)
    x[0, :, 0] = 4.0 * np.arange(m)
    return x


def rod_sums(m):
    """(sep_r2, sep_inv) of rod(m) by hand: 16 s^2 (m - s) and (m - s) / (4 s)."""
    s = np.arange(1, m, dtype=np.float64)
    return 16.0 * s * s * (m - s), (m - s) / (4.0 * s)


def cube():
    """float32 [1, 8, 3]: the vertices of the unit cube."""
    return np.array([[(i, j, k) for i in (0, 1) for j in (0, 1) for k in (0, 1)]], dtype=np.float32)


def picked(x, sel):
    return x if sel is None else x[:, np.asarray(sel, dtype=np.int64)]


# --------------------------------------------------------------------------------------------------- references --
def chain_sums_ld(x, sel=None):
    """x float32 [N, n, 3] -> (sep_r2, sep_inv [N, m - 1], inv_sum [N]) in longdouble, and finite bool [N].  A structure
    that is not finite among its selected atoms has NaN rows; coincident atoms give +inf."""
    p = picked(x, sel).astype(LD)
    N, m = p.shape[:2]
    r2s, invs = np.empty((N, m - 1), dtype=LD), np.empty((N, m - 1), dtype=LD)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        for s in range(1, m):
            d = p[:, s:] - p[:, :m - s]
            r2 = (d * d).sum(-1)
            r2s[:, s - 1] = r2.sum(1)
            invs[:, s - 1] = (LD(1) / np.sqrt(r2)).sum(1)
        finite = np.isfinite(p).all(axis=(1, 2))
        r2s[~finite], invs[~finite] = np.nan, np.nan
        return r2s, invs, invs.sum(1), finite


def gyration_ld(x, sel=None):
    """-> (tensor longdouble [N, 6] as (xx, yy, zz, xy, xz, yz) about the exact centroid, eig float64 [N, 3] ascending by
    eigvalsh of its rounding, ree longdouble [N])."""
    p = picked(x, sel).astype(LD)
    d = p - p.mean(1, keepdims=True)
    m = p.shape[1]
    T = np.stack([(d[..., a] * d[..., b]).sum(1) / LD(m) for a, b in ((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))], 1)
    e = p[:, -1] - p[:, 0]
    return T, eigvalsh6(T.astype(np.float64)), np.sqrt((e * e).sum(-1))


def eigvalsh6(t):
    """float64 [N, 6] -> eigvalsh of the symmetric matrices, ascending [N, 3]."""
    t = np.asarray(t, dtype=np.float64)
    A = np.stack([t[:, [0, 3, 4]], t[:, [3, 1, 5]], t[:, [4, 5, 2]]], 1)
    return np.linalg.eigvalsh(A)


def shape_numbers(e):
    """eig [.., 3] ascending -> (asphericity, acylindricity, kappa2, prolateness), in the arithmetic of e."""
    l1, l2, l3 = e[..., 0], e[..., 1], e[..., 2]
    T = l1 + l2 + l3
    return (l3 - (l1 + l2) / 2, l2 - l1, 1 - 3 * (l1 * l2 + l2 * l3 + l3 * l1) / (T * T),
            (3 * l1 - T) * (3 * l2 - T) * (3 * l3 - T) / (T * T * T))


def scaling_ld(x, sel=None, w=None):
    """-> (r_rms longdouble [m - 1], 1 / rh_mean longdouble, n_struct) over the finite structures of positive weight."""
    r2s, _invs, inv_sum, finite = chain_sums_ld(x, sel)
    N, m = r2s.shape[0], r2s.shape[1] + 1
    w = np.ones(N, dtype=LD) if w is None else np.asarray(w).astype(LD)
    use = finite & (w > 0)
    W = w[use].sum()
    s = np.arange(1, m).astype(LD)
    r_rms = np.sqrt((w[use, None] * r2s[use]).sum(0) / (W * (LD(m) - s)))
    return r_rms, (w[use] * (2 * inv_sum[use] / LD(m * m))).sum() / W, int(use.sum())


# -------------------------------------------------------------------------------------------------------- cases --
SHAPE_M, SHAPE_N = (2, 3, 63, 64, 65, 129, 257), (1, 3, 70)


@functools.lru_cache(maxsize=None)
def case(N, m, kind="all"):
    """A pool and its references, computed once: kind "all" (every atom), "subset" (an ascending selection of m of
    m + 9 atoms) or "descending" (the same chain, selected from its far end)."""
    n_extra = 9 if kind == "subset" else 0
    x = walk(N, m, n_extra=n_extra)
    sel = None
    if kind == "subset":
        sel = np.sort(np.random.default_rng(m).permutation(m + n_extra)[:m])
    elif kind == "descending":
        sel = np.arange(m)[::-1].copy()
    r2s, invs, inv_sum, finite = chain_sums_ld(x, sel)
    T, e, ree = gyration_ld(x, sel)
    for a in (x, r2s, invs, inv_sum, T, e, ree):
        a.setflags(write=False)
    return dict(x=x, sel=sel, m=m, N=N, sep_r2=r2s, sep_inv=invs, inv_sum=inv_sum, finite=finite, tensor=T, eig=e, ree=ree)


def worst(got, want, rel_bound):
    """max |got - want| / (rel_bound * |want|) over the elements: the largest fraction of the bound that is used."""
    got, want = np.asarray(got).astype(LD), np.asarray(want).astype(LD)
    return float(np.max(np.abs(got - want) / (LD(rel_bound) * np.abs(want))))
