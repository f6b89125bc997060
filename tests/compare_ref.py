"""References of the ensemble-comparison tests (tests/test_compare.py, tests/test_compare_host.py): numpy restatements of
what include/codlad_hip.h states for codlad_dist_hist (the float32 bin decision of codlad_pair_hist, over the structures of
a pool), codlad_column_hist (the float64 decision) and codlad_hist_divergence (float64 in the stated order), the same
histogram and the same divergences in wider arithmetic, the derived bounds, and the seeded pools.  Every array a case hands
out is read-only."""
import functools

import numpy as np

from tests import pair_hist_ref as ph

F = np.float32
EPS = 2.0 ** -52
MAX_BINS, MAX_SEL, MAX_COLS, MAX_ROWS = 256, 2048, 4098, 1048576


def pair_index(i, j, m):
    return i * m - i * (i + 1) // 2 + (j - i - 1)


def pairs(m):
    """(i, j): the selection positions of every row, i ascending and j ascending within i."""
    return np.triu_indices(m, 1)


def _sel(x, sel):
    return np.asarray(x, dtype=F) if sel is None else np.asarray(x, dtype=F)[:, np.asarray(sel, dtype=np.int64)]


def finite_of(x, sel=None):
    return np.isfinite(_sel(x, sel)).all(axis=(1, 2))


def _count(ts, n_bins):
    """ts [S, P] -> int64 [P, n_bins + 2]: column 1 + (int)t where t < n_bins, the last column otherwise, column 0 empty."""
    S, P = ts.shape
    H = np.zeros((P, n_bins + 2), dtype=np.int64)
    for t in ts:
        inside = t < n_bins
        col = np.where(inside, 1 + np.where(inside, t, 0).astype(np.int64), n_bins + 1)
        np.add.at(H, (np.arange(P), col), 1)
    return H


def hist32(x, sel, inv_dr, n_bins):
    """x float32 [N, n, 3] -> (H int64 [P, n_bins + 2], finite bool [N], n_counted) by the header's float32 sequence
    (pair_hist_ref.t32, operation by operation) over the finite structures; inv_dr the float32 number the kernel is given."""
    xs = _sel(x, sel)
    fin = finite_of(x, sel)
    i, j = pairs(xs.shape[1])
    ts = np.stack([ph.t32(s, i, j, F(inv_dr)) for s in xs[fin]]) if fin.any() else np.zeros((0, i.size), dtype=F)
    assert ts.dtype == F
    return _count(ts, n_bins), fin, int(fin.sum())


def t64(x, sel, inv_dr):
    """float64 r * inv_dr of the finite structures from the float32 coordinates the kernel reads, [S, P]."""
    xs = _sel(x, sel)[finite_of(x, sel)].astype(np.float64)
    i, j = pairs(xs.shape[1])
    d = xs[:, j] - xs[:, i]
    return np.sqrt((d * d).sum(2)) * float(F(inv_dr))


def hist64(x, sel, inv_dr, n_bins):
    return _count(t64(x, sel, inv_dr), n_bins)


def delta_of(x, sel, inv_dr):
    """4 max |t32 - t64| over the pool (pair_hist_ref.case's margin): how far the fp32 decision may sit from the float64 one,
    in bins."""
    xs = _sel(x, sel)[finite_of(x, sel)]
    i, j = pairs(xs.shape[1])
    if not xs.shape[0]:
        return 0.0
    t32 = np.stack([ph.t32(s, i, j, F(inv_dr)) for s in xs]).astype(np.float64)
    return 4.0 * float(np.abs(t32 - t64(x, sel, inv_dr)).max())


def sandwich(H, ts64, delta, n_bins):
    """For every pair and every bin edge b = 0 .. n_bins: #64{t < b - delta} <= sum_{column <= b} H[p] <= #64{t < b + delta}
    (pair_hist_ref.sandwich over the structures of one pair).  H [P, n_bins + 2] -> the number of (pair, edge) that break it."""
    edges = np.arange(n_bins + 1, dtype=np.float64)
    bad = 0
    for p in range(H.shape[0]):
        t = np.sort(ts64[:, p])
        cum = np.cumsum(H[p])[:n_bins + 1]                       # columns 0 .. b: everything below edge b
        lo = np.searchsorted(t, edges - delta, side="left")
        hi = np.searchsorted(t, edges + delta, side="left")
        bad += int(((cum < lo) | (cum > hi)).sum())
    return bad


def column_hist_ref(values, lo, inv_width, n_bins, periodic):
    """codlad_column_hist in float64, one rounding per operation: values [N, C] -> (H int64 [C, n_bins + 2], n_valid [C])."""
    v = np.asarray(values, dtype=np.float64)
    N, C = v.shape
    H, n_valid = np.zeros((C, n_bins + 2), dtype=np.int64), np.zeros(C, dtype=np.int64)
    with np.errstate(over="ignore", invalid="ignore"):
        t = (v - np.float64(lo)) * np.float64(inv_width)
    ok = np.isfinite(v)
    if periodic:
        ok &= np.abs(t) < 2147483648.0
        k = np.floor(np.where(ok, t, 0.0)).astype(np.int64) % n_bins          # numpy's % on integers is non-negative here
        col = 1 + k
    else:
        f = np.floor(np.where(ok, t, 0.0))
        col = np.where(t < 0, 0, np.where(f >= n_bins, n_bins + 1, 1 + np.clip(f, 0, n_bins - 1).astype(np.int64)))
    for s in range(N):
        c = np.nonzero(ok[s])[0]
        np.add.at(H, (c, col[s, c]), 1)
        n_valid[c] += 1
    return H, n_valid


def divergence_ref(HA, HB):
    """codlad_hist_divergence in float64 in the header's order: k ascending, every sum added to 0 -> (js, tv, w1) [rows]."""
    HA, HB = np.asarray(HA, dtype=np.int64), np.asarray(HB, dtype=np.int64)
    rows, cols = HA.shape
    js, tv, w1 = (np.full(rows, np.nan) for _ in range(3))
    for r in range(rows):
        a, b = HA[r], HB[r]
        nA, nB = int(a.sum()), int(b.sum())
        if nA == 0 or nB == 0 or (a < 0).any() or (b < 0).any():
            continue
        p, q = a.astype(np.float64) / np.float64(nA), b.astype(np.float64) / np.float64(nB)
        mid = 0.5 * (p + q)
        with np.errstate(divide="ignore", invalid="ignore"):
            tp = np.where(a > 0, p * np.log2(p / mid), 0.0)
            tq = np.where(b > 0, q * np.log2(q / mid), 0.0)
        term, gap = tp + tq, np.abs(p - q)
        sj = sv = sw = cA = cB = np.float64(0.0)
        for k in range(cols):
            sj, sv = sj + term[k], sv + gap[k]
            cA, cB = cA + p[k], cB + q[k]
            if k < cols - 1:
                sw = sw + abs(cA - cB)
        js[r], tv[r], w1[r] = 0.5 * sj, 0.5 * sv, sw
    return js, tv, w1


def divergence_ld(HA, HB):
    """The same quantities in np.longdouble (sums by numpy, any order) -> (js, tv, w1) [rows] as longdouble."""
    L = np.longdouble
    HA, HB = np.asarray(HA, dtype=np.int64), np.asarray(HB, dtype=np.int64)
    rows = HA.shape[0]
    js, tv, w1 = (np.full(rows, np.nan, dtype=L) for _ in range(3))
    for r in range(rows):
        a, b = HA[r], HB[r]
        if a.sum() == 0 or b.sum() == 0 or (a < 0).any() or (b < 0).any():
            continue
        p, q = a.astype(L) / L(a.sum()), b.astype(L) / L(b.sum())
        mid = (p + q) / L(2)
        with np.errstate(divide="ignore", invalid="ignore"):
            tp = np.where(a > 0, p * np.log2(np.where(a > 0, p / np.where(mid > 0, mid, 1), 1)), L(0))
            tq = np.where(b > 0, q * np.log2(np.where(b > 0, q / np.where(mid > 0, mid, 1), 1)), L(0))
        js[r] = (tp.sum() + tq.sum()) / L(2)
        tv[r] = np.abs(p - q).sum() / L(2)
        w1[r] = np.abs(np.cumsum(p) - np.cumsum(q))[:-1].sum()
    return js, tv, w1


def bounds(cols):
    """(js, tv, w1): the header's bounds CODLAD_DIVERGENCE_*_BOUND against the exact value, from cols, 2^-52 and a log2
    within one unit in the last place."""
    return (4.0 * cols + 8.0) * EPS, (cols + 2.0) * EPS, (2.0 * cols * cols + 2.0 * cols) * EPS


HAND_JS = 0.5 * (0.5 + 0.5 * np.log2(2.0 / 3.0) + np.log2(4.0 / 3.0))      # p = (1/2, 1/2) against q = (0, 1): 0.311278...


# ------------------------------------------------------------------------------------------------------ the cases --
# (N, m, n_bins, dr, kind): a spread of N in {1, 2, 63, 64, 65, 300} x m in {2, 3, 15, 16, 17, 33, 129} - the edges of the
# batch of 16 structures and of the 16 x 16, 8 x 16, 8 x 8 and 4 x 8 tiles (n_bins 50, 100, 200 / 255, 256), several tiles,
# several chunks of structures - and n_bins in {1, 50, 255, 256}.  kind: "all" (no sel), "sel" (ascending), "mixed" (a sel
# that is not ascending), "far" (a short grid: most pairs in the overflow column)
SHAPES = ((1, 2, 50, 0.5, "all"), (2, 3, 1, 40.0, "all"), (63, 15, 50, 0.5, "sel"), (64, 16, 255, 0.125, "all"),
          (65, 17, 256, 0.125, "mixed"), (300, 33, 50, 0.5, "sel"), (65, 129, 50, 1.0, "all"), (300, 16, 100, 0.25, "mixed"),
          (2, 129, 200, 0.25, "sel"), (63, 33, 50, 0.1, "far"), (300, 2, 256, 0.0625, "all"), (64, 17, 1, 3.0, "far"))
LIMITS = ((2, 2048, 1, 64.0), (65, 3, 256, 0.125))               # (N, m, n_bins, dr): m and n_bins at their caps


def shape_id(key):
    return f"N{key[0]}-m{key[1]}-B{key[2]}-dr{key[3]}-{key[4]}"


def _freeze(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.flags.writeable = False
    return d


@functools.lru_cache(maxsize=None)
def pool(N, m, kind="all", seed=0):
    """x float32 [N, n, 3] and sel (None or int64 [m]): a random coil at a protein's density."""
    rng = np.random.default_rng(9000011 * N + 1013 * m + seed + sum(map(ord, kind)))
    n = m if kind in ("all", "far") else m + 7
    extent = 4.0 * max(m, 2) ** (1.0 / 3.0)
    x = (rng.uniform(-0.5, 0.5, (N, n, 3)) * extent).astype(F)
    sel = None
    if kind == "sel":
        sel = np.sort(rng.choice(n, m, replace=False)).astype(np.int64)
    elif kind == "mixed":
        sel = rng.permutation(n)[:m].astype(np.int64)
        if m > 1 and (np.diff(sel) > 0).all():
            sel = sel[::-1].copy()
    return _freeze(dict(x=x, sel=sel))


@functools.lru_cache(maxsize=None)
def case(key):
    N, m, n_bins, dr, kind = key
    c = pool(N, m, kind)
    inv_dr = F(1.0 / dr)
    H32, fin, n_counted = hist32(c["x"], c["sel"], inv_dr, n_bins)
    return _freeze(dict(x=c["x"], sel=c["sel"], inv_dr=inv_dr, H32=H32, finite=fin, n_counted=n_counted,
                        H64=hist64(c["x"], c["sel"], inv_dr, n_bins), t64=t64(c["x"], c["sel"], inv_dr),
                        delta=delta_of(c["x"], c["sel"], inv_dr)))


def lattice_pool(N, m):
    """N copies of m atoms at (i, 0, 0), the s-th stretched by the power of two 2^(s mod 3): every distance sits on a bin
    edge at dr = 1 / 2, 1, 2 (pair_hist_ref.lattice)."""
    x = np.repeat(ph.lattice(m), N, axis=0)
    return x * (2.0 ** (np.arange(N) % 3)).astype(F)[:, None, None]


def lattice_hist(N, m, dr, n_bins):
    """The closed form of lattice_pool(N, m) at a power-of-two dr: pair (i, j) of structure s is at exactly (j - i) 2^(s mod
    3), an exact float32 quotient -> int64 [P, n_bins + 2]."""
    i, j = pairs(m)
    H = np.zeros((i.size, n_bins + 2), dtype=np.int64)
    for s in range(N):
        k = ((j - i) * 2 ** (s % 3) / dr).astype(np.int64)       # exact: integers over a power of two
        np.add.at(H, (np.arange(i.size), np.where(k < n_bins, 1 + k, n_bins + 1)), 1)
    return H


def count_tables(rows, cols, seed, sparse=False):
    """Two seeded count tables int32 [rows, cols]; sparse: most columns empty, in one table or the other or both."""
    rng = np.random.default_rng(seed)
    A = rng.integers(0, 2000, (rows, cols))
    B = rng.integers(0, 50, (rows, cols)) + (A // 3)
    if sparse:
        A = np.where(rng.random((rows, cols)) < 0.8, 0, A)
        B = np.where(rng.random((rows, cols)) < 0.8, 0, B)
        A[:, 0] += 1                                                # no empty row: those are a case of their own
        B[:, -1] += 1
    return A.astype(np.int32), B.astype(np.int32)


DIVERGENCE_SHAPES = ((1, 3, False), (7, 52, False), (8256, 38, True), (64, 258, False), (65, 258, True), (300, 4, True))


def hinge_pools(n_a=64, n_b=48, m=6):
    """Two planted two-state pools of m atoms on a line 3.8 A apart, the last atom swung out so that its distance to atom 0
    is 5 A ("closed") or 9 A ("open") while every other pair stays where it is: pool a is half closed and half open, pool b
    all open -> (a, b) float32.  The pair (0, m - 1) has the proportions (1/2, 1/2) against (0, 1) at any grid that
    separates 5 from 9 A; pairs without the last atom have equal proportions."""
    base = np.zeros((m, 3), dtype=np.float64)
    base[:, 0] = 3.8 * np.arange(m)

    def state(d):
        s = base.copy()
        s[m - 1] = (0.0, d, 0.0)
        return s
    closed, opened = state(5.0), state(9.0)
    a = np.stack([closed if s % 2 == 0 else opened for s in range(n_a)]).astype(F)
    b = np.stack([opened] * n_b).astype(F)
    return a, b
