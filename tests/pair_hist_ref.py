"""References of the pair-histogram tests (tests/test_pair_hist.py, tests/test_pair_hist_host.py): the float32 restatement
of the bin decision include/codlad_hip.h states for codlad_pair_hist, the same histogram in float64, numpy restatements of
codlad_pair_hist_profile in its one stated order of additions, the derived bounds, and the seeded cases.  Every array a
case hands out is read-only."""
import functools

import numpy as np

from tests import saxs_ref as sr

F = np.float32
SINC_SLOPE = 0.43618          # max |d sinc(x) / dx|, attained at x ~ 2.0816
MAX_BINS, MAX_ATOMS, MAX_TYPES = 4096, 65535, sr.MAX_TYPES


def class_index(a, b, T):
    return a * T - a * (a - 1) // 2 + (b - a)


def classes(T):
    return [(a, b) for a in range(T) for b in range(a, T)]


def pair_classes(types, T):
    """(i, j, c): every pair i < j in the caller's atom order and its class."""
    types = np.asarray(types, dtype=np.int64)
    i, j = np.triu_indices(types.shape[0], 1)
    lo, hi = np.minimum(types[i], types[j]), np.maximum(types[i], types[j])
    return i, j, class_index(lo, hi, T)


# ------------------------------------------------------------------------------------------------ the restatement --
def t32(x, i, j, inv_dr):
    """The header's sequence for the pairs (i, j) of one structure x float32 [n, 3]: float32, one rounding per operation."""
    x = np.asarray(x, dtype=F)
    with np.errstate(over="ignore", invalid="ignore"):
        d = x[j] - x[i]
        dx, dy, dz = d[:, 0], d[:, 1], d[:, 2]
        r = np.sqrt((dx * dx + dy * dy) + dz * dz)
        t = r * F(inv_dr)
    assert t.dtype == F
    return t


def t64(x, i, j, dr):
    """The same quantity in float64 from the float32 coordinates the kernel reads: r / dr."""
    x = np.asarray(x, dtype=F).astype(np.float64)
    d = x[j] - x[i]
    return np.sqrt((d * d).sum(1)) / float(dr)


def _count(t, c, T, B):
    C = T * (T + 1) // 2
    inside = t < B
    bins = t[inside].astype(np.int64)
    H = np.zeros((C, B), dtype=np.int64)
    np.add.at(H, (c[inside], bins), 1)
    over = np.bincount(c[~inside], minlength=C).astype(np.int64)
    occupied = np.nonzero(H.sum(0))[0]
    return H, over, int(occupied[-1]) if occupied.size else -1


def hist32(x, types, T, dr, B):
    """x float32 [S, n, 3] -> (H int64 [S, C, B], over [S, C], d_bin [S]) by the float32 decision: t < (float)B ? (int)t :
    over, with inv_dr = float32(1 / dr).  Counts the pairs i < j in the caller's order."""
    i, j, c = pair_classes(types, T)
    out = [_count(t32(xs, i, j, F(1.0 / dr)), c, T, B) for xs in x]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out]), np.array([o[2] for o in out], dtype=np.int64)


def hist64(x, types, T, dr, B):
    """The same in float64 throughout."""
    i, j, c = pair_classes(types, T)
    out = [_count(t64(xs, i, j, dr), c, T, B) for xs in x]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out]), np.array([o[2] for o in out], dtype=np.int64)


def sinc_table(q, B, dr):
    x = ((np.arange(B, dtype=np.float64) + 0.5) * dr)[:, None] * np.asarray(q, dtype=np.float64)[None, :]
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(x == 0.0, 1.0, np.sin(x) / x)


def complete_of(over, finite):
    return np.array([bool(f) and not (o != 0).any() for o, f in zip(over, finite)])


def _mean(rows, keep):
    total, count = np.zeros(rows.shape[1]), 0
    for s in range(rows.shape[0]):                                   # index order
        if keep[s]:
            total, count = total + rows[s], count + 1
    return total / float(count) if count else np.full(rows.shape[1], np.nan)


def profile_ref(H, over, d_bin, finite, count, ff, sinc):
    """codlad_pair_hist_profile's I and mean_I in the header's order: per class the bins ascending up to d_bin, then the
    classes ascending; + and * in float64, one at a time (vectors over k only) -> (I [S, Q], mean [Q], complete [S])."""
    ff, sinc = np.asarray(ff, dtype=np.float64), np.asarray(sinc, dtype=np.float64)
    T, Q = ff.shape
    S = H.shape[0]
    complete = complete_of(over, finite)
    I = np.full((S, Q), np.nan)
    for s in range(S):
        if not complete[s]:
            continue
        partial = np.zeros((H.shape[1], Q))
        for b in range(int(d_bin[s]) + 1):                            # every class walks its bins in this order
            partial = partial + H[s, :, b].astype(np.float64)[:, None] * sinc[b][None, :]
        self_term, cross = np.zeros(Q), np.zeros(Q)
        for a in range(T):
            self_term = self_term + float(count[a]) * (ff[a] * ff[a])
        for c, (a, b) in enumerate(classes(T)):
            cross = cross + (ff[a] * ff[b]) * partial[c]
        I[s] = self_term + 2.0 * cross
    return I, _mean(I, complete), complete


def pr_ref(H, over, d_bin, finite, count, w, r2):
    """codlad_pair_hist_profile's P, I0, m2 and mean_P in the header's order -> (P [S, B], I0 [S], m2 [S], mean [B])."""
    w, r2 = np.asarray(w, dtype=np.float64), np.asarray(r2, dtype=np.float64)
    T = w.shape[0]
    S, _C, B = H.shape
    P, I0, m2 = np.full((S, B), np.nan), np.full(S, np.nan), np.full(S, np.nan)
    for s in range(S):
        if not finite[s]:
            continue
        last = int(d_bin[s])
        row = np.zeros(B)
        for c, (a, b) in enumerate(classes(T)):                       # the classes ascending, every bin on its own
            row[:last + 1] = row[:last + 1] + (w[a] * w[b]) * H[s, c, :last + 1].astype(np.float64)
        self_term, total, mom = 0.0, 0.0, 0.0
        for a in range(T):
            self_term = self_term + float(count[a]) * (w[a] * w[a])
        for b in range(last + 1):
            total = total + row[b]
            mom = mom + r2[b] * row[b]
        P[s], I0[s], m2[s] = row, self_term + 2.0 * total, mom
    return P, I0, m2, _mean(P, complete_of(over, finite))


# ---------------------------------------------------------------------------------------------- the derived bounds --
def profile_bound(types, ff, q, dr, delta):
    """|I_hist[k] - I_debye[k]| <= SINC_SLOPE q_k (dr / 2 + delta dr) 2 sum_{i<j} |f_i f_j|: a distance is read at the
    centre of its bin, at most dr / 2 away (delta bins more where the fp32 decision differs), and sinc(q r) changes by at
    most SINC_SLOPE q per unit of r."""
    f = np.abs(np.asarray(ff, dtype=np.float64)[np.asarray(types)])            # [n, Q]
    total = f.sum(0)
    pairs = (total * total - (f * f).sum(0)) / 2.0                             # sum_{i<j} |f_i f_j|
    return SINC_SLOPE * np.asarray(q, dtype=np.float64) * (dr / 2.0 + delta * dr) * 2.0 * pairs


def moment_ref(x, types, w):
    """Float64 pairwise: (m2 = sum_{i<j} w_i w_j r_ij^2, sum_{i<j} |w_i w_j| r_ij, sum_{i<j} |w_i w_j|) per structure."""
    x = np.asarray(x, dtype=F).astype(np.float64)
    wi = np.asarray(w, dtype=np.float64)[np.asarray(types)]
    i, j = np.triu_indices(x.shape[1], 1)
    ww = wi[i] * wi[j]
    out = []
    for xs in x:
        r = np.sqrt(((xs[j] - xs[i]) ** 2).sum(1))
        out.append(((ww * r * r).sum(), (np.abs(ww) * r).sum(), np.abs(ww).sum()))
    return np.array(out).reshape(-1, 3)


def moment_bound(sum_wr, sum_w, dr, delta):
    """|sum w_i w_j (r_c^2 - r^2)| with |r_c - r| <= e = dr / 2 + delta dr: |r_c^2 - r^2| <= e (2 r + e) per pair, which
    is r dr + dr^2 / 4 at delta = 0."""
    e = dr / 2.0 + delta * dr
    return e * (2.0 * sum_wr + e * sum_w)


# ------------------------------------------------------------------------------------------------------ the cases --
SIZES = sr.SIZES                               # (1, 2, 63, 64, 65, 129, 300): the edges of the 64-row tile, several tiles
T_SIZES = sr.T_SIZES                           # (1, 5, 32)
B_SIZES = (1, 64, 65, 400)
DRS = (0.5, 0.1)
SHIFTS = sr.SHIFTS
N_STRUCT = sr.N_STRUCT
Q_GRID = np.linspace(0.01, 0.5, 7).astype(F).astype(np.float64)      # float32 numbers: saxs_ref.debye64 reads the same


def case_keys():
    """(n, T, B, dr, shift): every size at the wide grid (no pair beyond it) and at a short fine one (most pairs beyond it,
    shifted), and every T and B at the tile edges."""
    keys = [(n, 5, 400, 0.5, 0.0) for n in SIZES] + [(n, 5, 65, 0.1, 500.0) for n in SIZES]
    keys += [(65, 1, 64, 0.5, 0.0), (63, MAX_TYPES, 1, 0.5, 500.0), (129, MAX_TYPES, 64, 0.1, 0.0),
             (300, MAX_TYPES, 400, 0.1, 500.0), (300, 1, 65, 0.5, 0.0), (2, 1, 1, 0.1, 500.0), (64, MAX_TYPES, 400, 0.5, 0.0)]
    return keys


def case_id(key):
    return f"n{key[0]}-T{key[1]}-B{key[2]}-dr{key[3]}-{'shifted' if key[4] else 'origin'}"


@functools.lru_cache(maxsize=None)
def case(key):
    """x float32 [3, n, 3], types int32 [n], count [T], ff float64 [T, 7] on Q_GRID and positive weights w [T]; H32, over32,
    d32 (the restatement), H64, over64, d64, the pairs' class and t64 per structure, delta = 4 max |t32 - t64| and near =
    the share of pairs whose float64 t lies within delta of a bin edge."""
    n, T, B, dr, shift = key
    rng = np.random.default_rng(7000003 * n + 1009 * T + 13 * B + int(1000 * dr) + int(shift))
    extent = 4.0 * max(n, 2) ** (1.0 / 3.0)                                            # a protein's density, roughly
    x = (rng.uniform(-0.5, 0.5, (N_STRUCT, n, 3)) * extent + shift).astype(F)
    if T >= 3:                        # the last type has no atom, the one before it exactly one
        types = rng.integers(0, T - 2, n).astype(np.int32)
        types[n // 2] = T - 2
    else:
        types = rng.integers(0, T, n).astype(np.int32)
    f0 = rng.uniform(-2.0, 9.0, T)
    width = rng.uniform(5.0, 40.0, T)
    ff = (f0[:, None] * np.exp(-width[:, None] * (Q_GRID[None, :] / (4 * np.pi)) ** 2)).astype(F).astype(np.float64)
    w = (np.abs(f0) + 0.5).astype(F).astype(np.float64)                                # positive: Rg is defined
    i, j, c = pair_classes(types, T)
    ts64 = np.stack([t64(xs, i, j, dr) for xs in x])
    ts32 = np.stack([t32(xs, i, j, F(1.0 / dr)) for xs in x]).astype(np.float64)
    delta = 4.0 * float(np.abs(ts32 - ts64).max()) if i.size else 0.0
    near = float((np.abs(ts64 - np.rint(ts64)) <= delta).mean()) if i.size else 0.0
    H32, over32, d32 = hist32(x, types, T, dr, B)
    H64, over64, d64 = hist64(x, types, T, dr, B)
    return sr._freeze(dict(x=x, types=types, count=np.bincount(types, minlength=T).astype(np.int64), ff=ff, w=w, cls=c, t64=ts64,
                           delta=delta, near=near, n_pairs=int(i.size), H32=H32, over32=over32, d32=d32, H64=H64, over64=over64,
                           d64=d64))


def lattice(n):
    """n atoms of one type at (i, 0, 0), float32 [1, n, 3]."""
    x = np.zeros((1, n, 3), dtype=F)
    x[0, :, 0] = np.arange(n, dtype=F)
    return x


def lattice_hist(n, dr, B):
    """The histogram of lattice(n) at an integer bin width dr in closed form -> (H int64 [B], over int, d_bin): there are
    n - d pairs at distance d = 1 .. n - 1 and bin b holds the distances dr b .. dr b + dr - 1.  For n <= 65535 and dr a
    power of two the header's fp32 sequence gives exactly d / dr: dx = d is a float32 number, dx * dx is d^2 (1 + e) with
    |e| < 2^-24, its correctly rounded root lies within d 2^-25 of d, less than half a unit in the last place of d, so it
    IS d; and d * (1 / dr) is exact (tests/test_size_limits_host.py runs this sequence in numpy for every d)."""
    d = np.arange(1, n, dtype=np.int64)
    count = n - d
    inside = d // dr < B
    H = np.bincount(d[inside] // dr, weights=count[inside], minlength=B).astype(np.int64)
    occupied = np.nonzero(H)[0]
    return H, int(count[~inside].sum()), int(occupied[-1]) if occupied.size else -1


def sandwich(H, c_of_pair, ts64, delta, B):
    """For every class and every bin edge b = 0 .. B: #64{t < b - delta} <= sum_{bin < b} H[c] <= #64{t < b + delta}.
    H [C, B] of one structure -> the number of (class, edge) pairs that break it."""
    edges = np.arange(B + 1, dtype=np.float64)
    bad = 0
    for c in range(H.shape[0]):
        t = np.sort(ts64[c_of_pair == c])
        cum = np.concatenate([[0], np.cumsum(H[c])])
        lo = np.searchsorted(t, edges - delta, side="left")
        hi = np.searchsorted(t, edges + delta, side="left")
        bad += int(((cum < lo) | (cum > hi)).sum())
    return bad
