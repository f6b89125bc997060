"""Cases and rules for non-finite input (tests/test_nonfinite_inputs.py, GPU) and the CPU test that holds them to what
they claim (tests/test_nonfinite_cases_host.py).  Nothing here touches a GPU.

The rule every entry point is held to: a NaN or +-inf coordinate or latent gives a DEFINED result - never an index out of
range, never "valid", never a changed bit in what did not read it.  The restatements are plain numpy, so a comparison
with a NaN is false and arithmetic with one is NaN, as IEEE 754 has it; none of them cleans a value up.

1. The k-NN rule of features_kernel (csrc/features_kernels.hip, stage B) in its own float32 arithmetic.  `parent_ranks` is
   the rule before the total order (rank = #{q: d_q < d_j or (d_q == d_j and q < j)}): a NaN distance gets rank 0 and is
   counted by no other rank, so ranks collide and slots of the neighbour row are never written.  `total_ranks` sorts a NaN
   after every number, ties by index: always a permutation.  `unread_edge` names the edges of a structure whose features
   read no bad residue.
2. The float64 all-pairs reference of tests/test_geometry_check.py under the contract of codlad_geometry_check: a template
   bond is broken when !(d < cut), min_dist is NaN and `valid` False when any coordinate is not finite.
3. Where the bad value goes: PLANTS = bad value x {one component, all three} x {first, middle, last element}.
"""
import functools

import numpy as np

from codlad_amd import synth
from tests import test_geometry_check as tg

NAN, INF = float("nan"), float("inf")
BAD_VALUES = {"nan": NAN, "+inf": INF, "-inf": -INF}
COMPONENTS = {"y": (1,), "xyz": (0, 1, 2)}
POSITIONS = ("first", "middle", "last")
PLANTS = [(b, c, p) for b in BAD_VALUES for c in COMPONENTS for p in POSITIONS]

KNN = 64
KNN_LENGTHS = (5, 46, 64, 65, 200)            # K < 32; K = L <= 64 (partial and full second half); K saturated
GEOMETRY_SIZES = (4, 255, 256, 257, 1025)     # of test_geometry_check.SIZES: the row block (256) and the column tile (1024)
assert set(GEOMETRY_SIZES) <= set(tg.SIZES)


def position(n, where):
    return {"first": 0, "middle": n // 2, "last": n - 1}[where]


def plant(x, row, bad, comps):
    """A copy of x [n, 3] with the components `comps` of row `row` set to the value named `bad`."""
    out = np.array(x, dtype=np.float32, copy=True)
    out[row, list(COMPONENTS[comps])] = BAD_VALUES[bad]
    return out


def bad_rows(x):
    """Rows of x [n, 3] with a component that is NaN or +-inf."""
    return np.flatnonzero(~np.isfinite(np.asarray(x)).all(-1))


# =====================================================================================================================
# 1. the k-NN rule
# =====================================================================================================================
@functools.lru_cache(maxsize=None)
def ca_trace(L, seed=None):
    """The interior CA trace [L, 3] (float32) of synth.make_protein(L, 70 + L), read-only."""
    x = synth.make_protein(L, (70 + L) if seed is None else seed, n_frames=1)["xyz_full"][0, 1:-1]
    x = np.ascontiguousarray(x, dtype=np.float32)
    x.setflags(write=False)
    return x


def distance_row(x, i):
    """features_kernel's dist_eps of node i to every node: sqrt((dx dx + dy dy) + dz dz + 1e-6), every operation rounded
    to float32 by itself.  (numpy's root is the correctly rounded one; the device's may differ from it in the last place,
    so device rows are held to the RULE through their own clean rows - test_nonfinite_inputs.rule_holds - and never to
    these distances.)"""
    x = np.asarray(x, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        d = x - x[i]
        s = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        return np.sqrt(s + np.float32(1e-6))


def parent_ranks(d):
    """rank[j] = #{q: d_q < d_j or (d_q == d_j and q < j)} - every comparison with a NaN is false."""
    q = np.arange(len(d))
    with np.errstate(invalid="ignore"):
        before = (d[:, None] < d[None, :]) | ((d[:, None] == d[None, :]) & (q[:, None] < q[None, :]))       # [q, j]
    return before.sum(0)


def total_ranks(d):
    """The same with a NaN after every number and two NaNs by index: q goes before j when the parent rule says so, or when
    d_j is NaN and (d_q is a number or q < j)."""
    q = np.arange(len(d))
    nan = np.isnan(d)
    with np.errstate(invalid="ignore"):
        before = (d[:, None] < d[None, :]) | ((d[:, None] == d[None, :]) & (q[:, None] < q[None, :]))
    before |= nan[None, :] & (~nan[:, None] | (q[:, None] < q[None, :]))
    return before.sum(0)


def neighbour_row(ranks, K):
    """What `if (rank < K) nb[rank] = j` leaves in a row of K slots: j, or -1 where no j wrote (with colliding ranks the
    slot's writer is the last in index order here; on the device it is whichever thread writes last)."""
    row = np.full(K, -1, dtype=np.int64)
    for j, r in enumerate(ranks):
        if r < K:
            row[r] = j
    return row


def knn_rows(x, ranks=total_ranks):
    """[L, K] neighbour rows of a structure under the rank rule `ranks`, -1 in slots never written."""
    L = len(x)
    K = min(KNN, L)
    return np.stack([neighbour_row(ranks(distance_row(x, i)), K) for i in range(L)])


def unwritten(rows):
    """Slots never written, per node."""
    return (rows < 0).sum(1)


def readers(i, j, L):
    """The residues the features of edge (i, j) read: the triplets of i and of j (positions, frames, the distance)."""
    return {p for p in (i - 1, i, i + 1, j - 1, j, j + 1) if 0 <= p < L}


def unread_edge(i, j, L, bad):
    """True when no reader of edge (i, j) is in `bad`."""
    return not (readers(i, j, L) & set(int(b) for b in bad))


def knn_cases(L):
    """(label, bad row, planted trace) for every plant on the trace of length L."""
    x = ca_trace(L)
    return [(f"{b}/{c}/{p}", position(L, p), plant(x, position(L, p), b, c)) for b, c, p in PLANTS]


# =====================================================================================================================
# 2. geometry_check
# =====================================================================================================================
def geometry_reference(x, radius, bonds, order=tg.ORDER, scale=tg.SCALE, clash=tg.CLASH, near=tg.NEAR):
    """test_geometry_check.reference under the contract for any bits -> (counts [5], min_dist, valid).  Differences: a
    template bond is broken when not d < cut, and min_dist is NaN when a coordinate is not finite."""
    with np.errstate(invalid="ignore", over="ignore"):
        _i, _j, d, cut, bond, excl = tg.pair_table(x, radius, bonds, order, scale)
        free = ~excl
        counts = [int((bond & ~(d < cut)).sum()), int((~bond & (d < cut)).sum()), int((d < cut).sum()),
                  int((free & (d <= near)).sum()), int((free & (np.sqrt(d * d + 1e-7) < clash)).sum())]
    if len(bad_rows(x)):
        dmin = NAN
    else:
        dmin = float(d[free].min()) if free.any() else INF
    return counts, dmin, counts[0] == 0 and counts[1] == 0 and not np.isnan(dmin)


def geometry_rows(n):
    """Where the bad atom goes: row 0, the last row, and column 1024 (the first of the second column tile)."""
    return sorted({0, n - 1} | ({1024} if n > 1024 else set()))


def geometry_cases(n):
    """(label, bad row, batch [3, n, 3] with structure 1 planted) over test_geometry_check.case(n)."""
    _radius, _bonds, xyz, _refs = tg.case(n)
    out = []
    for b in BAD_VALUES:
        for c in COMPONENTS:
            for row in geometry_rows(n):
                batch = xyz.copy()
                batch[1] = plant(xyz[1], row, b, c)
                out.append((f"{b}/{c}/row{row}", row, batch))
    return out


# =====================================================================================================================
# 3. small restatements of the decoder tail's decisions
# =====================================================================================================================
def first_index_argmin(d):
    """The index the scan `if (d_c < best) best = d_c, bi = c` from best = +inf, bi = 0 ends at, per row of d [n, C]: the
    first minimum of the numbers below +inf; 0 when nothing is (a NaN is never below)."""
    d = np.asarray(d)
    out = np.zeros(d.shape[0], dtype=np.int64)
    for r in range(d.shape[0]):
        best, bi = INF, 0
        for c in range(d.shape[1]):
            if d[r, c] < best:
                best, bi = d[r, c], c
        out[r] = bi
    return out


def vq_distances(z, codebook):
    """(|z|^2 + |e|^2) - 2 z.e per latent and code, float32 [n, C].  Rounded here as numpy rounds, not as vq_kernel's
    fused dot product does: for rows with a NaN or an inf, the only rows this is used on, every entry is NaN or +inf
    either way."""
    z, e = np.asarray(z, dtype=np.float32), np.asarray(codebook, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        sz, se = (z * z).sum(-1), (e * e).sum(-1)
        return (sz[:, None] + se[None, :]) - np.float32(2.0) * (z @ e.T)


def bond_graph_reference(xyz, recon, radius, heavy, scale=1.3):
    """bond_graph_kernel for one structure in its own float32 arithmetic -> the six counts.  A pair is bonded when
    d < (r_i + r_j) * scale, which is false for a d that is not a number: the reference's behaviour (its graphs are
    comparisons of a distance matrix), kept as it is."""
    n = len(radius)
    i, j = np.triu_indices(n, 1)
    radius = np.asarray(radius, dtype=np.float32)
    cut = (radius[i] + radius[j]) * np.float32(scale)

    def bonded(x):
        x = np.asarray(x, dtype=np.float32)
        with np.errstate(invalid="ignore", over="ignore"):
            d = x[i] - x[j]
            return np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]) < cut
    ref, gen = bonded(xyz), bonded(recon)
    hv = (np.asarray(heavy)[i] != 0) & (np.asarray(heavy)[j] != 0)
    return [int(ref.sum()), int(gen.sum()), int((ref != gen).sum()),
            int((ref & hv).sum()), int((gen & hv).sum()), int(((ref != gen) & hv).sum())]


def clash_share(xyz, pairs, clash=1.2):
    """The share of `pairs` at sqrt(d^2 + 1e-7) < clash in float32, as float32 (one term of loss_nbr); 0 for no pairs.
    False for a distance that is not a number, as in the reference."""
    pairs = np.asarray(pairs).reshape(-1, 2)
    if not len(pairs):
        return np.float32(0.0)
    x = np.asarray(xyz, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        d = x[pairs[:, 0]] - x[pairs[:, 1]]
        r = np.sqrt(((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]) + np.float32(1e-7))
        return np.float32(float((r < np.float32(clash)).sum()) / float(len(pairs)))


def ic_nan_pattern(quads, atom):
    """bool [Q, 3]: which of (distance, angle, dihedral) of each quad (A1, A2, A3, A4) read `atom`: the distance A1 and A2,
    the angle A1, A2 and A3, the dihedral all four.  A quad with a negative index reads nothing (zeros are written)."""
    q = np.asarray(quads)
    live = (q >= 0).all(1)
    hit = q == atom
    return np.stack([hit[:, :2].any(1), hit[:, :3].any(1), hit.any(1)], 1) & live[:, None]
