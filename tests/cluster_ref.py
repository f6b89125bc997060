"""Host reference and inputs of the clustering tests (tests/test_cluster.py, tests/test_cluster_host.py).

The matrix reference is tests/ensemble_ref.kabsch - centre, 3x3 covariance, singular values, sign(det), in float64 - for
every pair of a pool; `all_pairs` is that arithmetic on stacked arrays (numpy's svd of a stack is the same LAPACK call per
matrix), held to kabsch itself in test_cluster_host.py, because 525 000 separate calls take half a minute.  The tolerance
is ensemble_ref.msd_bound.  The Daura reference is a plain loop over a boolean matrix.  Inputs are fp32, built on the CPU
from fixed seeds; every cached array is read-only."""
import functools

import numpy as np

from tests import ensemble_ref as er

PLANTED_CUTOFF, CONTINUUM_CUTOFF = 1.0, 2.0
MAX_N = 65536                                             # CODLAD_CLUSTER_MAX_N
POOL_SIZES = (1, 2, 15, 16, 17, 63, 64, 65, 130)          # at n = 65
ATOM_COUNTS = (1, 2, 3, 4, 5, 63, 64, 65, 257, 1000)      # at N = 17
LARGE = (1025, 5)
SHAPES = tuple((N, 65) for N in POOL_SIZES) + tuple((17, n) for n in ATOM_COUNTS if n != 65) + (LARGE,)
PLANTED_CASES = ((130, 65, 5), (65, 4, 3), (17, 257, 2))  # (N, n, K): the separated ones, no pair near the cut-off
SUB_POOL = (0, 15, 16, 17, 31, 47, 48, 63, 64, 65, 79, 80, 100, 111, 127, 128, 129)   # 17 of 130 across tile and block borders


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


@functools.lru_cache(maxsize=None)
def planted(N, n, K):
    """-> (x fp32 [N, n, 3], blob int [N]): K blobs of spread 5 A; a member is its blob plus 0.2 A noise, moved by a random
    rotation and a ~10 A translation; every odd member a further 1000 A away."""
    rng = np.random.default_rng(7919 * N + 31 * n + K)
    blobs = rng.standard_normal((K, n, 3)) * 5.0
    blob = rng.integers(0, K, N)
    x = np.empty((N, n, 3))
    for i in range(N):
        y = blobs[blob[i]] + 0.2 * rng.standard_normal((n, 3))
        y = y @ er._rotation(rng).T + 10.0 * rng.standard_normal(3)
        if i % 2:
            y = y + np.array([1000.0, -500.0, 250.0])
        x[i] = y
    return _frozen(x.astype(np.float32), blob)


@functools.lru_cache(maxsize=None)
def continuum(N=130, n=65):
    """One blob with noise growing from 0.05 to 3.0 A along the pool, every member rotated, every odd one 1000 A away: the
    neighbour relation at 2.0 A is not transitive."""
    rng = np.random.default_rng(1)
    base = rng.standard_normal((n, 3)) * 5.0
    x = np.empty((N, n, 3))
    for i, s in enumerate(np.linspace(0.05, 3.0, N)):
        y = (base + s * rng.standard_normal((n, 3))) @ er._rotation(rng).T
        if i % 2:
            y = y + np.array([1000.0, -500.0, 250.0])
        x[i] = y
    return _frozen(x.astype(np.float32))


@functools.lru_cache(maxsize=None)
def degenerate(n=65):
    """Both conformations of make_pair's planar, collinear, mirror and identical cases, near the origin and 1000 A away."""
    _labels, a, b, _refs = er.cases_of_size(n)
    keep = [k for k, (cat, _off) in enumerate(_labels) if cat in ("planar", "collinear", "mirror", "identical")]
    return _frozen(np.concatenate([np.stack((a[k], b[k])) for k in keep]).astype(np.float32))


def pool(N, n):
    """The pool of a shape of SHAPES: planted with five blobs (as many as there are members below five)."""
    return planted(N, n, min(5, N))[0]


def all_pairs(x):
    """x [N, n, 3] -> (msd [N, N] not clamped, e0n [N, N]) in float64: ensemble_ref.kabsch's arithmetic for every pair."""
    x = np.asarray(x, dtype=np.float64)
    N, n = x.shape[:2]
    xc = x - x.mean(1, keepdims=True)
    G = (xc * xc).sum((1, 2))
    cov = np.einsum("ink,jnl->ijkl", xc, xc)
    u, sv, vt = np.linalg.svd(cov)
    d = np.sign(np.linalg.det(u @ vt))
    e0 = G[:, None] + G[None, :]
    msd = (e0 - 2.0 * (sv[..., 0] + sv[..., 1] + d * sv[..., 2])) / n
    return msd, e0 / n


@functools.lru_cache(maxsize=None)
def reference(kind, *key):
    """(msd clamped at 0 [N, N], bound [N, N]) of planted(*key) / continuum() / degenerate() / pool(*key), once per session."""
    x = {"planted": lambda: planted(*key)[0], "continuum": continuum, "degenerate": degenerate, "pool": lambda: pool(*key)}[kind]()
    msd, e0n = all_pairs(x)
    return _frozen(np.maximum(msd, 0.0), er.msd_bound(x.shape[1], e0n))


def undecided(msd_ref, bound, cut2):
    """The pairs whose decision msd <= cut2 the bound does not settle."""
    return np.abs(msd_ref - cut2) <= bound


# ---------------------------------------------------------------------------------------------------------- bitmaps --
def pack(nb, garbage=False):
    """bool [N, N] -> int64 [N, ceil(N / 64)] of uint64 patterns; garbage: every padding bit set."""
    N = nb.shape[0]
    W = (N + 63) // 64
    full = np.zeros((N, W * 64), dtype=bool)
    full[:, :N] = nb
    if garbage:
        full[:, N:] = True
    words = (full.reshape(N, W, 64).astype(np.uint64) << np.arange(64, dtype=np.uint64)).sum(-1, dtype=np.uint64)
    return words.view(np.int64)


def unpack(bits, N):
    """int64 [N, W] -> bool [N, W * 64] (the padding bits included: the caller looks at [:, N:])."""
    u = np.ascontiguousarray(bits).view(np.uint64)
    return ((u[:, :, None] >> np.arange(64, dtype=np.uint64)) & np.uint64(1)).astype(bool).reshape(u.shape[0], -1)


def daura(nb, finite=None):
    """The rule, one cluster at a time, on a boolean matrix (row i = the neighbours of i; the diagonal is taken as set)."""
    nb = np.array(nb, dtype=bool)
    N = nb.shape[0]
    nb[np.arange(N), np.arange(N)] = True
    active = np.ones(N, dtype=bool) if finite is None else np.array(finite, dtype=bool)
    labels, centres, sizes = np.full(N, -1, dtype=np.int32), [], []
    while active.any():
        counts = (nb & active[None, :]).sum(1)
        counts[~active] = -1
        c = int(np.argmax(counts))                        # the first of equals: the lowest index
        members = nb[c] & active
        labels[members] = len(centres)
        centres.append(c)
        sizes.append(int(members.sum()))
        active &= ~members
    return dict(labels=labels, centres=np.array(centres, dtype=np.int32), sizes=np.array(sizes, dtype=np.int32), n_clusters=len(centres))


# ------------------------------------------------------------------------------------------ block-structured bitmaps --
def clique_members(cliques):
    """A clique is (first index, size) - consecutive structures - or an explicit list of indices -> a list of sorted lists."""
    out = [list(range(c[0], c[0] + c[1])) if isinstance(c, tuple) else sorted(int(i) for i in c) for c in cliques]
    flat = [i for m in out for i in m]
    assert len(flat) == len(set(flat)), "the cliques overlap"
    return out


def clique_matrix(N, cliques):
    """bool [N, N]: every member of a clique is the neighbour of every other; nothing else is set (no diagonal either)."""
    nb = np.zeros((N, N), dtype=bool)
    for m in clique_members(cliques):
        nb[np.ix_(m, m)] = True
    nb[np.arange(N), np.arange(N)] = False
    return nb


def clique_answer(N, cliques, finite=None):
    """Daura's rule on clique_matrix in closed form: among disjoint cliques a structure counts the members of its own
    clique that are still in the pool, so the cliques leave in descending size (of their finite members), the one with the
    lowest first finite member among equals, each centred on that member; when the largest count is 1 the closing launch
    numbers what is left - the structures of no clique and the cliques of one finite member - in ascending order.
    -> daura()'s dict plus rounds, the picks it took."""
    fin = np.ones(N, dtype=bool) if finite is None else np.asarray(finite, dtype=bool)
    groups = [[i for i in m if fin[i]] for m in clique_members(cliques)]
    big = sorted((g for g in groups if len(g) > 1), key=lambda g: (-len(g), g[0]))
    labels = np.full(N, -1, dtype=np.int32)
    for k, g in enumerate(big):
        labels[g] = k
    rest = np.nonzero(fin & (labels < 0))[0]
    labels[rest] = len(big) + np.arange(rest.shape[0])
    centres = np.array([g[0] for g in big] + rest.tolist(), dtype=np.int32)
    sizes = np.array([len(g) for g in big] + [1] * rest.shape[0], dtype=np.int32)
    return dict(labels=labels, centres=centres, sizes=sizes, n_clusters=int(centres.shape[0]),
                rounds=len(big) + (1 if rest.shape[0] else 0))


def limit_cliques(N, fill=False):
    """The cliques of the size-limit cases (tests/test_size_limits.py) for a pool of N structures, W = ceil(N / 64) words:
    cliques across the borders of the words 0, 63, 64, W / 2 - 1 and W - 1 (where N has them), one of the last structure
    with members of word 0, a run of pairs (more non-singleton cliques than one batch of rounds), and equal sizes with
    the lower first index winning.  Everything else is a singleton - or, with fill, all but every 41st of the rest goes
    into cliques of 389 that reach over six or seven words each (the plain loop takes a pass over the matrix per cluster:
    thousands of singletons are for the closed form alone)."""
    W = (N + 63) // 64
    out = [[0, 1, 2, N - 1]]                                        # the last structure with three of word 0
    used = {0, 1, 2, N - 1}

    def add(first, size):
        idx = [i for i in range(first, first + size) if 0 <= i < N and i not in used]
        if len(idx) > 1:
            out.append(idx)
            used.update(idx)

    for w, size in ((1, 9), (63, 7), (64, 11), (65, 5), (W // 2, 13), (W - 1, 6)):      # across the border before word w
        if 1 <= w < W:
            add(64 * w - size // 2, size)
    add(64 * (W - 1) - 40, 5)                                       # inside the word before the last: equal in size to (65, 5)
    add(10, 30)                                                     # the largest, inside word 0
    # four inside word 4: it ties with the first clique, which must win on its lower index - and loses to this one as soon
    # as a count leaves out the last word, where the first clique has its fourth member
    add(300, 4)
    for k in range(80):                                             # pairs: a second batch of rounds
        add(N // 3 + 3 * k if N < 2000 else 1000 + 37 * k, 2)
    if fill:
        free = [i for i in range(N) if i not in used]
        rest = [i for k, i in enumerate(free) if k % 41]            # every 41st of them stays a singleton
        out += [rest[a:a + 389] for a in range(0, len(rest), 389) if len(rest[a:a + 389]) > 1]
    return out


def from_edges(N, edges):
    nb = np.zeros((N, N), dtype=bool)
    for i, j in edges:
        nb[i, j] = nb[j, i] = True
    return nb


def _star(N, hub, leaves):
    """A hub with its leaves, everything else alone: cluster 0 is the star, the rest follow in ascending order."""
    members = sorted([hub] + list(leaves))
    labels = np.zeros(N, dtype=np.int32)
    rest = [i for i in range(N) if i not in members]
    labels[rest] = 1 + np.arange(len(rest))
    return (N, [(hub, leaf) for leaf in leaves], labels.tolist(), [hub] + rest, [len(members)] + [1] * len(rest))


def _pairs_then_singles(n_pairs, n_single):
    N = 2 * n_pairs + n_single
    labels = [k // 2 for k in range(2 * n_pairs)] + [n_pairs + k for k in range(n_single)]
    centres = [2 * k for k in range(n_pairs)] + [2 * n_pairs + k for k in range(n_single)]
    return (N, [(2 * k, 2 * k + 1) for k in range(n_pairs)], labels, centres, [2] * n_pairs + [1] * n_single)


# name -> (N, edges, labels, centres, sizes), the answers derived by hand from the rule
HAND = {
    "chain A~B~C, A and C apart: B has three, one cluster": (3, [(0, 1), (1, 2)], [0, 0, 0], [1], [3]),
    "two pairs with equal counts: the lower index first": (4, [(0, 1), (2, 3)], [0, 0, 1, 1], [0, 2], [2, 2]),
    # counts 4 2 2 3 3 2: 0 takes 1 2 3; then 4 and 5 both count 2 (4 had 3, 5 had 2 before) and 4 wins
    "a tie that appears after the first removal": (6, [(0, 1), (0, 2), (0, 3), (3, 4), (4, 5)], [0, 0, 0, 0, 1, 1], [0, 4], [4, 2]),
    "all singletons": (5, [], [0, 1, 2, 3, 4], [0, 1, 2, 3, 4], [1] * 5),
    "one cluster of everything": (70, [(i, j) for i in range(70) for j in range(i)], [0] * 70, [0], [70]),
    "N = 64, the hub at 63": _star(64, 63, (0, 1, 2)),
    "N = 65, the hub at 64": _star(65, 64, (0, 62, 63)),
    "N = 129, the hub at 128": _star(129, 128, (0, 64, 127)),
    "70 pairs and 60 singletons: a second batch of rounds": _pairs_then_singles(70, 60),
}
