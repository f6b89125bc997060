"""Clustering of an ensemble (csrc/cluster_kernels.hip): the superposed RMSD of every pair of a pool of up to 65 536
structures as one float64 matrix product on the MFMA units (rmsd_matrix), the neighbour bitmap at a cut-off without the
N x N table (rmsd_neighbours), Daura's (GROMOS) clustering of such a bitmap on the device (cluster_neighbours), and the
three together (cluster).  The host enqueues the rounds of the clustering in batches and reads one integer per batch."""
import math
import numbers

import torch

from .. import _lib
from . import _inputs
from .ensemble import _moments, _pair_msd

CLUSTER_MAX_N = _lib.CLUSTER_MAX_N
CLUSTER_BATCH = 64            # rounds enqueued between two looks at the number of structures still active


def _matrix(x, sel, n_sel, cut2, squared, want_matrix, want_bits):
    N, n = x.shape[:2]
    dev = x.device
    lib = _lib.lib()
    mom = _moments(x, N, n, sel, n_sel)
    scratch = _inputs.scratch("codlad_rmsd_matrix_scratch_bytes", N, n_sel or n, dev=dev)
    out = torch.empty(N, N, dtype=torch.float64, device=dev) if want_matrix else None
    # the bitmap and the finite bytes share one allocation of two words or more (tests/memcheck.py cannot tell a
    # one-element integer buffer from its poison)
    n_bits = N * ((N + 63) // 64) if want_bits else 0
    ints = torch.empty(max(2, n_bits + (N + 7) // 8), dtype=torch.int64, device=dev)
    bits = ints[:n_bits].view(N, (N + 63) // 64) if want_bits else None
    finite = ints[n_bits:].view(torch.uint8)[:N]
    p = _lib.ptr
    rc = lib.codlad_rmsd_matrix(p(x), p(mom), N, n, p(sel), n_sel, float(cut2), int(bool(squared)), p(out), p(bits), p(finite),
                                p(scratch), _lib.stream_ptr(dev))
    _lib.check(rc, "codlad_rmsd_matrix")
    return out, bits, finite


def rmsd_matrix(x, sel=None, squared=False):
    """x [N, n, 3] (one pool, N <= 65 536) -> float64 [N, N] on the device: the RMSD of every pair after the optimal proper
    rotation plus translation over the atoms sel (default: all); the msd with squared=True.  Symmetric to the bit, the
    diagonal exactly 0; the row and the column of a structure with a NaN or an infinity among its selected atoms are NaN.
    An element depends on its two structures alone, and a repeat gives the same bits - not those of superposed_rmsd_batch,
    whose sums have another order."""
    x, sel, n_sel = _inputs.pool(x, sel, "rmsd_matrix", CLUSTER_MAX_N)
    return _matrix(x, sel, n_sel, 0.0, squared, True, False)[0]


def rmsd_neighbours(x, cutoff, sel=None, return_matrix=False):
    """Who is within `cutoff` (RMSD, a positive finite number) of whom -> dict: bits int64 [N, ceil(N / 64)] (uint64 patterns:
    bit j & 63 of word j >> 6 of row i is set iff both structures are finite and msd_ij <= cutoff^2, the diagonal bit of a
    finite structure included, bits at j >= N zero), finite bool [N], n = N, and with return_matrix rmsd float64 [N, N].
    Without return_matrix no N x N table is made: 512 MB of bits for 65 536 structures."""
    c = _inputs.positive(cutoff, "cutoff", "rmsd_neighbours")
    x, sel, n_sel = _inputs.pool(x, sel, "rmsd_neighbours", CLUSTER_MAX_N)
    out, bits, finite = _matrix(x, sel, n_sel, c * c, False, return_matrix, True)
    res = dict(bits=bits, finite=finite.to(torch.bool), n=x.shape[0])
    if return_matrix:
        res["rmsd"] = out
    return res


def cluster_neighbours(bits, n, finite=None, weights=None):
    """Daura's (GROMOS) clustering of a neighbour bitmap (rmsd_neighbours' layout; any bitmap may be given - the diagonal
    bit is taken as set, bits at j >= n are ignored): among the structures still in the pool the one with the most
    neighbours in the pool, itself included and the lowest index among equals, is the centre of the next cluster; it and
    those neighbours leave the pool; until the pool is empty.  finite bool [n]: a False structure is never in the pool.
    -> dict: labels int32 [n] (the clusters are numbered in the order they were picked; -1 for a non-finite structure),
    centres, sizes int32 [K], n_clusters, rounds (the picks it took), populations float64 [K]: the weights' sums per cluster
    over the sum of all labelled structures' weights (both added in ascending index), sizes / sum(sizes) without weights."""
    _inputs.need_cuda(bits, "cluster_neighbours: bits")
    if not (isinstance(n, numbers.Integral) and 1 <= n <= CLUSTER_MAX_N):
        raise ValueError(f"cluster_neighbours: n must be an integer in 1 .. {CLUSTER_MAX_N}, got {n!r}")
    n = int(n)
    W = (n + 63) // 64
    if bits.dtype != torch.int64 or tuple(bits.shape) != (n, W):
        raise ValueError(f"cluster_neighbours: bits must be int64 [{n}, {W}], got {bits.dtype} {tuple(bits.shape)}")
    dev = bits.device
    fin = None
    if finite is not None:
        fin = torch.as_tensor(finite).reshape(-1)
        if fin.shape[0] != n:
            raise ValueError(f"cluster_neighbours: finite must have one entry per structure ({n}), got {fin.shape[0]}")
        fin = fin.to(device=dev).to(torch.uint8).contiguous()
    w = None if weights is None else _inputs.weights(weights, n, dev, "cluster", False)
    bits = bits.contiguous()
    lib = _lib.lib()
    scratch = _inputs.scratch("codlad_cluster_scratch_bytes", n, dev=dev, dtype=torch.int64)
    state = torch.zeros(_lib.CLUSTER_STATE_WORDS, dtype=torch.int32, device=dev)          # phase 0: new
    labels, centres, sizes = torch.empty(3, n, dtype=torch.int32, device=dev).unbind(0)
    p = _lib.ptr
    for _batch in range(n // CLUSTER_BATCH + 2):              # a round removes one structure or more
        rc = lib.codlad_cluster_daura(p(bits), p(fin), n, CLUSTER_BATCH, p(state), p(labels), p(centres), p(sizes), p(scratch),
                                      _lib.stream_ptr(dev))
        _lib.check(rc, "codlad_cluster_daura")
        if int(state[_lib.CLUSTER_ST_ACTIVE]) == 0:           # the one transfer of the batch
            break
    else:
        raise RuntimeError("cluster_neighbours: the pool did not empty")
    st = state.tolist()
    K = st[_lib.CLUSTER_ST_CLUSTERS]
    centres, sizes = centres[:K].clone(), sizes[:K].clone()
    if w is None or K == 0:
        pop = sizes.to(torch.float64) / sizes.sum().to(torch.float64)
    else:
        # the clusters' sums, and the total as the one cluster of everything that has a label: both in ascending index
        sums = torch.empty(K + 1, dtype=torch.float64, device=dev)
        everything = torch.where(labels >= 0, 0, -1).to(torch.int32).contiguous()
        for lab, k, at in ((labels, K, sums[:K]), (everything, 1, sums[K:])):
            _lib.check(lib.codlad_cluster_populations(p(lab), p(w), n, k, p(at), _lib.stream_ptr(dev)), "codlad_cluster_populations")
        pop = sums[:K] / sums[K]
    return dict(labels=labels, centres=centres, sizes=sizes, n_clusters=K, populations=pop, rounds=st[_lib.CLUSTER_ST_ROUNDS])


def cluster(x, cutoff, sel=None, weights=None, return_matrix=False):
    """Daura's clustering of the pool x [N, n, 3] at the RMSD cut-off `cutoff` over the atoms sel: rmsd_neighbours, then
    cluster_neighbours of its bitmap -> cluster_neighbours' dict plus finite bool [N], centre_rmsd float64 [N] (the RMSD of
    every structure to the centre of its cluster, NaN for a non-finite structure) and, with return_matrix,
    rmsd [N, N].  centre_rmsd is read from the matrix when it was asked for; otherwise it is N pairs through
    superposed_rmsd_batch's kernel, to the bit what that gives for (structure, its centre).  weights [N] (>= 0, finite;
    for instance reweight's w) turn the populations into the weighted ones."""
    c = _inputs.positive(cutoff, "cutoff", "cluster")
    x, sel, n_sel = _inputs.pool(x, sel, "cluster", CLUSTER_MAX_N)
    N = x.shape[0]
    if weights is not None:
        _inputs.weights(weights, N, x.device, "cluster", False)                      # refused before any launch
    rmsd, bits, finite = _matrix(x, sel, n_sel, c * c, False, return_matrix, True)
    out = cluster_neighbours(bits, N, finite=finite, weights=weights)
    lab = out["labels"].to(torch.int64)
    ok = lab >= 0
    idx = torch.arange(N, device=x.device)
    if out["n_clusters"]:
        centre_of = torch.where(ok, out["centres"].to(torch.int64)[lab.clamp(min=0)], idx)
    else:
        centre_of = idx
    if return_matrix:
        cr = rmsd[idx, centre_of]
    else:
        pairs = torch.stack((idx, centre_of), 1).to(torch.int32).contiguous()
        cr, _ = _pair_msd(x, x, pairs, sel, n_sel, False, False)
    out["centre_rmsd"] = torch.where(ok, cr, torch.full_like(cr, math.nan))
    out["finite"] = finite.to(torch.bool)
    out["bits"] = bits
    if return_matrix:
        out["rmsd"] = rmsd
    return out


__all__ = ["CLUSTER_MAX_N", "CLUSTER_BATCH", "rmsd_matrix", "rmsd_neighbours", "cluster_neighbours", "cluster"]
