"""Superposition-free distance RMSD (csrc/drmsd_kernels.hip; the arithmetic and its bounds are stated in
include/codlad_hip.h): dRMSD(a, b) = sqrt(sum (d_kl(a) - d_kl(b))^2 / P) over the P pairs k < l, l - k >= min_sep, of an
ORDERED atom selection (position k of `sel` is chain position k), with d the fp32 pair distance.  It needs no frame, so
it is the distance between two conformations of a disordered chain: every pair of a pool or of two pools as one float64
matrix product whose operand is made from the coordinates inside the kernel (drmsd_matrix), the neighbour bitmap at a
cut-off without the N x N table (drmsd_neighbours), a list of pairs by the direct sum (drmsd_pairs), and Daura's
clustering of the bitmap through cluster_neighbours, unchanged (cluster_drmsd)."""
import math

import torch

from .. import _lib
from . import _inputs
from .cluster import CLUSTER_MAX_N, cluster_neighbours

DRMSD_MAX_SEL = _lib.DRMSD_MAX_SEL

__all__ = ["DRMSD_MAX_SEL", "drmsd_matrix", "drmsd_neighbours", "drmsd_pairs", "cluster_drmsd"]


def _chain(x, sel, min_sep, what, max_n=None, name="x"):
    """(the checked structures, sel on the device, n_sel, m, min_sep): a CPU tensor is refused first, then a pool that is
    too large, the selection (a repeated atom among it), its size and min_sep."""
    x = _inputs.structures(x, f"{what}: {name}")
    if max_n is not None and x.shape[0] > max_n:
        raise ValueError(f"{what}: at most {max_n} structures in one pool, got {x.shape[0]}")
    if sel is not None:
        idx = torch.as_tensor(sel).reshape(-1)
        if idx.numel() != torch.unique(idx).numel():
            raise ValueError(f"{what}: sel names an atom twice")
    sel, n_sel = _inputs.selection(sel, x.shape[1], x.device)
    m = n_sel or x.shape[1]
    if not 2 <= m <= DRMSD_MAX_SEL:
        raise ValueError(f"{what}: 2 .. {DRMSD_MAX_SEL} selected atoms, got {m}")
    min_sep = _inputs.count(min_sep, "min_sep", m - 1, what)
    return x, sel, n_sel, m, min_sep


def _same_atoms(x, y, what):
    if y.shape[1] != x.shape[1]:
        raise ValueError(f"{what}: the two pools have {x.shape[1]} and {y.shape[1]} atoms")
    if y.device != x.device:
        raise ValueError(f"{what}: the two pools are on {x.device} and {y.device}")


def _matrix(x, y, sel, n_sel, m, min_sep, cut2, squared, want_matrix, want_bits):
    Na, n = x.shape[:2]
    Nb = 0 if y is None else y.shape[0]
    dev = x.device
    scratch = _inputs.scratch("codlad_drmsd_matrix_scratch_bytes", Na, Nb, m, min_sep, dev=dev)
    out = torch.empty(Na, Nb or Na, dtype=torch.float64, device=dev) if want_matrix else None
    # the bitmap and the finite bytes share one allocation of two words or more, as in cluster._matrix
    n_bits = Na * ((Na + 63) // 64) if want_bits else 0
    ints = torch.empty(max(2, n_bits + (Na + 7) // 8 + (Nb + 7) // 8), dtype=torch.int64, device=dev)
    bits = ints[:n_bits].view(Na, (Na + 63) // 64) if want_bits else None
    fx = ints[n_bits:].view(torch.uint8)[:Na]
    fy = ints[n_bits + (Na + 7) // 8:].view(torch.uint8)[:Nb] if Nb else None
    p = _lib.ptr
    rc = _lib.lib().codlad_drmsd_matrix(p(x), Na, p(y), Nb, n, p(sel), n_sel, min_sep, float(cut2), int(bool(squared)), p(out),
                                        p(bits), p(fx), p(fy), p(scratch), _lib.stream_ptr(dev))
    _lib.check(rc, "codlad_drmsd_matrix")
    return out, bits, fx, fy


def drmsd_matrix(x, y=None, sel=None, min_sep=1, squared=False):
    """x [N, n, 3] (one pool, N <= 65 536) -> float64 [N, N] on the device: the dRMSD of every pair over the pairs of the
    ordered selection sel (default: all atoms) that are min_sep or more chain positions apart; the msd with squared=True.
    Symmetric to the bit, the diagonal exactly 0, and exactly 0 between two structures with the same distances (a
    duplicate, a mirror image, an fp32-exact translate); the row and the column of a structure with a NaN or an infinity
    among its selected atoms are NaN.  An element depends on its two structures, sel and min_sep alone, and a repeat gives
    the same bits.  With y [Nb, n, 3]: float64 [N, Nb], every structure of x against every structure of y (generated
    against true frames: the nearest-frame scores are its row and column minima)."""
    x, sel_d, n_sel, m, min_sep = _chain(x, sel, min_sep, "drmsd_matrix", CLUSTER_MAX_N if y is None else None)
    if y is not None:
        y = _inputs.structures(y, "drmsd_matrix: y")
        _same_atoms(x, y, "drmsd_matrix")
    return _matrix(x, y, sel_d, n_sel, m, min_sep, 0.0, squared, True, False)[0]


def drmsd_neighbours(x, cutoff, sel=None, min_sep=1, return_matrix=False):
    """Who is within `cutoff` (dRMSD, a positive finite number) of whom -> rmsd_neighbours' dict: bits int64 [N, ceil(N /
    64)] in its layout (cluster_neighbours takes it unchanged), finite bool [N], n = N, and with return_matrix drmsd
    float64 [N, N].  Without return_matrix no N x N table is made."""
    c = _inputs.positive(cutoff, "cutoff", "drmsd_neighbours")
    x, sel, n_sel, m, min_sep = _chain(x, sel, min_sep, "drmsd_neighbours", CLUSTER_MAX_N)
    out, bits, finite, _ = _matrix(x, None, sel, n_sel, m, min_sep, c * c, False, return_matrix, True)
    res = dict(bits=bits, finite=finite.to(torch.bool), n=x.shape[0])
    if return_matrix:
        res["drmsd"] = out
    return res


def _pairs(a, b, pairs, sel, n_sel, m, min_sep, per_position):
    dev = a.device
    K = pairs.shape[0]
    msd = torch.empty(max(K, 2), dtype=torch.float64, device=dev)[:K]
    pos = torch.empty(K, m, dtype=torch.float64, device=dev) if per_position else None
    p = _lib.ptr
    rc = _lib.lib().codlad_drmsd_pairs(p(a), a.shape[0], p(b), b.shape[0], a.shape[1], p(sel), n_sel, min_sep, p(pairs), K, p(msd),
                                       p(pos), _lib.stream_ptr(dev))
    _lib.check(rc, "codlad_drmsd_pairs")
    return msd, pos


def drmsd_pairs(a, b, pairs, sel=None, min_sep=1, per_position=False, squared=False):
    """The dRMSD (the msd with squared=True) of the pairs [K, 2] (index into a [Na, n, 3], index into b [Nb, n, 3]) by the
    direct sum of (d_kl(a) - d_kl(b))^2 in float64: no cancellation, the route for a structure against its cluster centre
    or a generated member against its true frame -> float64 [K] (NaN where a structure is not finite).  With
    per_position: (that, float64 [K, m]): per chain position k the mean of (d_kl(a) - d_kl(b))^2 over its partners l -
    where the two structures differ (NaN for a position without partners)."""
    a, sel, n_sel, m, min_sep = _chain(a, sel, min_sep, "drmsd_pairs", name="a")
    b = _inputs.structures(b, "drmsd_pairs: b")
    _same_atoms(a, b, "drmsd_pairs")
    pairs = torch.as_tensor(pairs)
    if pairs.dim() != 2 or pairs.shape[1] != 2 or pairs.shape[0] == 0 or pairs.is_floating_point():
        raise ValueError(f"drmsd_pairs: pairs must be a non-empty integer [K, 2] tensor, got {tuple(pairs.shape)}")
    lo, hi = pairs.min(0).values.tolist(), pairs.max(0).values.tolist()
    if min(lo) < 0 or hi[0] >= a.shape[0] or hi[1] >= b.shape[0]:
        raise ValueError(f"drmsd_pairs: pairs has an index outside the pools ({a.shape[0]}, {b.shape[0]})")
    pairs = pairs.to(device=a.device, dtype=torch.int32).contiguous()
    msd, pos = _pairs(a, b, pairs, sel, n_sel, m, min_sep, per_position)
    out = msd if squared else torch.sqrt(msd)
    return (out, pos) if per_position else out


def cluster_drmsd(x, cutoff, sel=None, min_sep=1, weights=None, return_matrix=False):
    """Daura's clustering of the pool x [N, n, 3] at the dRMSD cut-off `cutoff`: drmsd_neighbours, then cluster_neighbours of
    its bitmap -> cluster's dict with centre_drmsd float64 [N] in the place of centre_rmsd (the dRMSD of every structure
    to the centre of its cluster, NaN for a non-finite structure) and, with return_matrix, drmsd [N, N].  centre_drmsd is
    read from the matrix when it was asked for; otherwise it is N pairs through drmsd_pairs' kernel."""
    c = _inputs.positive(cutoff, "cutoff", "cluster_drmsd")
    x, sel, n_sel, m, min_sep = _chain(x, sel, min_sep, "cluster_drmsd", CLUSTER_MAX_N)
    N = x.shape[0]
    if weights is not None:
        _inputs.weights(weights, N, x.device, "cluster_drmsd", False)                # refused before any launch
    table, bits, finite, _ = _matrix(x, None, sel, n_sel, m, min_sep, c * c, False, return_matrix, True)
    out = cluster_neighbours(bits, N, finite=finite, weights=weights)
    lab = out["labels"].to(torch.int64)
    ok = lab >= 0
    idx = torch.arange(N, device=x.device)
    centre_of = torch.where(ok, out["centres"].to(torch.int64)[lab.clamp(min=0)], idx) if out["n_clusters"] else idx
    if return_matrix:
        cd = table[idx, centre_of]
    else:
        pairs = torch.stack((idx, centre_of), 1).to(torch.int32).contiguous()
        cd = torch.sqrt(_pairs(x, x, pairs, sel, n_sel, m, min_sep, False)[0])
    out["centre_drmsd"] = torch.where(ok, cd, torch.full_like(cd, math.nan))
    out["finite"] = finite.to(torch.bool)
    out["bits"] = bits
    if return_matrix:
        out["drmsd"] = table
    return out
