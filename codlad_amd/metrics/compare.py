"""Comparing two ensembles by their distributions (csrc/compare_kernels.hip; the arithmetic is stated in
include/codlad_hip.h): the histogram of every pairwise distance over the structures of a pool (distance_histogram), the
histogram over the structures of any per-structure quantity (column_histogram), the Jensen-Shannon divergence, total
variation and 1-Wasserstein distance of two count tables row by row (histogram_divergence), and the composed scores of a
generated pool against the pool it was asked to reproduce (ensemble_compare): distances, radius of gyration, backbone and
side-chain torsions, cluster populations.  Counts are integers: the bits repeat and do not depend on the order of the
structures.  Unweighted ensembles only."""
import math

import numpy as np
import torch

from .. import _lib
from . import _inputs

COMPARE_MAX_BINS, DIST_HIST_MAX_SEL, DIVERGENCE_MAX_COLS = _lib.COMPARE_MAX_BINS, _lib.DIST_HIST_MAX_SEL, _lib.DIVERGENCE_MAX_COLS
COMPARE_MAX_ROWS = _lib.COMPARE_MAX_ROWS
TORSION_NAMES = ("phi", "psi", "omega", "chi1", "chi2", "chi3", "chi4")

__all__ = ["COMPARE_MAX_BINS", "COMPARE_MAX_ROWS", "DIST_HIST_MAX_SEL", "DIVERGENCE_MAX_COLS", "TORSION_NAMES", "pair_index",
           "pair_table", "pair_matrix", "distance_histogram", "column_histogram", "histogram_divergence", "ensemble_compare"]


def pair_index(i, j, m):
    """The row of the pair (i < j) of m selection positions: CODLAD_DIST_HIST_PAIR of include/codlad_hip.h."""
    return i * m - i * (i + 1) // 2 + (j - i - 1)


def pair_table(m):
    """int64 numpy [m (m - 1) / 2, 2]: the (i, j) of every row, i ascending and j ascending within i."""
    i, j = np.triu_indices(m, 1)
    return np.stack((i, j), 1).astype(np.int64)


def _n_bins(n_bins, what, name="n_bins"):
    return _inputs.count(n_bins, name, COMPARE_MAX_BINS, what, types=(int, np.integer))      # numpy integers are taken here


def _pool(x, sel, what):
    x, sel, n_sel = _inputs.pool(x, sel, what, COMPARE_MAX_ROWS)
    m = n_sel or x.shape[1]
    if not 2 <= m <= DIST_HIST_MAX_SEL:
        raise ValueError(f"{what}: 2 .. {DIST_HIST_MAX_SEL} selected atoms, got {m}")
    return x, sel, n_sel, m


def _table_bytes(fn, rows, n_bins, what):
    nbytes = getattr(_lib.lib(), fn)(rows, n_bins)
    if nbytes < 0:
        raise ValueError(f"{what}: {_lib.lib().codlad_last_error().decode()}")
    return nbytes


def _dist_launch(x, sel, n_sel, m, inv_dr, n_bins, what):
    N, n = x.shape[:2]
    dev = x.device
    words = _table_bytes("codlad_dist_hist_bytes", m, n_bins, what) // 4
    H = torch.empty(words, dtype=torch.int32, device=dev).view(m * (m - 1) // 2, n_bins + 2)
    finite = _inputs.flags(N, dev)
    n_counted = torch.empty(2, dtype=torch.int32, device=dev)[:1]
    p = _lib.ptr
    rc = _lib.lib().codlad_dist_hist(p(x), N, n, p(sel), n_sel, inv_dr, n_bins, p(H), p(finite), p(n_counted), _lib.stream_ptr(dev))
    _lib.check(rc, "codlad_dist_hist")
    return H, finite.to(torch.bool), n_counted


def _grid(dr, r_max, n_bins, what):
    """(dr, r_max, n_bins) as given -> (n_bins, r_max, inv_dr as the kernel reads it): two of the three fix the grid; dr
    and n_bins given leave r_max = n_bins dr, dr and r_max given leave n_bins = ceil(r_max / dr)."""
    if dr is None:
        n_bins = _n_bins(n_bins, what)
        r_max = _inputs.positive(r_max, "r_max", what)
        dr = r_max / n_bins
    else:
        dr = _inputs.positive(dr, "dr", what)
        if r_max is None:
            n_bins = _n_bins(n_bins, what)
        else:
            n_bins = max(1, int(math.ceil(_inputs.positive(r_max, "r_max", what) / dr - 1e-9)))
            if n_bins > COMPARE_MAX_BINS:
                raise ValueError(f"{what}: at most {COMPARE_MAX_BINS} bins, r_max = {r_max} at dr = {dr} asks for {n_bins}")
        r_max = n_bins * dr
    inv_dr = np.float32(1.0 / dr)
    if not (np.isfinite(inv_dr) and inv_dr > 0):
        raise ValueError(f"{what}: the bin width {dr} has no float32 reciprocal")
    return n_bins, float(r_max), float(inv_dr)


def _box_diagonal(x, sel):
    """The largest bounding-box diagonal over the finite structures of x (a 0-dim float64 device tensor, -inf when there is
    none): no distance within a structure exceeds it."""
    xs = (x if sel is None else x[:, sel.to(torch.int64)]).to(torch.float64)
    ok = torch.isfinite(xs).all(dim=2).all(dim=1)
    span = xs.amax(dim=1) - xs.amin(dim=1)
    diag = torch.sqrt((span * span).sum(dim=1))
    return torch.where(ok, diag, torch.full_like(diag, -math.inf)).max()


def distance_histogram(x, sel=None, dr=None, r_max=None, n_bins=50):
    """The histogram over the pool x [N, n, 3] (device, N <= 1 048 576) of the distance of every pair of the atoms sel
    (default: all; 2 .. 2 048 of them) -> dict of device tensors:
      H int32 [P, n_bins + 2]    row p = the pair pairs[p]; column 1 + k counts the structures whose distance falls in
                                 [k dr, (k + 1) dr) by the fp32 decision include/codlad_hip.h states, the last column those at
                                 r_max or beyond, column 0 is always 0 (the layout column_histogram shares)
      edges float64 [n_bins + 1], finite bool [N] (False: a NaN or an infinity among the selected atoms - the structure takes
      no part), n_counted int32 [1] (every row of H sums to it), pairs int64 [P, 2] (selection POSITIONS i < j), r_max
    The grid: n_bins bins up to r_max (default: the largest bounding-box diagonal of the finite structures plus 1 A, rounded
    up to a whole A - one host read; the overflow column is then empty), or bins of width dr (n_bins of them, or up to a given
    r_max).  Integer counts: the bits repeat and a permuted pool gives the same H."""
    what = "distance_histogram"
    x, sel, n_sel, m = _pool(x, sel, what)
    if dr is None and r_max is None:
        _n_bins(n_bins, what)
        r_max = _default_r_max(float(_box_diagonal(x, sel)), what)
    n_bins, r_max, inv_dr = _grid(dr, r_max, n_bins, what)
    H, finite, n_counted = _dist_launch(x, sel, n_sel, m, inv_dr, n_bins, what)
    edges = torch.arange(n_bins + 1, dtype=torch.float64, device=x.device) * (r_max / n_bins)
    return dict(H=H, edges=edges, finite=finite, n_counted=n_counted, pairs=torch.from_numpy(pair_table(m)).to(x.device), r_max=r_max)


def _default_r_max(diag, what):
    if not math.isfinite(diag):
        raise ValueError(f"{what}: the pool has no finite structure")
    return float(math.ceil(diag + 1.0))


def column_histogram(values, lo, hi, n_bins, periodic=False):
    """The histogram over the structures of every column of values [N, C] (or [N]; device, any float type, read as float64):
    n_bins bins of width (hi - lo) / n_bins from lo -> dict: H int32 [C, n_bins + 2] - column 0 counts the values below lo,
    column 1 + k those in bin k, the last column those at hi or beyond; with periodic=True a value is wrapped into [lo, hi)
    first (torsions: lo = -180, hi = 180) and the outer columns stay 0 - and n_valid int32 [C], the values counted: a NaN or
    an infinity is not.  The float64 decision is stated in include/codlad_hip.h."""
    what = "column_histogram"
    _inputs.need_cuda(values, f"{what}: values")
    n_bins = _n_bins(n_bins, what)
    try:
        lo, hi = float(lo), float(hi)
    except (TypeError, ValueError):
        lo = hi = math.nan
    if not (math.isfinite(lo) and math.isfinite(hi) and hi > lo):
        raise ValueError(f"{what}: lo and hi must be finite numbers with lo < hi")
    inv_width = n_bins / (hi - lo)
    if not (math.isfinite(inv_width) and inv_width > 0):
        raise ValueError(f"{what}: the bin width (hi - lo) / n_bins has no float64 reciprocal")
    v = values.detach()
    if v.dim() == 1:
        v = v[:, None]
    if v.dim() != 2 or v.numel() == 0:
        raise ValueError(f"{what}: values must be a non-empty [N, C] tensor, got {tuple(values.shape)}")
    N, C = v.shape
    if N > COMPARE_MAX_ROWS or C > COMPARE_MAX_ROWS:
        raise ValueError(f"{what}: at most {COMPARE_MAX_ROWS} structures and columns, got {N} x {C}")
    v = v.to(torch.float64).contiguous()
    dev = v.device
    words = _table_bytes("codlad_column_hist_bytes", C, n_bins, what) // 4
    H = torch.empty(max(words, 2), dtype=torch.int32, device=dev)[:words].view(C, n_bins + 2)
    n_valid = torch.empty(max(C, 2), dtype=torch.int32, device=dev)[:C]
    p = _lib.ptr
    rc = _lib.lib().codlad_column_hist(p(v), N, C, lo, inv_width, n_bins, int(bool(periodic)), p(H), p(n_valid), _lib.stream_ptr(dev))
    _lib.check(rc, "codlad_column_hist")
    return dict(H=H, n_valid=n_valid)


def histogram_divergence(HA, HB):
    """Two count tables int32 [rows, cols] (or [cols]; device, 2 <= cols <= 4 098) -> dict of float64 [rows]: js, the
    Jensen-Shannon divergence of the rows' proportions in bits (0 .. 1); tv, the total variation (0 .. 1); w1, the
    1-Wasserstein distance in units of one column.  NaN for a row that is empty in either table or holds a negative count.
    Equal proportions give exactly 0 and swapping the tables gives the same bits (include/codlad_hip.h)."""
    what = "histogram_divergence"
    _inputs.need_cuda(HA, f"{what}: HA")
    _inputs.need_cuda(HB, f"{what}: HB")
    if HA.dim() == 1 and HB.dim() == 1:
        HA, HB = HA[None], HB[None]
    if HA.dim() != 2 or HA.shape != HB.shape or HA.device != HB.device or HA.shape[0] == 0:
        raise ValueError(f"{what}: two tables of one shape [rows, cols] on one device, got {tuple(HA.shape)} and {tuple(HB.shape)}")
    if HA.dtype.is_floating_point or HB.dtype.is_floating_point:
        raise ValueError(f"{what}: the tables hold integer counts (weighted histograms are not supported)")
    rows, cols = HA.shape
    if not 2 <= cols <= DIVERGENCE_MAX_COLS:
        raise ValueError(f"{what}: 2 .. {DIVERGENCE_MAX_COLS} columns, got {cols}")
    if rows * cols >= 1 << 31:
        raise ValueError(f"{what}: rows x cols must stay below 2^31, got {rows} x {cols}")
    a, b = (t.detach().to(torch.int32).contiguous() for t in (HA, HB))
    out = torch.empty(3, max(rows, 2), dtype=torch.float64, device=a.device)
    js, tv, w1 = (out[k, :rows] for k in range(3))
    p = _lib.ptr
    rc = _lib.lib().codlad_hist_divergence(p(a), p(b), rows, cols, p(js), p(tv), p(w1), _lib.stream_ptr(a.device))
    _lib.check(rc, "codlad_hist_divergence")
    return dict(js=js, tv=tv, w1=w1)


def pair_matrix(v, m):
    """A per-pair vector v [P], P = m (m - 1) / 2 in distance_histogram's row order -> the symmetric [m, m] with a zero
    diagonal."""
    P = m * (m - 1) // 2
    if v.dim() != 1 or v.shape[0] != P:
        raise ValueError(f"pair_matrix: {m} atoms have {P} pairs, got {tuple(v.shape)}")
    i, j = torch.triu_indices(m, m, 1, device=v.device)
    M = torch.zeros(m, m, dtype=v.dtype, device=v.device)
    M[i, j] = v
    M[j, i] = v
    return M


def _nanmean(t, dim=None):
    ok = ~torch.isnan(t)
    z = torch.where(ok, t, torch.zeros_like(t))
    if dim is None:
        return z.sum() / ok.sum()
    return z.sum(dim) / ok.sum(dim)


def _torsion_table(s):
    """stereo_check's dict -> float64 [S, R * 7]: phi, psi, omega, chi1 .. chi4 per residue; NaN where the residue has no
    such angle, and in every angle of a residue flagged undefined."""
    v = s["values"][..., :7].to(torch.float64)
    undefined = (s["flags"] & _lib.STEREO_FLAGS["undefined"]) != 0
    v = torch.where(undefined[..., None], torch.full_like(v, math.nan), v)
    return v.reshape(v.shape[0], -1)


def ensemble_compare(a, b, top=None, sel=None, n_bins=50, r_max=None, torsion_bins=36, rg_bins=50, cluster_cutoff=None,
                     min_separation=2):
    """How far the distributions of the pool a [Na, n, 3] are from those of the pool b [Nb, n, 3] (device; one topology; for
    instance generated against true frames), over the atoms sel (default: all; 2 .. 2 048) -> dict of device tensors:
      js_dist [m, m]            the Jensen-Shannon divergence (bits, 0 .. 1) of the distance distributions of every atom
                                pair, both pools binned on ONE grid of n_bins bins up to r_max (default: the larger
                                bounding-box diagonal of the finite structures of both pools plus 1 A, rounded up to a whole
                                A - the overflow column is then empty); symmetric, zero diagonal
      w1_dist [m, m]            their 1-Wasserstein distance in A
      js_dist_mean, js_dist_median   over the pairs with |i - j| >= min_separation selection positions
      js_rg, w1_rg              of the radius of gyration over sel (w1 in A), rg_bins bins on a range taken from both pools
      r_max, n_a, n_b           the grid's end and the structures of each pool that took part
      overflow                  the counts of both pools at r_max or beyond (0 with the default r_max)
    with top (a dataset_builder.Topology; a and b hold all its atoms):
      js_torsion [R, 7]         per residue the divergence of phi, psi, omega, chi1 .. chi4 (TORSION_NAMES), periodic
                                histograms of torsion_bins bins on [-180, 180); NaN where either pool has no valid value
      js_torsion_mean [7]       the mean per angle type over the residues that have it
    with cluster_cutoff (A): the two pools are clustered as ONE pool (metrics.cluster over sel) and each pool's cluster
      populations form a one-row count table -> js_cluster (ENCORE's CES) and n_clusters
    ValueError for pools of different atom counts, fewer than 2 or more than 2 048 selected atoms, a bin count outside
    1 .. 256, a pool without a finite structure, or more clusters than histogram_divergence takes columns."""
    from .cluster import cluster
    from .observables import radius_of_gyration
    from .stereo import stereo_check
    what = "ensemble_compare"
    _inputs.need_cuda(a, f"{what}: a")
    _inputs.need_cuda(b, f"{what}: b")
    n_bins = _n_bins(n_bins, what)
    torsion_bins = _n_bins(torsion_bins, what, "torsion_bins")
    rg_bins = _n_bins(rg_bins, what, "rg_bins")
    if isinstance(min_separation, bool) or not isinstance(min_separation, int) or min_separation < 1:
        raise ValueError(f"{what}: min_separation must be a positive integer, got {min_separation!r}")
    if a.dim() == 3 and b.dim() == 3 and a.shape[1] != b.shape[1]:
        raise ValueError(f"{what}: the pools have {a.shape[1]} and {b.shape[1]} atoms: one topology, one selection")
    a, sel_d, n_sel, m = _pool(a, sel, what)
    b = _pool(b, sel, what)[0]
    if b.device != a.device:
        raise ValueError(f"{what}: the pools are on different devices")
    if top is not None and top.n_atoms != a.shape[1]:
        raise ValueError(f"{what}: the pools have {a.shape[1]} atoms, the topology {top.n_atoms}")
    dev = a.device
    # distances: one grid for both pools
    if r_max is None:
        diag = torch.stack((_box_diagonal(a, sel_d), _box_diagonal(b, sel_d))).tolist()          # the one host read
        if not min(diag) > -math.inf:
            raise ValueError(f"{what}: a pool has no finite structure")
        r_max = _default_r_max(max(diag), what)
    n_bins, r_max, inv_dr = _grid(None, r_max, n_bins, what)
    HA, fin_a, n_a = _dist_launch(a, sel_d, n_sel, m, inv_dr, n_bins, what)
    HB, fin_b, n_b = _dist_launch(b, sel_d, n_sel, m, inv_dr, n_bins, what)
    n_a, n_b = int(n_a), int(n_b)
    if not (n_a and n_b):
        raise ValueError(f"{what}: a pool has no finite structure")
    d = histogram_divergence(HA, HB)
    pairs = torch.from_numpy(pair_table(m)).to(dev)
    far = (pairs[:, 1] - pairs[:, 0]) >= min_separation
    js_far = d["js"][far]
    nan = torch.full((), math.nan, dtype=torch.float64, device=dev)
    out = dict(js_dist=pair_matrix(d["js"], m), w1_dist=pair_matrix(d["w1"] * (r_max / n_bins), m),
               js_dist_mean=js_far.mean() if js_far.numel() else nan, js_dist_median=js_far.median() if js_far.numel() else nan,
               r_max=r_max, n_a=n_a, n_b=n_b, overflow=HA[:, -1].sum() + HB[:, -1].sum())
    # radius of gyration: a common range from both pools, widened so that the largest value falls inside
    rg_a, rg_b = radius_of_gyration(a, sel), radius_of_gyration(b, sel)
    both = torch.cat((rg_a[fin_a], rg_b[fin_b]))
    lo, hi = float(both.min()), float(both.max())
    pad = max((hi - lo) * 1e-6, abs(hi) * 1e-12, 1e-12)
    lo, hi = lo - pad, hi + pad
    ra = column_histogram(torch.where(fin_a, rg_a, nan), lo, hi, rg_bins)["H"]
    rb = column_histogram(torch.where(fin_b, rg_b, nan), lo, hi, rg_bins)["H"]
    dr_ = histogram_divergence(ra, rb)
    out.update(js_rg=dr_["js"][0], w1_rg=dr_["w1"][0] * ((hi - lo) / rg_bins))
    if top is not None:
        ta, tb = _torsion_table(stereo_check(a, top)), _torsion_table(stereo_check(b, top))
        ha = column_histogram(ta, -180.0, 180.0, torsion_bins, periodic=True)["H"]
        hb = column_histogram(tb, -180.0, 180.0, torsion_bins, periodic=True)["H"]
        js_t = histogram_divergence(ha, hb)["js"].view(top.n_residues, 7)
        out.update(js_torsion=js_t, js_torsion_mean=_nanmean(js_t, 0))
    if cluster_cutoff is not None:
        cl = cluster(torch.cat((a, b)), cluster_cutoff, sel=sel)
        K = int(cl["n_clusters"])
        if K > DIVERGENCE_MAX_COLS:
            raise ValueError(f"{what}: {K} clusters at the cut-off {cluster_cutoff}, at most {DIVERGENCE_MAX_COLS} "
                             "(choose a larger cut-off)")
        lab = cl["labels"].to(torch.int64)
        cols = max(K, 2)                                              # one cluster: a second, empty column
        pa = torch.bincount(lab[:a.shape[0]][lab[:a.shape[0]] >= 0], minlength=cols).to(torch.int32)
        pb = torch.bincount(lab[a.shape[0]:][lab[a.shape[0]:] >= 0], minlength=cols).to(torch.int32)
        out.update(js_cluster=histogram_divergence(pa, pb)["js"][0], n_clusters=K)
    return out
