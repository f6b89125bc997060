"""Typed pair-distance histograms of an ensemble (codlad_pair_hist, csrc/pair_hist_kernels.hip) and what follows from
them (codlad_pair_hist_profile): for every structure an integer count of atom pairs per (type a <= type b, distance bin) -
q-independent, one pass over the pairs - from which the pair distribution P(r) with D_max and a real-space Rg, and the
SAXS profile on ANY q grid, are short float64 combinations.  The profile is FoXS's route and a stated approximation of
the Debye sum of saxs_profile: every distance is read at the centre of its bin, so with bins of width dr
  |I_hist(q) - I_debye(q)| <= 0.43618 q (dr / 2) 2 sum_{i<j} |f_i f_j|       (0.43618 = max |d sinc(x) / dx|)
up to the fp32 rounding of the bin decision."""
import math

import numpy as np
import torch

from .. import _lib
from . import _inputs
from .saxs import SAXS_MAX_Q, SAXS_MAX_TYPES, SAXS_Q_LIMIT, _host, default_q, form_factors, saxs_groups

PAIR_HIST_MAX_BINS, PAIR_HIST_MAX_ATOMS = _lib.PAIR_HIST_MAX_BINS, _lib.PAIR_HIST_MAX_ATOMS
PAIR_HIST_ITEM_COLS = 2048         # the columns of a work item: 64 rows x 2048 columns, 512 pairs a lane
PAIR_HIST_RESIDUE_LENGTH, PAIR_HIST_MARGIN = 3.85, 30.0      # A: the default r_max, per residue and per chain

__all__ = ["PAIR_HIST_MAX_BINS", "PAIR_HIST_MAX_ATOMS", "PAIR_HIST_ITEM_COLS", "pair_class_index", "pair_classes",
           "contour_r_max", "pair_histogram_lists", "pair_histogram", "pair_distribution", "pair_distribution_lists",
           "saxs_profile_hist", "saxs_profile_hist_lists"]


def pair_class_index(a, b, n_types):
    """The row of the class (a <= b) among n_types types: CODLAD_PAIR_HIST_CLASS of include/codlad_hip.h."""
    return a * n_types - a * (a - 1) // 2 + (b - a)


def pair_classes(n_types):
    """int64 numpy [T (T + 1) / 2, 2]: the (a, b) of every class row, a ascending and b ascending within a."""
    return np.array([(a, b) for a in range(n_types) for b in range(a, n_types)], dtype=np.int64).reshape(-1, 2)


def contour_r_max(top):
    """The default r_max of a topology: PAIR_HIST_RESIDUE_LENGTH = 3.85 A (the CA-CA distance of a trans peptide) per
    residue plus PAIR_HIST_MARGIN = 30 A (two extended side chains), summed over the chains.  A bound on every distance
    within INTACT chains that touch; a broken chain or chains that drifted apart can exceed it (then `overflow` says so)."""
    chains = {}
    for c in top.chain_ids:
        chains[c] = chains.get(c, 0) + 1
    return sum(PAIR_HIST_RESIDUE_LENGTH * n + PAIR_HIST_MARGIN for n in chains.values())


def _bins(dr, r_max):
    """dr and r_max checked -> (dr, the number of bins, inv_dr as the kernel reads it)."""
    try:
        dr, r_max = float(dr), float(r_max)
    except (TypeError, ValueError):
        raise ValueError(f"pair_hist: dr and r_max must be numbers, got {dr!r} and {r_max!r}") from None
    if not (math.isfinite(dr) and dr > 0 and math.isfinite(r_max) and r_max > 0):
        raise ValueError(f"pair_hist: dr and r_max must be positive numbers, got {dr!r} and {r_max!r}")
    inv_dr = np.float32(1.0 / dr)
    n_bins = max(1, int(math.ceil(r_max / dr - 1e-9)))
    if n_bins > PAIR_HIST_MAX_BINS or not (np.isfinite(inv_dr) and inv_dr > 0):
        raise ValueError(f"pair_hist: at most {PAIR_HIST_MAX_BINS} bins, r_max = {r_max} A at dr = {dr} A asks for {n_bins} "
                         "(choose a wider bin or a shorter r_max)")
    return dr, n_bins, inv_dr


def _work_items(type_start, cols=PAIR_HIST_ITEM_COLS):
    """The cut of all pairs into codlad_pair_hist's items (a, b, row0, col0, col1), int32 numpy [n_items, 5]: tiles of 64
    sorted positions of type a against at most `cols` sorted positions of type b; when a = b the columns start behind the
    tile's first row (the kernel keeps column > row).  Never empty: (0, 0, 0, 0, 0) is an item without a pair."""
    items = []
    T = len(type_start) - 1
    for a in range(T):
        a0, a1 = int(type_start[a]), int(type_start[a + 1])
        for b in range(a, T):
            b1 = int(type_start[b + 1])
            for row0 in range(a0, a1, _lib.PAIR_HIST_ROWS):
                for c0 in range(row0 + 1 if a == b else int(type_start[b]), b1, cols):
                    items.append((a, b, row0, c0, min(c0 + cols, b1)))
    return np.array(items or [(0, 0, 0, 0, 0)], dtype=np.int32).reshape(-1, _lib.PAIR_HIST_ITEM_WORDS)


def _hist_tables(types, n_types, dr, r_max, dev):
    """The checked tables of codlad_pair_hist on `dev` -> dict: order int32 [n], type_start int32 [T + 1], items int32
    [n_items, 5], count int32 [T], classes int64 [C, 2], edges float64 [B + 1], and dr, inv_dr, n_bins, n_types."""
    dr, n_bins, inv_dr = _bins(dr, r_max)
    typ = _host(types, np.int64).reshape(-1)
    T = int(n_types)
    if not 1 <= T <= SAXS_MAX_TYPES:
        raise ValueError(f"pair_hist: 1 .. {SAXS_MAX_TYPES} atom types, got {T}")
    if typ.shape[0] > PAIR_HIST_MAX_ATOMS:
        raise ValueError(f"pair_hist: at most {PAIR_HIST_MAX_ATOMS} atoms (a count fits an int32), got {typ.shape[0]}")
    if not typ.shape[0] or typ.min() < 0 or typ.max() >= T:
        raise ValueError(f"pair_hist: every atom type must be in [0, {T})")
    order = np.argsort(typ, kind="stable").astype(np.int32)                 # by type, ties ascending
    count = np.bincount(typ, minlength=T).astype(np.int32)
    start = np.concatenate([[0], np.cumsum(count)]).astype(np.int32)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)      # noqa: E731
    return dict(order=up(order), type_start=up(start), items=up(_work_items(start)), count=up(count),
                classes=up(pair_classes(T)), edges=up(np.arange(n_bins + 1, dtype=np.float64) * dr), dr=dr, inv_dr=float(inv_dr),
                n_bins=n_bins, n_types=T)


def _hist_launch(xyz, t):
    x = _inputs.structures(xyz, "pair_hist: xyz", t["order"].shape[0])
    dev = x.device
    S, n, T, B = x.shape[0], x.shape[1], t["n_types"], t["n_bins"]
    C = T * (T + 1) // 2
    H = torch.empty(S, C, B, dtype=torch.int32, device=dev)
    over = torch.empty(S, C, dtype=torch.int32, device=dev)
    d_bin = torch.empty(S, dtype=torch.int32, device=dev)
    finite = torch.empty(S, dtype=torch.uint8, device=dev)
    p = _lib.ptr
    rc = _lib.lib().codlad_pair_hist(p(x), S, n, p(t["order"]), p(t["type_start"]), T, t["inv_dr"], B, p(t["items"]),
                                     t["items"].shape[0], p(H), p(over), p(d_bin), p(finite), _lib.stream_ptr(dev))
    _lib.check(rc, "codlad_pair_hist")
    return dict(H=H, over=over, d_bin=d_bin, finite=finite.to(torch.bool), edges=t["edges"], classes=t["classes"],
                count=t["count"], dr=t["dr"])


def pair_histogram_lists(xyz, types, n_types, dr=0.5, r_max=100.0):
    """The typed pair-distance histogram of xyz [S, n_atoms, 3] (device) with types int [n_atoms] in [0, n_types) and
    B = ceil(r_max / dr) bins of width dr (A) -> dict of device tensors:
      H int32 [S, C, B]      the pairs i < j of class c = pair_class_index(a, b, n_types), a <= b their types, whose
                             distance falls in [bin dr, (bin + 1) dr): the fp32 decision include/codlad_hip.h states
      over int32 [S, C]      the pairs at r_max or beyond: none is left out silently
      d_bin int32 [S]        the highest occupied bin over all classes, -1 if there is no pair
      finite bool [S]        False: a coordinate is NaN or +-inf - H, over and d_bin of the structure are -1
      edges float64 [B + 1], classes int64 [C, 2] (the (a, b) of every row), count int32 [n_types], dr
    Integer counts: the bits repeat from call to call and do not depend on the order of the atoms or on the batch.
    ValueError for dr or r_max that is not a positive number, more than PAIR_HIST_MAX_BINS bins, more than
    PAIR_HIST_MAX_ATOMS atoms, n_types outside 1 .. SAXS_MAX_TYPES or a type outside [0, n_types).  The tables are rebuilt
    on every call: for repeated calls on a protein use pair_histogram."""
    _inputs.need_cuda(xyz, "pair_hist: xyz")
    return _hist_launch(xyz, _hist_tables(types, n_types, dr, r_max, xyz.device))


def pair_histogram(xyz, top, dr=0.5, r_max=None):
    """pair_histogram_lists of xyz [S, n_atoms, 3] (device), S structures of the topology `top`, with the types of
    saxs_groups(top).  r_max None: contour_r_max(top), a bound for intact chains.  The tables are built once per
    (topology, dr, r_max, device); no host transfer."""
    _inputs.need_cuda(xyz, "pair_hist: xyz")
    r_max = contour_r_max(top) if r_max is None else r_max
    _bins(dr, r_max)

    def build():
        groups, types = saxs_groups(top)
        return _hist_tables(types, len(groups), dr, r_max, xyz.device)
    return _hist_launch(xyz, _inputs.cached(top, "_pair_hist_tables", (float(dr), float(r_max), str(xyz.device)), build))


def _hist_of(what, xyz, top, dr, r_max, hist):
    """The histogram a derived quantity starts from: `hist` checked against the topology, or a fresh pair_histogram."""
    if hist is None:
        return pair_histogram(xyz, top, dr, r_max)
    _hist_of_lists(what, hist)
    n_groups = _inputs.cached(top, "_pair_hist_groups", "n", lambda: len(saxs_groups(top)[0]))
    if hist["count"].shape[0] != n_groups:
        raise ValueError(f"{what}: hist has {hist['count'].shape[0]} types, the topology {n_groups}")
    return hist


def _profile_launch(h, ff=None, sinc=None, w=None, r2=None, with_mean=True):
    """codlad_pair_hist_profile on a histogram dict: the profile when ff and sinc are given, the pair distribution when w
    and r2 are."""
    H, dev = h["H"], h["H"].device
    S, C, B = H.shape
    T = h["count"].shape[0]
    finite = h["finite"].to(torch.uint8)
    complete = torch.empty(S, dtype=torch.uint8, device=dev)
    new = lambda *shape: torch.empty(*shape, dtype=torch.float64, device=dev)      # noqa: E731
    Q = ff.shape[1] if ff is not None else 0
    partial, I, mean_I, P, I0, m2, mean_P = (None,) * 7
    if ff is not None:
        partial, I, mean_I = new(S, C, Q), new(S, Q), new(Q) if with_mean else None
    if w is not None:
        P, I0, m2, mean_P = new(S, B), new(S), new(S), new(B) if with_mean else None
    p = _lib.ptr
    rc = _lib.lib().codlad_pair_hist_profile(p(H), p(h["over"]), p(h["d_bin"]), p(finite), S, T, B, p(h["count"]), p(ff), p(sinc), Q,
                                             p(partial), p(I), p(mean_I), p(w), p(r2), p(P), p(I0), p(m2), p(mean_P), p(complete),
                                             _lib.stream_ptr(dev))
    _lib.check(rc, "codlad_pair_hist_profile")
    return dict(I=I, mean_I=mean_I, P=P, I0=I0, m2=m2, mean_P=mean_P, complete=complete.to(torch.bool))


def pair_distribution(xyz, top, dr=0.5, r_max=None, solvent_density=0.334, hist=None):
    """The pair distribution P(r) of xyz [S, n_atoms, 3] (device), S structures of the topology `top`: the typed histogram
    weighted with the forward amplitudes w = form_factors([0], saxs_groups(top), solvent_density) -> dict of device tensors:
      r float64 [B]          the bin centres (bin + 1/2) dr
      P float64 [S, B]       sum over the classes (a <= b) of w_a w_b H[s][c][bin], every pair once; 0 beyond d_bin
      mean float64 [B]       the average over the finite structures without overflow, added in index order
      d_max float64 [S]      (d_bin + 1) dr: the upper edge of the highest occupied bin; 0 without a pair
      I0 float64 [S]         sum_i w_i^2 + 2 sum_bin P: the forward scattering (sum_i w_i)^2 of the pairs below r_max
      rg float64 [S]         sqrt(sum_bin r^2 P / I0): the real-space radius of gyration (NaN where I0 <= 0)
      finite bool [S]        False: a coordinate is NaN or +-inf - NaN in every row
      overflow bool [S]      True: pairs at r_max or beyond are missing from P, I0 and rg (they hold for r < r_max)
    r_max None: contour_r_max(top), a bound for intact chains.  hist: a pair_histogram result of the same topology (then
    xyz, dr and r_max are not read).  The tables are built once per (topology, dr, r_max, solvent_density, device); no host
    transfer; float64 sums in one order (include/codlad_hip.h), so the bits repeat."""
    if hist is None:
        _inputs.need_cuda(xyz, "pair_hist: xyz")
    h = _hist_of("pair_distribution", xyz, top, dr, r_max, hist)
    dev, B, step = h["H"].device, h["H"].shape[2], float(h["dr"])

    def build():
        r = (np.arange(B, dtype=np.float64) + 0.5) * step
        w = form_factors([0.0], saxs_groups(top)[0], solvent_density)[:, 0]
        return tuple(torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (r, r * r, w))
    r, r2, w = _inputs.cached(top, "_pair_distribution_tables", (step, B, float(solvent_density), str(dev)), build)
    out = _profile_launch(h, w=w, r2=r2)
    return dict(r=r, **_pr_result(h, out, step))


def _pr_result(h, out, step):
    d_max = torch.where(h["finite"], (h["d_bin"] + 1).to(torch.float64) * step, torch.full_like(out["I0"], float("nan")))
    return dict(P=out["P"], mean=out["mean_P"], d_max=d_max, I0=out["I0"], rg=torch.sqrt(out["m2"] / out["I0"]),
                finite=h["finite"], overflow=(h["over"] > 0).any(dim=1))


def _device_table(a, shape, what, dev):
    a = _host(a, np.float64)
    if a.shape != tuple(shape) or not np.isfinite(a).all():
        raise ValueError(f"{what} must be {list(shape)} finite numbers, got {list(a.shape)}")
    return torch.from_numpy(np.array(a)).to(dev)


def pair_distribution_lists(hist, weights):
    """pair_distribution's P, mean, d_max, I0, rg, finite and overflow of a pair_histogram_lists result `hist` with one
    weight per type, weights [n_types] (float64)."""
    h = _hist_of_lists("pair_distribution_lists", hist)
    dev, B, step = h["H"].device, h["H"].shape[2], float(h["dr"])
    r = (np.arange(B, dtype=np.float64) + 0.5) * step
    w = _device_table(weights, (h["count"].shape[0],), "pair_distribution_lists: weights", dev)
    return _pr_result(h, _profile_launch(h, w=w, r2=torch.from_numpy(r * r).to(dev)), step)


def saxs_profile_hist_lists(hist, table, q):
    """saxs_profile_hist's I, mean and complete of a pair_histogram_lists result `hist` with table [n_types, Q] (float64, the
    form factor of every type at every q) and q [Q] in [0, SAXS_Q_LIMIT] (float64)."""
    h = _hist_of_lists("saxs_profile_hist_lists", hist)
    dev, B, step = h["H"].device, h["H"].shape[2], float(h["dr"])
    q64 = _check_q("saxs_profile_hist_lists", q)
    ff = _device_table(table, (h["count"].shape[0], q64.shape[0]), "saxs_profile_hist_lists: table", dev)
    out = _profile_launch(h, ff=ff, sinc=torch.from_numpy(_sinc_table(q64, B, step)).to(dev))
    return dict(I=out["I"], mean=out["mean_I"], complete=out["complete"])


def _hist_of_lists(what, hist):
    need = ("H", "over", "d_bin", "finite", "count", "dr")
    if not isinstance(hist, dict) or any(k not in hist for k in need):
        raise ValueError(f"{what}: hist must be a result of pair_histogram (a dict with {', '.join(need)})")
    _inputs.need_cuda(hist["H"], f"{what}: hist")
    T = hist["count"].shape[0]
    if hist["H"].dim() != 3 or hist["H"].shape[1] != T * (T + 1) // 2:
        raise ValueError(f"{what}: hist has {T} types and H {tuple(hist['H'].shape)}")
    return hist


def _check_q(what, q):
    q64 = _host(default_q() if q is None else q, np.float64).reshape(-1)
    if not 1 <= q64.shape[0] <= SAXS_MAX_Q:
        raise ValueError(f"{what}: 1 .. {SAXS_MAX_Q} q values, got {q64.shape[0]}")
    if not (np.isfinite(q64).all() and (q64 >= 0).all() and (q64 <= SAXS_Q_LIMIT).all()):
        raise ValueError(f"{what}: every q must be a number in [0, {SAXS_Q_LIMIT}] 1/A")
    return q64


def _sinc_table(q, n_bins, dr):
    """float64 numpy [B, Q]: sinc(q_k (bin + 1/2) dr), sinc(0) = 1."""
    x = ((np.arange(n_bins, dtype=np.float64) + 0.5) * dr)[:, None] * q[None, :]
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(x == 0.0, 1.0, np.sin(x) / x)


def saxs_profile_hist(xyz, top, q=None, dr=0.5, r_max=None, solvent_density=0.334, hist=None):
    """SAXS profiles from the typed pair-distance histogram: saxs_profile's dict
      q float32 [Q], I float64 [S, Q], mean float64 [Q], finite bool [S], n_finite
    plus complete bool [S]: False for a structure with pairs at r_max or beyond, whose row of I is NaN (a profile that
    lacks pairs is wrong, never silently truncated); mean is over the finite and complete structures.  Every distance is
    read at the centre of its bin: I = sum_a n_a f_a^2 + 2 sum_c f_a f_b sum_bin H sinc(q (bin + 1/2) dr), within the bound
    of the module docstring of saxs_profile's Debye sum.  The form factors are form_factors(q, ...) and the sinc table in
    float64, from q as given (not rounded to float32).  hist: a pair_histogram result of the same topology - the pair walk is
    skipped (xyz, dr and r_max are not read): another q grid without another pass over the pairs.  ValueError for a q
    outside [0, SAXS_Q_LIMIT] or more than SAXS_MAX_Q of them, and pair_histogram's refusals.  The tables are built once
    per (topology, q, dr, bins, solvent_density, device)."""
    if hist is None:
        _inputs.need_cuda(xyz, "pair_hist: xyz")
    q64 = _check_q("saxs_profile_hist", q)
    h = _hist_of("saxs_profile_hist", xyz, top, dr, r_max, hist)
    dev, B, step = h["H"].device, h["H"].shape[2], float(h["dr"])

    def build():
        ff = form_factors(q64, saxs_groups(top)[0], solvent_density)
        return (torch.from_numpy(np.ascontiguousarray(ff)).to(dev), torch.from_numpy(_sinc_table(q64, B, step)).to(dev),
                torch.from_numpy(q64.astype(np.float32)).to(dev))
    ff, sinc, qd = _inputs.cached(top, "_saxs_hist_tables", (q64.tobytes(), step, B, float(solvent_density), str(dev)), build)
    out = _profile_launch(h, ff=ff, sinc=sinc)
    return dict(q=qd, I=out["I"], mean=out["mean_I"], finite=h["finite"], n_finite=h["finite"].sum(), complete=out["complete"])
