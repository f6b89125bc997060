"""Drop-in for the evaluation helpers of the reference's test loop (reference test.py:97-166, called at
test.py:589-593), computed on the GPU by one fused pass (`codlad_eval_metrics`) instead of ~60 ATen ops
and, for the clash metric, a sort-based `unique` per call.  Same names, argument order and return values
as the reference functions; tensors must be on the GPU (no CPU path).

`evaluate` computes all eight numbers in one launch; the per-metric functions call it with the lists
they need.  The clash list (rows of cat(edge_list, nbr_list) occurring once) depends on the topology
only and is cached per (edge_list, nbr_list) pair.

`geometry_check` needs no true structure: generated structures against the template topology they were built from
(broken / spurious covalent bonds, clashes; codlad_geometry_check, one all-pairs launch).
"""
import ctypes as C

import torch

from . import _lib

NAMES = ("loss_bond", "loss_angle", "loss_torsion", "loss_xyz", "loss_graph", "loss_nbr", "loss_inter", "loss_pi_pi")
_CLASH_CACHE = {}


def _need_cuda(t, what):
    if t is not None and not t.is_cuda:
        raise RuntimeError(f"{what} must be a CUDA tensor: the metrics run on the MI355X only")


def clash_list(edge_list, nbr_list):
    """Rows of cat(edge_list, nbr_list) that occur exactly once (reference test.py:121-123)."""
    key = (edge_list.data_ptr(), edge_list._version, tuple(edge_list.shape),
           nbr_list.data_ptr(), nbr_list._version, tuple(nbr_list.shape))
    if key not in _CLASH_CACHE:
        if len(_CLASH_CACHE) > 16:
            _CLASH_CACHE.clear()
        both = torch.cat((edge_list, nbr_list)).to(torch.int64)
        big = int(both.max()) + 1 if both.numel() else 1
        codes, counts = (both[:, 0] * big + both[:, 1]).unique(return_counts=True)   # sorted like unique(dim=0)
        once = codes[counts == 1]
        _CLASH_CACHE[key] = (torch.stack((once // big, once % big), 1).contiguous(), edge_list, nbr_list)
    return _CLASH_CACHE[key][0]


def evaluate(xyz_recon=None, xyz=None, edge_list=None, clash=None, bb_NO_list=None, interaction_list=None,
             pi_pi_list=None, ic_recon=None, ic=None, mask=None):
    """-> float32 tensor [8] on the device, in the order of NAMES; absent inputs leave their entries 0
    (or NaN for the reconstruction losses, which divide by the mask count like the reference)."""
    dev = next(t for t in (xyz_recon, ic_recon) if t is not None).device
    lib = _lib.lib()
    keep = []

    def f32(t, what):
        if t is None:
            return None, 0
        _need_cuda(t, what)
        t = t.detach().to(torch.float32).contiguous()
        keep.append(t)
        return t, t.shape[0]

    def i64(t, what, width):
        if t is None or t.shape[0] == 0:
            return None, 0
        _need_cuda(t, what)
        t = t.detach().to(torch.int64).contiguous()
        assert t.dim() == 2 and t.shape[1] == width, what
        keep.append(t)
        return t, t.shape[0]

    m = _lib.MetricInputs()
    xr, n_atoms = f32(xyz_recon, "xyz_recon")
    xt, _ = f32(xyz if xyz is not None else xyz_recon, "xyz")
    m.xyz_recon, m.xyz, m.n_atoms = _lib.ptr(xr), _lib.ptr(xt), n_atoms
    for field, count, t, width in (("edge_list", "n_edges", edge_list if xyz is not None else None, 2),
                                   ("clash_list", "n_clash", clash, 2), ("bb_NO_list", "n_bb", bb_NO_list, 2),
                                   ("interaction_list", "n_inter", interaction_list, 2),
                                   ("pi_pi_list", "n_pipi", pi_pi_list, 4)):
        tt, n = i64(t, field, width)
        setattr(m, field, _lib.ptr(tt))
        setattr(m, count, n)
    if ic_recon is not None:
        a, _ = f32(ic.reshape(-1, 3), "ic")
        b, n_ic = f32(ic_recon.reshape(-1, 3), "ic_recon")
        k, _ = f32(mask.reshape(-1), "mask")
        assert a.shape == b.shape and k.shape[0] == n_ic
        m.ic, m.ic_recon, m.ic_mask, m.n_ic = _lib.ptr(a), _lib.ptr(b), _lib.ptr(k), n_ic
    out = torch.zeros(8, dtype=torch.float32, device=dev)
    scratch = torch.empty(lib.codlad_metrics_scratch_bytes(), dtype=torch.uint8, device=dev)
    rc = lib.codlad_eval_metrics(C.byref(m), _lib.ptr(out), _lib.ptr(scratch), _lib.stream_ptr(dev))
    _lib.check(rc, "codlad_eval_metrics")
    return out


def recon_result(ic_recon, ic, mask_):
    o = evaluate(ic_recon=ic_recon, ic=ic, mask=mask_)
    return o[0], o[1], o[2]


def xyz_result(xyz_recon, xyz):
    return evaluate(xyz_recon=xyz_recon, xyz=xyz)[3]


def ged_result(xyz_recon, xyz, edge_list):
    return evaluate(xyz_recon=xyz_recon, xyz=xyz, edge_list=edge_list)[4]


def clash_result(edge_list, nbr_list, xyz_recon, bb_NO_list):
    return evaluate(xyz_recon=xyz_recon, clash=clash_list(edge_list, nbr_list), bb_NO_list=bb_NO_list)[5]


def inter_result(interaction_list, pi_pi_list, xyz_recon):
    o = evaluate(xyz_recon=xyz_recon, interaction_list=interaction_list, pi_pi_list=pi_pi_list)
    return o[6], o[7]


def all_results(ic_recon, ic, mask_, xyz_recon, xyz, edge_list, nbr_list, bb_NO_list, interaction_list, pi_pi_list):
    """The five calls of reference test.py:589-593 as one launch -> dict of 0-d device tensors."""
    o = evaluate(xyz_recon=xyz_recon, xyz=xyz, edge_list=edge_list, clash=clash_list(edge_list, nbr_list),
                 bb_NO_list=bb_NO_list, interaction_list=interaction_list, pi_pi_list=pi_pi_list,
                 ic_recon=ic_recon, ic=ic, mask=mask_)
    return dict(zip(NAMES, o))


# Covalent cut-off radii by atomic number 1..107 (the reference's COVCUTOFFTABLE, utils/protein_module.py:128-234: a
# table of constants, kept as data)
COV_CUTOFF = (0.23, 0.93, 0.68, 0.35, 0.83, 0.68, 0.68, 0.68, 0.64, 1.12, 0.97, 1.1, 1.35, 1.2, 0.75, 1.02, 0.99, 1.57,
              1.33, 0.99, 1.44, 1.47, 1.33, 1.35, 1.35, 1.34, 1.33, 1.5, 1.52, 1.45, 1.22, 1.17, 1.21, 1.22, 1.21, 1.91,
              1.47, 1.12, 1.78, 1.56, 1.48, 1.47, 1.35, 1.4, 1.45, 1.5, 1.59, 1.69, 1.63, 1.46, 1.46, 1.47, 1.4, 1.98,
              1.67, 1.34, 1.87, 1.83, 1.82, 1.81, 1.8, 1.8, 1.99, 1.79, 1.76, 1.75, 1.74, 1.73, 1.72, 1.94, 1.72, 1.57,
              1.43, 1.37, 1.35, 1.37, 1.32, 1.5, 1.5, 1.7, 1.55, 1.54, 1.54, 1.68, 1.7, 2.4, 2.0, 1.9, 1.88, 1.79, 1.61,
              1.58, 1.55, 1.53, 1.51, 1.5, 1.5, 1.5, 1.5, 1.5, 1.5, 1.5, 1.5, 1.57, 1.49, 1.43, 1.41)


def bond_graph_counts(xyz, xyz_recon, num_atoms, atomic_nums, scale=1.3):
    """int32 [n_struct, 6] on the device: per structure {bonds in xyz, bonds in xyz_recon, differing pairs} over all
    atoms and over heavy atoms (codlad_bond_graph_counts)."""
    _need_cuda(xyz, "xyz")
    _need_cuda(xyz_recon, "xyz_recon")
    dev = xyz.device
    z = torch.as_tensor(atomic_nums).to(torch.int64).cpu()
    if int(z.min()) < 1 or int(z.max()) > len(COV_CUTOFF):
        raise ValueError("atomic number outside the covalent cut-off table (1..107)")
    radius = torch.tensor(COV_CUTOFF, dtype=torch.float32)[z - 1].to(dev)
    heavy = (z != 1).to(torch.int32).to(dev)
    na = [int(n) for n in torch.as_tensor(num_atoms).tolist()]
    assert sum(na) == xyz.shape[0] == xyz_recon.shape[0] == z.numel()
    ptr = torch.zeros(len(na) + 1, dtype=torch.int32)
    ptr[1:] = torch.cumsum(torch.tensor(na, dtype=torch.int64), 0).to(torch.int32)
    ptr = ptr.to(dev)
    counts = torch.empty(len(na), 6, dtype=torch.int32, device=dev)
    a = xyz.detach().to(torch.float32).contiguous()
    b = xyz_recon.detach().to(torch.float32).contiguous()
    rc = _lib.lib().codlad_bond_graph_counts(_lib.ptr(a), _lib.ptr(b), _lib.ptr(radius), _lib.ptr(heavy), _lib.ptr(ptr),
                                             len(na), max(na), C.c_float(scale), _lib.ptr(counts), _lib.stream_ptr(dev))
    _lib.check(rc, "codlad_bond_graph_counts")
    return counts


def valid_ratio_and_cut_off_result(xyz, xyz_recon, num_atoms, atomic_nums):
    """Drop-in for reference test.py:168-188: per structure, whether the bond graph of the reconstruction equals the
    reference's (heavy atoms / all atoms) and the relative difference of their bond counts, returned as the
    reference returns them: four lists with one entry per structure (the graph ratios as one-element lists, as
    count_valid_graphs does).  The ASE Atoms objects of the reference are plain containers here."""
    cnt = bond_graph_counts(xyz, xyz_recon, num_atoms, atomic_nums).cpu().to(torch.int64)
    heavy_valid, all_valid, heavy_ged, all_ged = [], [], [], []
    for ref_a, gen_a, diff_a, ref_h, gen_h, diff_h in cnt.tolist():
        heavy_valid.append(1.0 if diff_h == 0 else 0.0)
        all_valid.append(1.0 if diff_a == 0 else 0.0)
        # (ref_graph - gen_graph).sum().abs() / ref_graph.sum() on the full 0/1 matrices (each pair counted twice)
        heavy_ged.append([(torch.tensor(2 * (ref_h - gen_h)).abs() / torch.tensor(2 * ref_h)).item()])
        all_ged.append([(torch.tensor(2 * (ref_a - gen_a)).abs() / torch.tensor(2 * ref_a)).item()])
    return heavy_valid, all_valid, heavy_ged, all_ged


def superposed_rmsd(a, b):
    """Minimal RMSD of two conformations [n_atoms, 3] after optimal rigid superposition (what mdtraj's md.rmsd
    returns for single-frame trajectories, reference test.py:52-53, 74-75): Kabsch, RMSD^2 = (|a|^2 + |b|^2 -
    2 (s1 + s2 + sign(det) s3)) / n with s the singular values of the 3x3 covariance of the centred coordinates.
    mdtraj is not available offline: PARITY UNPINNED (published algorithm)."""
    a = a.to(torch.float64) - a.to(torch.float64).mean(0)
    b = b.to(torch.float64) - b.to(torch.float64).mean(0)
    cov = (a.t() @ b).cpu()
    u, sv, vt = torch.linalg.svd(cov)
    d = torch.sign(torch.linalg.det(u @ vt))
    e0 = float((a * a).sum() + (b * b).sum())
    msd = max(e0 - 2.0 * float(sv[0] + sv[1] + d * sv[2]), 0.0) / a.shape[0]
    return msd ** 0.5


# --- Superposition on the device (codlad_ens_*, csrc/ensemble_kernels.hip): minimal RMSD under a proper rotation plus
# translation for many pairs per launch, fp64 after an exact conversion of the fp32 coordinates, deterministic sums.

def _coords(t, what, dims):
    _need_cuda(t, what)
    if t.dim() != dims or t.shape[-1] != 3 or t.numel() == 0:
        raise ValueError(f"{what} must be a non-empty [{', '.join('?' * (dims - 1))}, 3] tensor, got {tuple(t.shape)}")
    return t.detach().to(torch.float32).contiguous()


def _selection(sel, n_atoms, dev):
    """sel (index list / tensor, or None) -> (int32 device tensor or None, count for the C ABI)."""
    if sel is None:
        return None, 0
    idx = torch.as_tensor(sel).reshape(-1).to(torch.int64)
    if idx.numel() == 0:
        raise ValueError("sel is empty")
    if int(idx.min()) < 0 or int(idx.max()) >= n_atoms:
        raise ValueError(f"sel has an index outside [0, {n_atoms})")
    return idx.to(device=dev, dtype=torch.int32).contiguous(), idx.numel()


def _moments(x, n_conf, n_atoms, sel, n_sel):
    mom = torch.empty(n_conf, 4, dtype=torch.float64, device=x.device)
    _lib.check(_lib.lib().codlad_ens_moments(_lib.ptr(x), n_conf, n_atoms, _lib.ptr(sel), n_sel, _lib.ptr(mom),
                                             _lib.stream_ptr(x.device)), "codlad_ens_moments")
    return mom


def _pair_msd(A, B, pairs, sel, n_sel, squared, want_transform):
    """A [nA, n, 3], B [nB, n, 3] fp32 pools, pairs int32 [P, 2] (device) -> out [P] (and Rt [P, 12] or None)."""
    nA, n_atoms, nB, P = A.shape[0], A.shape[1], B.shape[0], pairs.shape[0]
    momA, momB = _moments(A, nA, n_atoms, sel, n_sel), _moments(B, nB, n_atoms, sel, n_sel)
    out = torch.empty(P, dtype=torch.float64, device=A.device)
    Rt = torch.empty(P, 12, dtype=torch.float64, device=A.device) if want_transform else None
    rc = _lib.lib().codlad_ens_pair_msd(_lib.ptr(A), _lib.ptr(momA), nA, _lib.ptr(B), _lib.ptr(momB), nB, n_atoms,
                                        _lib.ptr(sel), n_sel, _lib.ptr(pairs), P, int(bool(squared)), _lib.ptr(out),
                                        _lib.ptr(Rt), _lib.stream_ptr(A.device))
    _lib.check(rc, "codlad_ens_pair_msd")
    return out, Rt


def _one_to_one(a, b, what):
    """a [P, n, 3], b [P, n, 3] or [n, 3] -> fp32 pools and the pair list (k, k) or (k, 0)."""
    a = _coords(a, f"{what}: a", 3)
    b = _coords(b, f"{what}: b", b.dim() if b.dim() in (2, 3) else 3)
    if b.dim() == 2:
        b = b[None]
    P, n = a.shape[0], a.shape[1]
    if b.shape[1] != n or b.shape[0] not in (1, P) or b.device != a.device:
        raise ValueError(f"{what}: b {tuple(b.shape)} does not match a {tuple(a.shape)} (b is [P, n, 3] or [n, 3], same device)")
    k = torch.arange(P, dtype=torch.int32, device=a.device)
    pairs = torch.stack((k, k if b.shape[0] == P else torch.zeros_like(k)), 1).contiguous()
    return a, b, pairs


def superposed_rmsd_batch(a, b, sel=None, squared=False, return_transform=False):
    """Minimal RMSD of a[k] onto b[k] (b [P, n, 3]) or onto the one target b [n, 3], after the optimal proper rotation
    plus translation, for all P pairs in one launch set.  -> float64 [P] on the device (the msd with squared=True);
    with return_transform also float64 R [P, 3, 3] and t [P, 3] such that a @ R.T + t is superposed on b.  sel: the atom
    indices the fit and the RMSD use (default: all)."""
    a, b, pairs = _one_to_one(a, b, "superposed_rmsd_batch")
    sel, n_sel = _selection(sel, a.shape[1], a.device)
    out, Rt = _pair_msd(a, b, pairs, sel, n_sel, squared, return_transform)
    if return_transform:
        return out, Rt[:, :9].reshape(-1, 3, 3), Rt[:, 9:]
    return out


def superpose(a, b, sel=None):
    """-> fp32 [P, n, 3]: ALL atoms of every a[k] moved by the transform that superposes its atoms `sel` (default: all)
    on those of b[k] (or of the one target b [n, 3]); computed in fp64 and rounded once."""
    a, b, pairs = _one_to_one(a, b, "superpose")
    sel, n_sel = _selection(sel, a.shape[1], a.device)
    _out, Rt = _pair_msd(a, b, pairs, sel, n_sel, True, True)
    moved = torch.empty_like(a)
    _lib.check(_lib.lib().codlad_ens_apply(_lib.ptr(a), _lib.ptr(Rt), a.shape[0], a.shape[1], _lib.ptr(moved),
                                           _lib.stream_ptr(a.device)), "codlad_ens_apply")
    return moved


def pairwise_rmsd(x, sel=None):
    """x [G, F, n, 3] (members x frames) -> float64 [F, G, G]: the superposed RMSD of every pair of members of a frame.
    The upper triangle is computed (bit for bit what superposed_rmsd_batch gives for the pair) and mirrored; the diagonal
    is written as 0."""
    x = _coords(x, "pairwise_rmsd: x", 4)
    G, F, n = x.shape[:3]
    sel, n_sel = _selection(sel, n, x.device)
    mom = _moments(x, G * F, n, sel, n_sel)
    out = torch.empty(F, G, G, dtype=torch.float64, device=x.device)
    _lib.check(_lib.lib().codlad_ens_pairwise(_lib.ptr(x), _lib.ptr(mom), G, F, n, _lib.ptr(sel), n_sel, 0,
                                              _lib.ptr(out), _lib.stream_ptr(x.device)), "codlad_ens_pairwise")
    return out


def diversity_terms(gen, ref):
    """The two RMSD tables of the diversity score.  gen [G, F, n, 3] (or a list of G [F, n, 3]), ref [F, n, 3] ->
    float64 [G, F] RMSD of gen[g, p] to ref[p], and [G, F] RMSD of gen[g, p] to the UNALIGNED member mean gen.mean(0)[p]
    (the reference takes np.mean of the raw structures).  One launch set for both tables."""
    if isinstance(gen, (list, tuple)):
        gen = torch.stack([torch.as_tensor(g) for g in gen])
    gen = _coords(gen, "diversity_terms: gen", 4)
    ref = _coords(ref, "diversity_terms: ref", 3)
    G, F, n = gen.shape[:3]
    if tuple(ref.shape) != (F, n, 3) or ref.device != gen.device:
        raise ValueError(f"diversity_terms: ref {tuple(ref.shape)} does not match gen {tuple(gen.shape)}")
    targets = torch.cat((ref, gen.mean(0)))                      # [2 F, n, 3]: pool B
    k = torch.arange(G * F, dtype=torch.int32, device=gen.device)
    p = k % F
    pairs = torch.cat((torch.stack((k, p), 1), torch.stack((k, p + F), 1))).contiguous()
    out, _ = _pair_msd(gen.reshape(G * F, n, 3), targets, pairs, None, 0, False, False)
    return out[:G * F].reshape(G, F), out[G * F:].reshape(G, F)


def compute_div(gen_structures, ref_structure):
    """Diversity score of reference test.py:37-95: 1 - (mean RMSD of every generated frame to the mean generated
    structure) / (mean RMSD of every generated frame to the reference frame).  gen_structures: list (ensemble members)
    of [n_frames, n_atoms, 3]; ref_structure [n_frames, n_atoms, 3].  CUDA tensors take the device path
    (diversity_terms: two launches for all G x F x 2 superpositions, one transfer of the final scalar); CPU tensors the
    float64 SVD loop over superposed_rmsd."""
    gen = [torch.as_tensor(g) for g in gen_structures]
    ref = torch.as_tensor(ref_structure)
    if ref.is_cuda:
        to_ref, to_mean = diversity_terms(gen, ref)
        return float(1.0 - to_mean.mean() / to_ref.mean())
    mean_gen = torch.stack(gen).mean(0)
    to_ref = [superposed_rmsd(g[p], ref[p]) for g in gen for p in range(g.shape[0])]
    to_mean = [superposed_rmsd(g[p], mean_gen[p]) for g in gen for p in range(g.shape[0])]
    return 1.0 - (sum(to_mean) / len(to_mean)) / (sum(to_ref) / len(to_ref))


# --- Reference-free geometry check (codlad_geometry_check, csrc/geometry_kernels.hip): generated structures judged
# against the template topology they were built from, with no true coordinates.

GEOMETRY_COUNTS = ("broken", "spurious", "bonded", "near", "clash")


def exclusion_csr(bonds, order, n_atoms):
    """The pairs within `order` bonds (dataset_builder.high_order_edges' pair set) as the CSR codlad_geometry_check reads:
    (ptr int32 [n_atoms + 1], partners int32) - row i lists, sorted, every j != i within `order` bonds of i (so the list
    is symmetric), with _lib.GEOM_BOND_FLAG set on the bonded (order-1) ones.  Walks adjacency lists: no n x n matrix."""
    adj = [set() for _ in range(n_atoms)]
    for i, j in torch.as_tensor(bonds).reshape(-1, 2).tolist():
        if not (0 <= i < n_atoms and 0 <= j < n_atoms) or i == j:
            raise ValueError(f"bond ({i}, {j}) is not a pair of different atoms of [0, {n_atoms})")
        adj[i].add(j)
        adj[j].add(i)
    ptr, words = [0], []
    for i in range(n_atoms):
        seen, frontier = {i}, {i}
        for _ in range(order):
            frontier = {k for f in frontier for k in adj[f]} - seen
            seen |= frontier
        seen.discard(i)
        words += [j | _lib.GEOM_BOND_FLAG if j in adj[i] else j for j in sorted(seen)]
        ptr.append(len(words))
    return torch.tensor(ptr, dtype=torch.int32), torch.tensor(words, dtype=torch.int32)


def _geometry_tables(top, order, dev):
    """(radius, excl_ptr, excl, bonds) of a topology on `dev`, built once and kept ON the topology object (its lifetime,
    no key that a reused address could alias)."""
    cache = top.__dict__.setdefault("_geometry_tables", {})
    key = (int(order), str(dev))
    if key not in cache:
        from .utils.dataset_builder import standard_bonds
        z = torch.as_tensor(top.atomic_nums()).to(torch.int64)
        if z.numel() and (int(z.min()) < 1 or int(z.max()) > len(COV_CUTOFF)):
            raise ValueError("atomic number outside the covalent cut-off table (1..107)")
        bonds = standard_bonds(top)
        ptr, words = exclusion_csr(bonds, order, top.n_atoms)
        cache[key] = (torch.tensor(COV_CUTOFF, dtype=torch.float32)[z - 1].to(dev).contiguous(), ptr.to(dev), words.to(dev),
                      bonds.to(torch.int32).to(dev).contiguous())
    return cache[key]


def _geometry_launch(xyz, radius, ptr_, words, bonds, scale, clash_dist, near_dist):
    _need_cuda(xyz, "xyz")
    if xyz.dim() != 3 or xyz.shape[-1] != 3 or xyz.shape[0] == 0:
        raise ValueError(f"geometry_check: xyz must be a non-empty [S, n_atoms, 3] tensor, got {tuple(xyz.shape)}")
    if xyz.shape[1] != radius.shape[0] or ptr_.shape[0] != radius.shape[0] + 1:
        raise ValueError(f"geometry_check: xyz has {xyz.shape[1]} atoms, the topology {radius.shape[0]}")
    dev = xyz.device
    x = xyz.detach().to(torch.float32).contiguous()
    S = x.shape[0]
    counts = torch.empty(S, 5, dtype=torch.int32, device=dev)
    min_dist = torch.empty(S, dtype=torch.float32, device=dev)
    rc = _lib.lib().codlad_geometry_check(_lib.ptr(x), S, x.shape[1], _lib.ptr(radius), _lib.ptr(ptr_), _lib.ptr(words),
                                          _lib.ptr(bonds), bonds.shape[0], C.c_float(scale), C.c_float(clash_dist),
                                          C.c_float(near_dist), _lib.ptr(counts), _lib.ptr(min_dist), _lib.stream_ptr(dev))
    _lib.check(rc, "codlad_geometry_check")
    out = {k: counts[:, c] for c, k in enumerate(GEOMETRY_COUNTS)}
    out.update(counts=counts, min_dist=min_dist, valid=(counts[:, 0] == 0) & (counts[:, 1] == 0) & ~torch.isnan(min_dist))
    return out


def geometry_check_lists(xyz, radius, bonds, order=2, scale=1.3, clash_dist=1.2, near_dist=9.0):
    """geometry_check for a topology given as lists: radius [n_atoms] (covalent cut-off radii), bonds [n_bonds, 2] (each
    bond once, i < j).  The exclusion list is rebuilt on every call: for repeated calls on a protein use geometry_check."""
    _need_cuda(xyz, "xyz")
    dev = xyz.device
    bonds = torch.as_tensor(bonds).reshape(-1, 2).to(torch.int64).cpu()
    if bonds.numel() and not bool((bonds[:, 0] < bonds[:, 1]).all()):
        raise ValueError("geometry_check: bonds must be pairs i < j")
    radius = torch.as_tensor(radius).detach().to(torch.float32).reshape(-1)
    ptr_, words = exclusion_csr(bonds, order, radius.shape[0])
    return _geometry_launch(xyz, radius.to(dev).contiguous(), ptr_.to(dev), words.to(dev),
                            bonds.to(torch.int32).to(dev).contiguous(), scale, clash_dist, near_dist)


def geometry_check(xyz, top, order=2, scale=1.3, clash_dist=1.2, near_dist=9.0):
    """xyz [S, n_atoms, 3] (device): S structures of the topology `top` (a dataset_builder.Topology of the written, i.e.
    interior, residues) -> dict of device tensors, one entry per structure, over unordered atom pairs:
      broken    template bonds (standard_bonds) not at d < (r_i + r_j) * scale, r = COV_CUTOFF of the element (a bond
                whose d is not a number is broken)
      spurious  pairs at d < (r_i + r_j) * scale that are no template bond
      bonded    all pairs at d < (r_i + r_j) * scale (= n_bonds - broken + spurious)
      near      pairs more than `order` bonds apart at d <= near_dist
      clash     of those, the ones at sqrt(d^2 + 1e-7) < clash_dist (clash / near: the first term of clash_result with
                the structure's own neighbour list)
      min_dist  the smallest d over pairs more than `order` bonds apart (inf: there is none; NaN: a coordinate of the
                structure is NaN or +-inf)
      valid     broken == 0 and spurious == 0 and min_dist is not NaN: the covalent graph of the structure IS the
                template's.  A structure with a non-finite coordinate is never valid: a comparison with a NaN distance is
                false, so its pairs are in no count but `broken`, and bonded == n_bonds - broken + spurious still holds.
    and `counts`, the five counts as one int32 [S, 5] in the order of GEOMETRY_COUNTS.  One launch, no host transfer."""
    _need_cuda(xyz, "xyz")
    if xyz.dim() == 3 and xyz.shape[1] != top.n_atoms:
        raise ValueError(f"geometry_check: xyz has {xyz.shape[1]} atoms, the topology {top.n_atoms}")
    if order < 1:
        raise ValueError(f"geometry_check: order must be >= 1, got {order}")
    return _geometry_launch(xyz, *_geometry_tables(top, order, xyz.device), scale, clash_dist, near_dist)


# --- Stereochemistry check (codlad_stereo_check, csrc/stereo_kernels.hip): the torsions and chiral volumes of generated
# structures and the decisions taken on them - the part of the reference-free judgement the covalent graph cannot see.

STEREO_COLUMNS = ("phi", "psi", "omega", "chi1", "chi2", "chi3", "chi4", "v_ca", "v_side")
STEREO_COUNTS = ("inverted_ca", "inverted_side", "cis_pro", "cis_nonpro", "twisted", "undefined")
STEREO_FLAGS = _lib.STEREO_FLAGS           # name -> bit of `flags`
# the side-chain path of a residue: chi_k is the torsion of its atoms k - 1 .. k + 2 (IUPAC: the branch with the lower number)
CHI_PATH = {nm: ["N", "CA", "CB"] + tail.split() for nm, tail in {
    "ALA": "", "GLY": "", "ARG": "CG CD NE CZ", "ASN": "CG OD1", "ASP": "CG OD1", "CYS": "SG", "GLN": "CG CD OE1",
    "GLU": "CG CD OE1", "HIS": "CG ND1", "ILE": "CG1 CD1", "LEU": "CG CD1", "LYS": "CG CD CE NZ", "MET": "CG SD CE",
    "PHE": "CG CD1", "PRO": "CG CD", "SER": "OG", "SEP": "OG", "THR": "OG1", "TPO": "OG1", "TRP": "CG CD1", "TYR": "CG CD1",
    "VAL": "CG1"}.items()}
SIDE_CENTRE = {"THR": "OG1", "TPO": "OG1", "ILE": "CG1"}       # the residues with a chiral CB: X of v_side


def stereo_tables(top):
    """(sites int32 [n_res, 9, 4], res_kind uint8 [n_res]) of a dataset_builder.Topology, on the host: the atoms of the nine
    quantities of STEREO_COLUMNS per residue, by atom name (codlad_stereo_check's layout, include/codlad_hip.h).  A row
    that holds a -1 is a quantity the residue does not have: no phi / omega before the first residue of a chain and no psi
    after the last (neighbours are consecutive residues with equal chain_ids, standard_bonds' peptide-bond rule), as many
    chi as the residue type has, no v_ca for GLY, v_side for THR / TPO / ILE only.  Bit 0 of res_kind: the residue is PRO.
    Built once and kept on the topology object."""
    cache = top.__dict__.setdefault("_stereo_tables", {})
    if "host" not in cache:
        n_res = top.n_residues
        sites = torch.full((n_res, len(STEREO_COLUMNS), 4), -1, dtype=torch.int32)
        kind = torch.zeros(n_res, dtype=torch.uint8)
        for r, nm in enumerate(top.res_names):
            at = lambda name, d=0: top.atom(r + d, name)                                                    # noqa: E731
            prev = r > 0 and top.chain_ids[r - 1] == top.chain_ids[r]
            nxt = r + 1 < n_res and top.chain_ids[r + 1] == top.chain_ids[r]
            rows = [[at("C", -1), at("N"), at("CA"), at("C")] if prev else None,
                    [at("N"), at("CA"), at("C"), at("N", 1)] if nxt else None,
                    [at("CA", -1), at("C", -1), at("N"), at("CA")] if prev else None]
            path = CHI_PATH.get(nm, [])
            rows += [[at(a) for a in path[k:k + 4]] if k + 4 <= len(path) else None for k in range(4)]
            rows.append([at("CA"), at("N"), at("C"), at("CB")])
            rows.append([at("CB"), at("CA"), at(SIDE_CENTRE[nm]), at("CG2")] if nm in SIDE_CENTRE else None)
            for q, row in enumerate(rows):
                if row is not None and min(row) >= 0:
                    sites[r, q] = torch.tensor(row, dtype=torch.int32)
            kind[r] = _lib.STEREO_KIND_PRO if nm == "PRO" else 0
        cache["host"] = (sites, kind)
    return cache["host"]


def stereo_check(xyz, top):
    """xyz [S, n_atoms, 3] (device): S structures of the topology `top` -> dict of device tensors; R = top.n_residues:
      phi, psi, omega [S, R]   backbone torsions of the residue, degrees in (-180, 180]; omega is the peptide bond INTO it
      chi [S, R, 4]            side-chain torsions chi1 .. chi4
      v_ca, v_side [S, R]      signed volumes (A^3) at CA (> 0: an L residue) and at the CB of THR / TPO / ILE (> 0: natural)
      values [S, R, 9]         all of the above in the order of STEREO_COLUMNS; NaN = the residue has no such quantity
      flags uint8 [S, R]       STEREO_FLAGS: inverted_ca, inverted_side (the volume is finite and not > 0), cis
                               (|omega| < 30), twisted (30 <= |omega| <= 150), undefined (a quantity the residue has is not finite)
      counts int32 [S, 6]      residues per structure in the order of STEREO_COUNTS, each also under its name
      stereo_ok bool [S]       inverted_ca, inverted_side, cis_nonpro, twisted and undefined are all 0 (cis-PRO occurs in nature)
    One launch, no host transfer.  A statement about geometry, like geometry_check's `valid`, not about accuracy."""
    _need_cuda(xyz, "xyz")
    if xyz.dim() != 3 or xyz.shape[-1] != 3 or xyz.shape[0] == 0:
        raise ValueError(f"stereo_check: xyz must be a non-empty [S, n_atoms, 3] tensor, got {tuple(xyz.shape)}")
    if xyz.shape[1] != top.n_atoms:
        raise ValueError(f"stereo_check: xyz has {xyz.shape[1]} atoms, the topology {top.n_atoms}")
    dev = xyz.device
    cache = top.__dict__.setdefault("_stereo_tables", {})
    if str(dev) not in cache:
        cache[str(dev)] = tuple(t.to(dev).contiguous() for t in stereo_tables(top))
    sites, kind = cache[str(dev)]
    x = xyz.detach().to(torch.float32).contiguous()
    S, R = x.shape[0], top.n_residues
    values = torch.empty(S, R, len(STEREO_COLUMNS), dtype=torch.float32, device=dev)
    flags = torch.empty(S, R, dtype=torch.uint8, device=dev)
    counts = torch.empty(S, len(STEREO_COUNTS), dtype=torch.int32, device=dev)
    rc = _lib.lib().codlad_stereo_check(_lib.ptr(x), S, x.shape[1], _lib.ptr(sites), _lib.ptr(kind), R, _lib.ptr(values),
                                        _lib.ptr(flags), _lib.ptr(counts), _lib.stream_ptr(dev))
    _lib.check(rc, "codlad_stereo_check")
    out = {k: counts[:, c] for c, k in enumerate(STEREO_COUNTS)}
    bad = [c for c, k in enumerate(STEREO_COUNTS) if k != "cis_pro"]
    out.update(phi=values[..., 0], psi=values[..., 1], omega=values[..., 2], chi=values[..., 3:7], v_ca=values[..., 7],
               v_side=values[..., 8], values=values, flags=flags, counts=counts, stereo_ok=(counts[:, bad] == 0).all(dim=1))
    return out


# --- Restrained clash relaxation (codlad_relax, csrc/relax_kernels.hip): what follows the two checks - atoms that overlap
# are pushed apart while every distance within two bonds and every torsion about a rigid bond is held to the input's.

RELAX_DEFAULTS = dict(k_r=100.0, k_t=50.0, k_c=30.0, contact_scale=1.6, h0=0.01, h_max=0.1)
RELAX_ENERGIES = ("distance", "torsion", "repulsion")


def ring_bonds(bonds, n_atoms):
    """The bonds (i, j), i < j, whose ends stay connected when the bond is removed: the ring bonds of any bond graph."""
    adj = [set() for _ in range(n_atoms)]
    pairs = sorted({(min(i, j), max(i, j)) for i, j in torch.as_tensor(bonds).reshape(-1, 2).tolist()})
    for i, j in pairs:
        adj[i].add(j)
        adj[j].add(i)
    out = []
    for i, j in pairs:
        seen, stack = {i}, [i]
        while stack and j not in seen:
            a = stack.pop()
            for b in adj[a]:
                if b not in seen and (a, b) != (i, j):
                    seen.add(b)
                    stack.append(b)
        if j in seen:
            out.append((i, j))
    return out


def torsion_quads(bonds, rigid, n_atoms):
    """int32 [Q, 4]: for every rigid bond b - c every (a, b, c, d) with a in adj(b) \\ {c}, d in adj(c) \\ {b}, a != d."""
    adj = [set() for _ in range(n_atoms)]
    for i, j in torch.as_tensor(bonds).reshape(-1, 2).tolist():
        adj[i].add(j)
        adj[j].add(i)
    quads = [(a, b, c, d) for b, c in sorted({(min(p), max(p)) for p in rigid})
             for a in sorted(adj[b] - {c}) for d in sorted(adj[c] - {b}) if a != d]
    return torch.tensor(quads, dtype=torch.int32).reshape(-1, 4)


def quad_csr(quads, n_atoms):
    """(ptr int32 [n_atoms + 1], refs int32): per atom the quads it is part of, as 4 * quad + position, ascending."""
    quads = torch.as_tensor(quads).reshape(-1, 4).to(torch.int64)
    if quads.numel() and (int(quads.min()) < 0 or int(quads.max()) >= n_atoms):
        raise ValueError(f"a quad has an atom outside [0, {n_atoms})")
    atoms = quads.reshape(-1)
    order = torch.argsort(atoms, stable=True)                 # refs of an atom ascend: they are the flat positions
    ptr = torch.zeros(n_atoms + 1, dtype=torch.int64)
    ptr[1:] = torch.cumsum(torch.bincount(atoms, minlength=n_atoms), 0)
    return ptr.to(torch.int32), order.to(torch.int32)


def relax_tables(top, order=2):
    """The host tables of the relaxation of a dataset_builder.Topology -> dict, built once and kept on the topology object:
      radius float32 [n]                COV_CUTOFF of the element
      pair_ptr, pair_j                  exclusion_csr(bonds, 2, n): the pairs whose distance is restrained
      excl_ptr, excl                    exclusion_csr(bonds, order, n): the pairs that are never repelled
      rigid int64 [B, 2]                the rigid bonds: ring bonds (ring_bonds), the peptide bond C - N, ARG NE - CZ
      quads int32 [Q, 4]                torsion_quads over them; quad_ptr, quad_ref: quad_csr
      fixed bool [n]                    the default fixed mask: the CA atoms (a backmapped structure stays on its CG input)"""
    cache = top.__dict__.setdefault("_relax_tables", {})
    key = (int(order), "host")
    if key not in cache:
        from .utils.dataset_builder import standard_bonds
        z = torch.as_tensor(top.atomic_nums()).to(torch.int64)
        if z.numel() and (int(z.min()) < 1 or int(z.max()) > len(COV_CUTOFF)):
            raise ValueError("atomic number outside the covalent cut-off table (1..107)")
        n = top.n_atoms
        bonds = standard_bonds(top)
        rigid = set(ring_bonds(bonds, n))
        for r, nm in enumerate(top.res_names):
            if r + 1 < top.n_residues and top.chain_ids[r + 1] == top.chain_ids[r]:
                rigid.add((top.atom(r, "C"), top.atom(r + 1, "N")))
            if nm == "ARG":
                rigid.add((top.atom(r, "NE"), top.atom(r, "CZ")))
        have = {tuple(b) for b in bonds.tolist()}
        rigid = sorted(p for p in {(min(p), max(p)) for p in rigid} if p in have)       # a residue that lacks an atom: -1
        quads = torsion_quads(bonds, rigid, n)
        pair_ptr, pair_j = exclusion_csr(bonds, 2, n)
        excl_ptr, excl = (pair_ptr, pair_j) if order == 2 else exclusion_csr(bonds, order, n)
        quad_ptr, quad_ref = quad_csr(quads, n)
        cache[key] = dict(radius=torch.tensor(COV_CUTOFF, dtype=torch.float32)[z - 1].contiguous(), pair_ptr=pair_ptr, pair_j=pair_j,
                          excl_ptr=excl_ptr, excl=excl, rigid=torch.tensor(rigid, dtype=torch.int64).reshape(-1, 2), quads=quads,
                          quad_ptr=quad_ptr, quad_ref=quad_ref, fixed=torch.from_numpy(top.name == "CA"))
    return cache[key]


_RELAX_DEVICE_KEYS = ("radius", "excl_ptr", "excl", "pair_ptr", "pair_j", "quads", "quad_ptr", "quad_ref")


def _relax_device_tables(tab, dev):
    return {k: tab[k].to(dev).contiguous() for k in _RELAX_DEVICE_KEYS}


def _relax_tables_on(top, order, dev):
    cache = top.__dict__.setdefault("_relax_tables", {})
    key = (int(order), str(dev))
    if key not in cache:
        cache[key] = _relax_device_tables(relax_tables(top, order), dev)
    return cache[key]


def _relax_lists_tables(radius, bonds, quads, order, dev):
    bonds = torch.as_tensor(bonds).reshape(-1, 2).to(torch.int64).cpu()
    if bonds.numel() and not bool((bonds[:, 0] < bonds[:, 1]).all()):
        raise ValueError("relax: bonds must be pairs i < j")
    radius = torch.as_tensor(radius).detach().to(torch.float32).reshape(-1)
    n = radius.shape[0]
    quads = torch.as_tensor(quads).reshape(-1, 4).to(torch.int32).cpu()
    pair_ptr, pair_j = exclusion_csr(bonds, 2, n)
    excl_ptr, excl = (pair_ptr, pair_j) if order == 2 else exclusion_csr(bonds, order, n)
    quad_ptr, quad_ref = quad_csr(quads, n)
    return _relax_device_tables(dict(radius=radius, pair_ptr=pair_ptr, pair_j=pair_j, excl_ptr=excl_ptr, excl=excl, quads=quads,
                                     quad_ptr=quad_ptr, quad_ref=quad_ref), dev)


def _relax_constants(constants, names):
    bad = set(constants) - set(names)
    if bad:
        raise TypeError(f"relax: unknown constant(s) {sorted(bad)} (known: {', '.join(names)})")
    return [C.c_float(float(constants.get(k, RELAX_DEFAULTS[k]))) for k in names]


def _relax_inputs(xyz, tab, fixed, what):
    _need_cuda(xyz, "xyz")
    n = tab["radius"].shape[0]
    if xyz.dim() != 3 or xyz.shape[-1] != 3 or xyz.shape[0] == 0:
        raise ValueError(f"{what}: xyz must be a non-empty [S, n_atoms, 3] tensor, got {tuple(xyz.shape)}")
    if xyz.shape[1] != n:
        raise ValueError(f"{what}: xyz has {xyz.shape[1]} atoms, the topology {n}")
    fixed = torch.as_tensor(fixed).reshape(-1)
    if fixed.shape[0] != n:
        raise ValueError(f"{what}: the fixed mask has {fixed.shape[0]} atoms, the topology {n}")
    return xyz.detach().to(torch.float32).contiguous(), fixed.to(device=xyz.device, dtype=torch.bool).to(torch.uint8).contiguous()


def _relax_table_args(t):
    p = _lib.ptr
    return [p(t["excl_ptr"]), p(t["excl"]) if t["excl"].numel() else None, p(t["pair_ptr"]),
            p(t["pair_j"]) if t["pair_j"].numel() else None, t["pair_j"].shape[0],
            p(t["quads"]) if t["quads"].numel() else None, t["quads"].shape[0], p(t["quad_ptr"]),
            p(t["quad_ref"]) if t["quad_ref"].numel() else None, t["quad_ref"].shape[0]]


def _relax_scratch(S, t, n_iter, dev):
    size = _lib.lib().codlad_relax_scratch_bytes(S, t["radius"].shape[0], t["pair_j"].shape[0], t["quads"].shape[0], n_iter)
    if size < 0:
        raise ValueError("relax: bad counts")
    return torch.empty(max(size, 8), dtype=torch.uint8, device=dev)


def _relax_energy_launch(xyz, xyz0, t, fixed, constants):
    x, fx = _relax_inputs(xyz, t, fixed, "relax_energy")
    x0 = x if xyz0 is None else _relax_inputs(xyz0, t, fixed, "relax_energy: xyz0")[0]
    if x0.shape != x.shape or x0.device != x.device:
        raise ValueError(f"relax_energy: xyz0 {tuple(x0.shape)} does not match xyz {tuple(x.shape)} (same shape, same device)")
    dev, S, n = x.device, x.shape[0], x.shape[1]
    energy = torch.empty(S, 3, dtype=torch.float64, device=dev)
    grad = torch.empty(S, n, 3, dtype=torch.float32, device=dev)
    gmax = torch.empty(S, dtype=torch.float32, device=dev)
    scratch = _relax_scratch(S, t, -1, dev)
    p = _lib.ptr
    rc = _lib.lib().codlad_relax_energy(p(x), p(x0), S, n, p(t["radius"]), p(fx), *_relax_table_args(t),
                                        *_relax_constants(constants, ("k_r", "k_t", "k_c", "contact_scale")), p(energy), p(grad),
                                        p(gmax), p(scratch), _lib.stream_ptr(dev))
    _lib.check(rc, "codlad_relax_energy")
    return dict(energy=energy, grad=grad, gmax=gmax, total=(energy[:, 0] + energy[:, 1]) + energy[:, 2])


def _relax_launch(xyz, t, fixed, n_iter, constants):
    x, fx = _relax_inputs(xyz, t, fixed, "relax")
    n_iter = int(n_iter)
    if n_iter < 0:
        raise ValueError(f"relax: n_iter must be >= 0, got {n_iter}")
    dev, S, n = x.device, x.shape[0], x.shape[1]
    out = torch.empty_like(x)
    tr = dict(energy=torch.empty(S, n_iter + 1, dtype=torch.float64, device=dev),
              trial_energy=torch.empty(S, n_iter, dtype=torch.float64, device=dev),
              step=torch.empty(S, n_iter, dtype=torch.float32, device=dev),
              accepted=torch.empty(S, n_iter, dtype=torch.uint8, device=dev),
              gmax=torch.empty(S, n_iter, dtype=torch.float32, device=dev),
              converged=torch.empty(S, dtype=torch.uint8, device=dev))
    scratch = _relax_scratch(S, t, n_iter, dev)
    p = _lib.ptr
    opt = lambda a: p(a) if a.numel() else None                                                               # noqa: E731
    rc = _lib.lib().codlad_relax(p(x), S, n, p(t["radius"]), p(fx), *_relax_table_args(t),
                                 *_relax_constants(constants, ("k_r", "k_t", "k_c", "contact_scale", "h0", "h_max")), n_iter,
                                 p(out), p(tr["energy"]), opt(tr["trial_energy"]), opt(tr["step"]), opt(tr["accepted"]),
                                 opt(tr["gmax"]), p(tr["converged"]), p(scratch), _lib.stream_ptr(dev))
    _lib.check(rc, "codlad_relax")
    return dict(tr, xyz=out, n_accepted=tr["accepted"].sum(1, dtype=torch.int32), energy0=tr["energy"][:, 0],
                trace_energy=tr["energy"], energy=tr["energy"][:, -1])


def relax_energy(xyz, top, xyz0=None, fixed=None, order=2, **constants):
    """One evaluation of the relaxation energy of xyz [S, n_atoms, 3] (device) against the start structure xyz0 (default:
    xyz itself, which makes the two restraint terms 0) -> dict of device tensors: energy float64 [S, 3] in the order of
    RELAX_ENERGIES, total float64 [S], grad float32 [S, n_atoms, 3] (0 on fixed atoms), gmax float32 [S].  Constants:
    k_r, k_t, k_c, contact_scale (RELAX_DEFAULTS).  The evaluation `relax` runs, bit for bit."""
    _need_cuda(xyz, "xyz")
    _need_cuda(xyz0, "xyz0")
    if xyz.dim() == 3 and xyz.shape[1] != top.n_atoms:
        raise ValueError(f"relax_energy: xyz has {xyz.shape[1]} atoms, the topology {top.n_atoms}")
    return _relax_energy_launch(xyz, xyz0, _relax_tables_on(top, order, xyz.device),
                                relax_tables(top, order)["fixed"] if fixed is None else fixed, constants)


def relax(xyz, top, n_iter=200, fixed=None, order=2, **constants):
    """Restrained clash relaxation of xyz [S, n_atoms, 3] (device), S structures of the topology `top`: exactly n_iter
    steepest-descent iterations per structure (accept a trial that lowers the energy and lengthen the step by 1.2, else
    halve it), each structure on its own, no host transfer.  The energy holds every distance within two bonds and every
    torsion about a rigid bond to the INPUT's and repels atoms more than `order` bonds apart that are closer than
    (r_i + r_j) * contact_scale; atoms of `fixed` (bool [n_atoms], default: the CAs) return bit for bit.  -> dict:
      xyz float32 [S, n_atoms, 3]; trace_energy float64 [S, n_iter + 1] (accepted state, column 0 = input), trial_energy
      float64, step, gmax float32, accepted uint8 [S, n_iter]; converged uint8 [S] (nothing pushes any more);
      n_accepted int32 [S]; energy0, energy float64 [S]: the total before and after.
    Constants: k_r, k_t, k_c, contact_scale, h0, h_max (RELAX_DEFAULTS).  What is wrong in the input - a broken ring, an
    inverted centre - is preserved: the restraints come from it."""
    _need_cuda(xyz, "xyz")
    if xyz.dim() == 3 and xyz.shape[1] != top.n_atoms:
        raise ValueError(f"relax: xyz has {xyz.shape[1]} atoms, the topology {top.n_atoms}")
    return _relax_launch(xyz, _relax_tables_on(top, order, xyz.device),
                         relax_tables(top, order)["fixed"] if fixed is None else fixed, n_iter, constants)


def relax_lists(xyz, radius, bonds, quads, fixed=None, n_iter=200, order=2, **constants):
    """relax for a topology given as lists: radius [n_atoms], bonds [n_bonds, 2] (each once, i < j), quads [Q, 4] (the
    restrained torsions), fixed bool [n_atoms] (default: none).  The tables are rebuilt on every call."""
    _need_cuda(xyz, "xyz")
    t = _relax_lists_tables(radius, bonds, quads, order, xyz.device)
    return _relax_launch(xyz, t, torch.zeros(t["radius"].shape[0], dtype=torch.bool) if fixed is None else fixed, n_iter, constants)


def relax_energy_lists(xyz, radius, bonds, quads, xyz0=None, fixed=None, order=2, **constants):
    """relax_energy for a topology given as lists (see relax_lists)."""
    _need_cuda(xyz, "xyz")
    _need_cuda(xyz0, "xyz0")
    t = _relax_lists_tables(radius, bonds, quads, order, xyz.device)
    return _relax_energy_launch(xyz, xyz0, t, torch.zeros(t["radius"].shape[0], dtype=torch.bool) if fixed is None else fixed,
                                constants)


# --- Ensemble observables (codlad_sasa, codlad_contact_counts, csrc/observables_kernels.hip; the radius of gyration from
# codlad_ens_moments): what describes a disordered-protein ensemble once its members have been judged one by one.

VDW_RADII = {"C": 1.70, "N": 1.55, "O": 1.52, "S": 1.80, "P": 1.80, "H": 1.20}       # Bondi (1964), A
SASA_MAX_POINTS = _lib.SASA_MAX_POINTS
_SPHERE_POINTS = {}


def vdw_radii(elements):
    """float64 numpy [n]: VDW_RADII of every element symbol (any case); an element not in the table raises ValueError."""
    import numpy as np
    elements = [str(e).strip().upper() for e in elements]
    unknown = sorted(set(elements) - set(VDW_RADII))
    if unknown:
        raise ValueError(f"no van der Waals radius for element(s) {unknown} (known: {', '.join(VDW_RADII)})")
    return np.array([VDW_RADII[e] for e in elements], dtype=np.float64)


def sphere_points(n):
    """float32 tensor [n, 3] (host): the golden spiral on the unit sphere, computed in float64 and rounded once -
    z_k = 1 - (2 k + 1) / n, phi_k = k pi (3 - sqrt 5), (sqrt(1 - z^2) cos phi, sqrt(1 - z^2) sin phi, z)."""
    import numpy as np
    n = int(n)
    if not 1 <= n <= SASA_MAX_POINTS:
        raise ValueError(f"sasa: n_points must be in 1 .. {SASA_MAX_POINTS}, got {n}")
    if n not in _SPHERE_POINTS:
        k = np.arange(n, dtype=np.float64)
        z = 1.0 - (2.0 * k + 1.0) / n
        phi = k * (np.pi * (3.0 - np.sqrt(5.0)))
        rho = np.sqrt(1.0 - z * z)
        _SPHERE_POINTS[n] = torch.from_numpy(np.stack([rho * np.cos(phi), rho * np.sin(phi), z], 1).astype(np.float32))
    return _SPHERE_POINTS[n]


def _sasa_atom_tables(radii, probe, n_points, dev):
    """(radius, unit_area, dirs) on `dev`: radius = fl32(vdW + probe), unit_area = fl32(4 pi R^2 / n_points) with R that
    fp32 radius and the quotient in float64."""
    import numpy as np
    radii = np.asarray(radii.detach().cpu().numpy() if torch.is_tensor(radii) else radii, dtype=np.float64).reshape(-1)
    if not (np.isfinite(radii).all() and (radii > 0).all()) or not float(probe) >= 0:
        raise ValueError("sasa: radii must be positive and the probe non-negative")
    dirs = sphere_points(n_points)
    radius = (radii + float(probe)).astype(np.float32)
    unit = (4.0 * np.pi * radius.astype(np.float64) ** 2 / int(n_points)).astype(np.float32)
    return torch.from_numpy(radius).to(dev), torch.from_numpy(unit).to(dev), dirs.to(dev).contiguous()


def _res_table(res_ptr, n_atoms):
    """res_ptr (or None) -> the HOST int32 table codlad_sasa reads, or None."""
    import numpy as np
    if res_ptr is None:
        return None
    tab = np.ascontiguousarray(np.asarray(res_ptr).reshape(-1), dtype=np.int32)
    if tab.shape[0] < 2:
        raise ValueError("sasa: res_ptr needs two entries or more (the atoms of residue r are res_ptr[r] .. res_ptr[r + 1] - 1)")
    if tab[0] < 0 or (np.diff(tab) < 0).any() or tab[-1] > n_atoms:
        raise ValueError(f"sasa: res_ptr must be non-decreasing within [0, {n_atoms}]")
    return tab


def _sasa_launch(xyz, radius, unit_area, dirs, res_tab):
    _need_cuda(xyz, "xyz")
    if xyz.dim() != 3 or xyz.shape[-1] != 3 or xyz.shape[0] == 0 or xyz.shape[1] == 0:
        raise ValueError(f"sasa: xyz must be a non-empty [S, n_atoms, 3] tensor, got {tuple(xyz.shape)}")
    if xyz.shape[1] != radius.shape[0]:
        raise ValueError(f"sasa: xyz has {xyz.shape[1]} atoms, the topology {radius.shape[0]}")
    dev = xyz.device
    x = xyz.detach().to(torch.float32).contiguous()
    S, n = x.shape[0], x.shape[1]
    R = 0 if res_tab is None else res_tab.shape[0] - 1
    exposed = torch.empty(S, n, dtype=torch.int32, device=dev)
    atom = torch.empty(S, n, dtype=torch.float32, device=dev)
    residue = torch.empty(S, R, dtype=torch.float32, device=dev) if R else None
    total = torch.empty(S, dtype=torch.float64, device=dev)
    finite = torch.empty(S, dtype=torch.uint8, device=dev)
    p = _lib.ptr
    rc = _lib.lib().codlad_sasa(p(x), S, n, p(radius), p(unit_area), p(dirs), dirs.shape[0],
                                res_tab.ctypes.data_as(C.c_void_p) if R else None, R, p(exposed), p(atom), p(residue), p(total),
                                p(finite), _lib.stream_ptr(dev))
    _lib.check(rc, "codlad_sasa")
    return dict(atom=atom, residue=residue, total=total, exposed=exposed, finite=finite.to(torch.bool))


def sasa_lists(xyz, radii, res_ptr=None, probe=1.4, n_points=960):
    """sasa for atoms given as lists: radii [n_atoms] (van der Waals, without the probe), res_ptr [R + 1] (the atoms of
    residue r are res_ptr[r] .. res_ptr[r + 1] - 1; None: no residues, `residue` is None).  The tables are rebuilt on every
    call: for repeated calls on a protein use sasa."""
    _need_cuda(xyz, "xyz")
    n = xyz.shape[1] if xyz.dim() == 3 else 0
    return _sasa_launch(xyz, *_sasa_atom_tables(radii, probe, n_points, xyz.device), _res_table(res_ptr, n))


def sasa(xyz, top, probe=1.4, n_points=960, radii=None):
    """Solvent-accessible surface area (Shrake-Rupley) of xyz [S, n_atoms, 3] (device), S structures of the topology `top`
    -> dict of device tensors:
      atom float32 [S, n_atoms]      A^2 per atom: exposed * 4 pi R^2 / n_points, R = van der Waals radius + probe
      residue float32 [S, R]         the atoms of each residue (top.first_atom) summed in float64, rounded once
      total float64 [S]              all atoms
      exposed int32 [S, n_atoms]     the test points of the atom that no other atom's sphere contains, of n_points
      finite bool [S]                False: a coordinate of the structure is NaN or +-inf - its exposed are -1, its areas NaN
    radii: van der Waals radii [n_atoms] in place of VDW_RADII of top.element (Bondi; heavy atoms, no hydrogens are added).
    The points are sphere_points(n_points).  Three launches, no host transfer; integer decisions and sums in one order, so
    the bits repeat from call to call and a structure's results do not depend on the others of the call."""
    _need_cuda(xyz, "xyz")
    if xyz.dim() == 3 and xyz.shape[1] != top.n_atoms:
        raise ValueError(f"sasa: xyz has {xyz.shape[1]} atoms, the topology {top.n_atoms}")
    if radii is not None:
        return _sasa_launch(xyz, *_sasa_atom_tables(radii, probe, n_points, xyz.device), _res_table(top.first_atom, top.n_atoms))
    cache = top.__dict__.setdefault("_sasa_tables", {})
    key = (float(probe), int(n_points), str(xyz.device))
    if key not in cache:
        cache[key] = _sasa_atom_tables(vdw_radii(top.element), probe, n_points, xyz.device) + \
            (_res_table(top.first_atom, top.n_atoms),)
    return _sasa_launch(xyz, *cache[key])


def radius_of_gyration(xyz, sel=None):
    """xyz [S, n_atoms, 3] (device) -> float64 [S] on the device: sqrt(sum |x - c|^2 / m) about the unweighted centroid c
    of the atoms `sel` (default: all), m their number - G of codlad_ens_moments, no kernel of its own.  NaN for a structure
    with a coordinate that is not a number."""
    x = _coords(xyz, "radius_of_gyration: xyz", 3)
    sel, n_sel = _selection(sel, x.shape[1], x.device)
    mom = _moments(x, x.shape[0], x.shape[1], sel, n_sel)
    return torch.sqrt(mom[:, 3] / float(n_sel or x.shape[1]))


def contact_map(xyz, sel=None, cutoff=8.0):
    """xyz [S, n_atoms, 3] (device) -> dict: counts int32 [m, m] (device), the number of structures in which atoms
    sel[a] and sel[b] (default: all atoms, m = n_atoms) are closer than `cutoff` (d^2 < fl32(cutoff^2) in fp32); frequency
    float64 [m, m] = counts / S; n_struct = S.  Symmetric, diagonal 0; a distance that is not a number is no contact."""
    x = _coords(xyz, "contact_map: xyz", 3)
    if not float(cutoff) >= 0:
        raise ValueError(f"contact_map: cutoff must be >= 0, got {cutoff}")
    S, n = x.shape[0], x.shape[1]
    sel, n_sel = _selection(sel, n, x.device)
    m = n_sel or n
    counts = torch.empty(m, m, dtype=torch.int32, device=x.device)
    rc = _lib.lib().codlad_contact_counts(_lib.ptr(x), S, n, _lib.ptr(sel), n_sel, C.c_float(float(cutoff) ** 2),
                                          _lib.ptr(counts), _lib.stream_ptr(x.device))
    _lib.check(rc, "codlad_contact_counts")
    # a tensor divisor: the correctly rounded quotient (a Python scalar would be turned into a multiplication by 1 / S)
    return dict(counts=counts, frequency=counts.to(torch.float64) / torch.tensor(float(S), dtype=torch.float64, device=x.device),
                n_struct=S)


# --- Secondary structure (codlad_dssp_hbonds, codlad_dssp_assign, csrc/dssp_kernels.hip): the Kabsch-Sander hydrogen
# bonds of every structure as bitmaps, the DSSP states read off them, and their propensity over the ensemble.

DSSP_CODES = _lib.DSSP_CODES                     # " HBEGITS": the letter of code 0 .. 7; 255 (undefined) prints as '?'
DSSP_NAMES = ("loop", "H", "B", "E", "G", "I", "T", "S")
DSSP_MAX_RES = _lib.DSSP_MAX_RES


def dssp_tables(top):
    """(bb int32 [n_res, 4], res_kind uint8 [n_res]) of a dataset_builder.Topology, on the host: the atom indices of N, CA,
    C, O of every residue by atom name (-1: the residue lists none) and, per residue, bit 0 = PRO (no amide H), bit 1 = the
    residue starts a chain (residue 0, or chain_ids differs from the previous residue's: stereo_tables' neighbour rule).
    Built once and kept on the topology object."""
    cache = top.__dict__.setdefault("_dssp_tables", {})
    if "host" not in cache:
        n_res = top.n_residues
        bb = torch.tensor([[top.atom(r, a) for a in ("N", "CA", "C", "O")] for r in range(n_res)],
                          dtype=torch.int32).reshape(n_res, 4)
        kind = torch.tensor([(_lib.DSSP_KIND_PRO if top.res_names[r] == "PRO" else 0) |
                             (_lib.DSSP_KIND_CHAIN_START if r == 0 or top.chain_ids[r - 1] != top.chain_ids[r] else 0)
                             for r in range(n_res)], dtype=torch.uint8)
        cache["host"] = (bb, kind)
    return cache["host"]


def _dssp_inputs(xyz, top, what):
    _need_cuda(xyz, "xyz")
    if xyz.dim() != 3 or xyz.shape[-1] != 3 or xyz.shape[0] == 0:
        raise ValueError(f"{what}: xyz must be a non-empty [S, n_atoms, 3] tensor, got {tuple(xyz.shape)}")
    if xyz.shape[1] != top.n_atoms:
        raise ValueError(f"{what}: xyz has {xyz.shape[1]} atoms, the topology {top.n_atoms}")
    if not 1 <= top.n_residues <= DSSP_MAX_RES:
        raise ValueError(f"{what}: the topology has {top.n_residues} residues, the kernels take 1 .. {DSSP_MAX_RES}")
    dev = xyz.device
    cache = top.__dict__.setdefault("_dssp_tables", {})
    if str(dev) not in cache:
        cache[str(dev)] = tuple(t.to(dev).contiguous() for t in dssp_tables(top))
    return xyz.detach().to(torch.float32).contiguous(), cache[str(dev)]


def hbonds(xyz, top):
    """Backbone hydrogen bonds of xyz [S, n_atoms, 3] (device), S structures of the topology `top` -> dict of device tensors
    (R = top.n_residues, W = ceil(R / 64); the rule is in include/codlad_hip.h):
      acc int64 [S, R, W]       bit j of row i (bit j % 64 of word j // 64): Hbond(i -> j), the C=O of i accepts the N-H of j
                                (E < -0.5 kcal/mol, Kabsch-Sander); the words are uint64 bit patterns held in int64
      don int64 [S, R, W]       bit j of row i: Hbond(j -> i); the transpose of acc
      geom uint8 [S, R]         bit 0: the link r -> r+1 is intact (same chain, C and N within 2.5 A); bit 1: bend (kappa > 70)
      kappa float32 [S, R]      the CA bend angle in degrees, NaN where undefined
      e_best float32 [S, R, 2], partner int32 [S, R, 2]
                                the lowest energy of the residue as acceptor ([..., 0]) and as donor ([..., 1]) and the partner
                                (ties: the lowest index); -1 and 0 where no pair is eligible
      finite bool [S]           False: a backbone coordinate is NaN or +-inf - bitmaps and geom 0, energies and kappa NaN,
                                partners -1
    Two launches, no host transfer; results are bit-identical from call to call and independent of the batch."""
    x, (bb, kind) = _dssp_inputs(xyz, top, "hbonds")
    return _hbonds_launch(x, bb, kind)[0]


def _hbonds_launch(x, bb, kind):
    dev = x.device
    S, R = x.shape[0], bb.shape[0]
    W = (R + 63) // 64
    acc = torch.empty(S, R, W, dtype=torch.int64, device=dev)
    don = torch.empty(S, R, W, dtype=torch.int64, device=dev)
    geom = torch.empty(S, R, dtype=torch.uint8, device=dev)
    kappa = torch.empty(S, R, dtype=torch.float32, device=dev)
    e_best = torch.empty(S, R, 2, dtype=torch.float32, device=dev)
    partner = torch.empty(S, R, 2, dtype=torch.int32, device=dev)
    finite = torch.empty(S, dtype=torch.uint8, device=dev)
    p = _lib.ptr
    rc = _lib.lib().codlad_dssp_hbonds(p(x), S, x.shape[1], p(bb), p(kind), R, p(acc), p(don), p(geom), p(kappa), p(e_best),
                                       p(partner), p(finite), _lib.stream_ptr(dev))
    _lib.check(rc, "codlad_dssp_hbonds")
    return dict(acc=acc, don=don, geom=geom, kappa=kappa, e_best=e_best, partner=partner, finite=finite.to(torch.bool)), finite


def dssp_assign(acc, don, geom, finite):
    """The pattern stage alone, on bitmaps in hbonds' layout (device; they need not come from hbonds) -> dict: ss uint8
    [S, R], bridge int32 [S, R, 2], counts int32 [S, 8]."""
    for t, what in ((acc, "acc"), (don, "don"), (geom, "geom"), (finite, "finite")):
        _need_cuda(t, what)
    S, R = geom.shape
    W = (R + 63) // 64
    if tuple(acc.shape) != (S, R, W) or tuple(don.shape) != (S, R, W) or tuple(finite.shape) != (S,) or S == 0 or R == 0:
        raise ValueError(f"dssp_assign: acc / don must be [S, R, ceil(R / 64)], geom [S, R], finite [S]; got "
                         f"{tuple(acc.shape)}, {tuple(don.shape)}, {tuple(geom.shape)}, {tuple(finite.shape)}")
    if acc.dtype != torch.int64 or don.dtype != torch.int64 or geom.dtype != torch.uint8:
        raise ValueError("dssp_assign: acc / don are int64 words, geom uint8")
    if R > DSSP_MAX_RES:
        raise ValueError(f"dssp_assign: {R} residues, the kernel takes 1 .. {DSSP_MAX_RES}")
    dev = geom.device
    fin = finite.to(torch.uint8).contiguous()
    ss = torch.empty(S, R, dtype=torch.uint8, device=dev)
    bridge = torch.empty(S, R, 2, dtype=torch.int32, device=dev)
    counts = torch.empty(S, 8, dtype=torch.int32, device=dev)
    p = _lib.ptr
    rc = _lib.lib().codlad_dssp_assign(p(acc.contiguous()), p(don.contiguous()), p(geom.contiguous()), p(fin), S, R, p(ss),
                                       p(bridge), p(counts), _lib.stream_ptr(dev))
    _lib.check(rc, "codlad_dssp_assign")
    return dict(ss=ss, bridge=bridge, counts=counts)


def ss_strings(ss):
    """ss uint8 [S, R] (any device) -> a list of S strings over DSSP_CODES, '?' for an undefined residue (one host copy)."""
    table = DSSP_CODES + "?" * (256 - len(DSSP_CODES))
    return ["".join(table[c] for c in row) for row in ss.detach().cpu().tolist()]


class _DsspResult(dict):
    """metrics.dssp's dict; `ss_string` is built (and the labels copied to the host) when it is first asked for."""

    def __missing__(self, key):
        if key != "ss_string":
            raise KeyError(key)
        self[key] = ss_strings(self["ss"])
        return self[key]


def dssp(xyz, top):
    """Secondary structure (DSSP: Kabsch & Sander 1983, classic priority H > B / E > G > I > T > S) of xyz [S, n_atoms, 3]
    (device), S structures of the topology `top` -> dict of device tensors:
      ss uint8 [S, R]             0 .. 7 = ' ', H, B, E, G, I, T, S (DSSP_CODES); 255 in a structure that is not finite
      ss_string                   a list of S strings over " HBEGITS", '?' for undefined; built on request only (out["ss_string"])
      bridge int32 [S, R, 2]      the lowest parallel and the lowest antiparallel bridge partner, -1 where there is none
      counts int32 [S, 8]         residues per code (-1: not finite), each also under its name: loop, H, B, E, G, I, T, S
      finite bool [S]
      acc, don, geom, kappa, e_best, partner: the first stage's tensors (hbonds)
    Three launches, no host transfer.  Differences from mkdssp: the full hydrogen-bond matrix is used (no truncation to a
    residue's two best partners), energies are not rounded to 0.001, there are no beta bulges and no sheet labels."""
    x, (bb, kind) = _dssp_inputs(xyz, top, "dssp")
    hb, finite = _hbonds_launch(x, bb, kind)
    out = _DsspResult(hb)
    out.update(dssp_assign(hb["acc"], hb["don"], hb["geom"], finite))
    out.update({k: out["counts"][:, c] for c, k in enumerate(DSSP_NAMES)})
    return out


def ss_propensity(ss):
    """ss uint8 [S, R] (device) -> float64 [R, 8] on the device: the share of the FINITE structures (those not labelled 255)
    that carry each code at each residue; NaN when no structure is finite."""
    _need_cuda(ss, "ss")
    if ss.dim() != 2 or ss.numel() == 0:
        raise ValueError(f"ss_propensity: ss must be a non-empty [S, R] tensor, got {tuple(ss.shape)}")
    codes = torch.arange(8, device=ss.device, dtype=ss.dtype)
    count = (ss[:, :, None] == codes).sum(dim=0).to(torch.float64)
    n_finite = (ss[:, 0] != _lib.DSSP_UNDEFINED).sum().to(torch.float64)
    # a tensor divisor: the correctly rounded quotient (a Python scalar would be turned into a multiplication by 1 / n)
    return count / n_finite
