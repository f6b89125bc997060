"""What the structure-analysis entry points share: the check of a structure batch, of a pool with its atom selection and
weights, of a positive number and a count, the flag and scratch buffers of a call, the per-topology cache, and the
tables of a template (covalent radii, exclusion CSR, bond list) that the geometry check and the relaxation both read."""
import math

import torch

from .. import _lib

# Covalent cut-off radii by atomic number 1..107 (the reference's COVCUTOFFTABLE, utils/protein_module.py:128-234: a
# table of constants, kept as data)
COV_CUTOFF = (0.23, 0.93, 0.68, 0.35, 0.83, 0.68, 0.68, 0.68, 0.64, 1.12, 0.97, 1.1, 1.35, 1.2, 0.75, 1.02, 0.99, 1.57,
              1.33, 0.99, 1.44, 1.47, 1.33, 1.35, 1.35, 1.34, 1.33, 1.5, 1.52, 1.45, 1.22, 1.17, 1.21, 1.22, 1.21, 1.91,
              1.47, 1.12, 1.78, 1.56, 1.48, 1.47, 1.35, 1.4, 1.45, 1.5, 1.59, 1.69, 1.63, 1.46, 1.46, 1.47, 1.4, 1.98,
              1.67, 1.34, 1.87, 1.83, 1.82, 1.81, 1.8, 1.8, 1.99, 1.79, 1.76, 1.75, 1.74, 1.73, 1.72, 1.94, 1.72, 1.57,
              1.43, 1.37, 1.35, 1.37, 1.32, 1.5, 1.5, 1.7, 1.55, 1.54, 1.54, 1.68, 1.7, 2.4, 2.0, 1.9, 1.88, 1.79, 1.61,
              1.58, 1.55, 1.53, 1.51, 1.5, 1.5, 1.5, 1.5, 1.5, 1.5, 1.5, 1.5, 1.57, 1.49, 1.43, 1.41)


def need_cuda(t, what):
    if t is not None and not t.is_cuda:
        raise RuntimeError(f"{what} must be a CUDA tensor: the metrics run on the MI355X only")


def structures(xyz, what, n_atoms=None, dims=3):
    """The one check of a batch of structures -> its contiguous fp32 copy.  RuntimeError for a CPU tensor; ValueError
    unless xyz is a non-empty [..., n_atoms, 3] tensor of `dims` axes whose atom count is n_atoms.  Empty: no structure
    where the atom count is held to a topology's, no element at all where there is none to hold it to (n_atoms None)."""
    need_cuda(xyz, what)
    if xyz.dim() != dims or xyz.shape[-1] != 3 or (xyz.numel() if n_atoms is None else xyz.shape[0]) == 0:
        raise ValueError(f"{what} must be a non-empty [{', '.join(('G', 'S', 'n_atoms', '3')[-dims:])}] tensor, got {tuple(xyz.shape)}")
    if n_atoms is not None and xyz.shape[-2] != n_atoms:
        raise ValueError(f"{what} has {xyz.shape[-2]} atoms, the topology {n_atoms}")
    return xyz.detach().to(torch.float32).contiguous()


def selection(sel, n_atoms, dev):
    """sel (index list / tensor, or None) -> (int32 device tensor or None, count for the C ABI)."""
    if sel is None:
        return None, 0
    idx = torch.as_tensor(sel).reshape(-1).to(torch.int64)
    if idx.numel() == 0:
        raise ValueError("sel is empty")
    if int(idx.min()) < 0 or int(idx.max()) >= n_atoms:
        raise ValueError(f"sel has an index outside [0, {n_atoms})")
    return idx.to(device=dev, dtype=torch.int32).contiguous(), idx.numel()


def pool(x, sel, what, max_n):
    """One pool of structures x [N, n, 3] and its atom selection -> (the checked structures, sel on the device, n_sel).  A
    CPU tensor is refused first, then a pool of more than max_n structures, then the selection."""
    x = structures(x, f"{what}: x")
    if x.shape[0] > max_n:
        raise ValueError(f"{what}: at most {max_n} structures in one pool, got {x.shape[0]}")
    sel, n_sel = selection(sel, x.shape[1], x.device)
    return x, sel, n_sel


def weights(weights, N, dev, what, need_positive):
    """Per-structure weights -> float64 [N] on dev; ValueError unless there are N of them, finite and >= 0.  With
    need_positive, None stays None (no weights) and one weight at least must be > 0."""
    if need_positive and weights is None:
        return None
    w = torch.as_tensor(weights).detach().to(torch.float64).reshape(-1)
    if w.shape[0] != N:
        raise ValueError(f"{what}: weights must have one value per structure ({N}), got {w.shape[0]}")
    if not bool(torch.isfinite(w).all()) or bool((w < 0).any()):
        raise ValueError(f"{what}: weights must be finite and >= 0")
    if need_positive and not bool((w > 0).any()):
        raise ValueError(f"{what}: every weight is 0")
    return w.to(dev).contiguous()


def positive(v, name, what):
    """v as a float; ValueError unless it is a positive finite number (a bool counts as the number it is)."""
    try:
        f = float(v)
    except (TypeError, ValueError):
        f = math.nan
    if not (math.isfinite(f) and f > 0):
        raise ValueError(f"{what}: {name} must be a positive finite number, got {v!r}")
    return f


def count(v, name, hi, what, types=(int,)):
    """v as an int; ValueError unless it is one of `types` (never a bool) in 1 .. hi."""
    if isinstance(v, bool) or not isinstance(v, types) or not 1 <= v <= hi:
        raise ValueError(f"{what}: {name} must be an integer in 1 .. {hi}, got {v!r}")
    return int(v)


def flags(N, dev):
    """An uninitialised uint8 [N] on dev for per-structure flags a kernel writes.  The allocation holds two elements or
    more: tests/memcheck.py cannot tell a one-element integer buffer from its poison."""
    return torch.empty(max(N, 2), dtype=torch.uint8, device=dev)[:N]


def scratch(fn_name, *args, dev, dtype=torch.float64):
    """The scratch tensor (float64 words; int64 where a kernel keeps integers there) of the size
    codlad_..._scratch_bytes(*args) asks for, rounded up to whole words; a negative size raises what _lib.check makes of
    the library's last error, under the function's name."""
    nbytes = getattr(_lib.lib(), fn_name)(*args)
    if nbytes < 0:
        _lib.check(-1, fn_name)
    return torch.empty((nbytes + 7) // 8, dtype=dtype, device=dev)


def cached(top, name, key, build):
    """build() once per (topology, name, key), kept ON the topology object as top.<name>[key]: its lifetime, no key that
    a reused address could alias.  Host tables and their per-device copies are entries of the same dict."""
    cache = top.__dict__.setdefault(name, {})
    if key not in cache:
        cache[key] = build()
    return cache[key]


def cov_radius(atomic_nums):
    """float32 [n] (host): COV_CUTOFF of every atomic number; one outside the table raises ValueError."""
    z = torch.as_tensor(atomic_nums).to(torch.int64).cpu()
    if z.numel() and (int(z.min()) < 1 or int(z.max()) > len(COV_CUTOFF)):
        raise ValueError("atomic number outside the covalent cut-off table (1..107)")
    return torch.tensor(COV_CUTOFF, dtype=torch.float32)[z - 1].contiguous()


def list_inputs(xyz, what, radius, bonds):
    """The arguments every *_lists entry point takes -> (the checked structures, radius float32 [n_atoms], bonds int64
    [n_bonds, 2], both on the host); ValueError unless every bond is a pair i < j."""
    radius = torch.as_tensor(radius).detach().to(torch.float32).reshape(-1)
    x = structures(xyz, f"{what}: xyz", radius.shape[0])
    bonds = torch.as_tensor(bonds).reshape(-1, 2).to(torch.int64).cpu()
    if bonds.numel() and not bool((bonds[:, 0] < bonds[:, 1]).all()):
        raise ValueError(f"{what}: bonds must be pairs i < j")
    return x, radius, bonds


def adjacency(bonds, n_atoms):
    """The neighbour set of every atom of a bond list (any order, repeats allowed; indices are not checked here)."""
    adj = [set() for _ in range(n_atoms)]
    for i, j in torch.as_tensor(bonds).reshape(-1, 2).tolist():
        adj[i].add(j)
        adj[j].add(i)
    return adj


def exclusion_csr(bonds, order, n_atoms):
    """The pairs within `order` bonds (dataset_builder.high_order_edges' pair set) as the CSR codlad_geometry_check reads:
    (ptr int32 [n_atoms + 1], partners int32) - row i lists, sorted, every j != i within `order` bonds of i (so the list
    is symmetric), with _lib.GEOM_BOND_FLAG set on the bonded (order-1) ones.  Walks adjacency lists: no n x n matrix."""
    for i, j in torch.as_tensor(bonds).reshape(-1, 2).tolist():
        if not (0 <= i < n_atoms and 0 <= j < n_atoms) or i == j:
            raise ValueError(f"bond ({i}, {j}) is not a pair of different atoms of [0, {n_atoms})")
    adj = adjacency(bonds, n_atoms)
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


def template_tables(top, order, dev=None):
    """(radius, excl_ptr, excl, bonds) of a template topology, the tables more than one stage reads: cov_radius of its atoms,
    exclusion_csr of standard_bonds(top) at `order`, and those bonds - on the host (bonds int64), or on `dev` (bonds int32).
    Each is built once per topology and uploaded once per device (top._template_tables), whatever orders are asked for."""
    from ..utils.dataset_builder import standard_bonds

    def table(key, build, upload=lambda t: t.to(dev)):
        host = cached(top, "_template_tables", key, build)
        return host if dev is None else cached(top, "_template_tables", (key, str(dev)), lambda: upload(host))
    bonds = cached(top, "_template_tables", "bonds", lambda: standard_bonds(top))
    ptr, words = table(("excl", int(order)), lambda: exclusion_csr(bonds, order, top.n_atoms), lambda pw: tuple(t.to(dev) for t in pw))
    return (table("radius", lambda: cov_radius(top.atomic_nums())), ptr, words,
            table("bonds", lambda: bonds, lambda t: t.to(torch.int32).to(dev).contiguous()))
