"""Reference-free geometry check (codlad_geometry_check, csrc/geometry_kernels.hip): generated structures judged against
the template topology they were built from, with no true coordinates (broken / spurious covalent bonds, clashes; one
all-pairs launch)."""
import ctypes as C

import torch

from .. import _lib
from . import _inputs

GEOMETRY_COUNTS = ("broken", "spurious", "bonded", "near", "clash")


def _geometry_launch(x, radius, ptr_, words, bonds, scale, clash_dist, near_dist):
    dev = x.device
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
    x, radius, bonds = _inputs.list_inputs(xyz, "geometry_check", radius, bonds)
    dev = x.device
    ptr_, words = _inputs.exclusion_csr(bonds, order, radius.shape[0])
    return _geometry_launch(x, radius.to(dev).contiguous(), ptr_.to(dev), words.to(dev),
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
    x = _inputs.structures(xyz, "geometry_check: xyz", top.n_atoms)
    if order < 1:
        raise ValueError(f"geometry_check: order must be >= 1, got {order}")
    # (radius, excl_ptr, excl, bonds): the template's uploads, the very tensors the relaxation reads
    tables = _inputs.cached(top, "_geometry_tables", (int(order), str(x.device)), lambda: _inputs.template_tables(top, order, x.device))
    return _geometry_launch(x, *tables, scale, clash_dist, near_dist)
