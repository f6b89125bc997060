"""Ensemble observables (codlad_sasa, codlad_contact_counts, csrc/observables_kernels.hip; the radius of gyration from
codlad_ens_moments): what describes a disordered-protein ensemble once its members have been judged one by one."""
import ctypes as C

import numpy as np
import torch

from .. import _lib
from . import _inputs
from .ensemble import _moments

VDW_RADII = {"C": 1.70, "N": 1.55, "O": 1.52, "S": 1.80, "P": 1.80, "H": 1.20}       # Bondi (1964), A
SASA_MAX_POINTS = _lib.SASA_MAX_POINTS
_SPHERE_POINTS = {}


def vdw_radii(elements):
    """float64 numpy [n]: VDW_RADII of every element symbol (any case); an element not in the table raises ValueError."""
    elements = [str(e).strip().upper() for e in elements]
    unknown = sorted(set(elements) - set(VDW_RADII))
    if unknown:
        raise ValueError(f"no van der Waals radius for element(s) {unknown} (known: {', '.join(VDW_RADII)})")
    return np.array([VDW_RADII[e] for e in elements], dtype=np.float64)


def sphere_points(n):
    """float32 tensor [n, 3] (host): the golden spiral on the unit sphere, computed in float64 and rounded once -
    z_k = 1 - (2 k + 1) / n, phi_k = k pi (3 - sqrt 5), (sqrt(1 - z^2) cos phi, sqrt(1 - z^2) sin phi, z)."""
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
    radii = np.asarray(radii.detach().cpu().numpy() if torch.is_tensor(radii) else radii, dtype=np.float64).reshape(-1)
    if not (np.isfinite(radii).all() and (radii > 0).all()) or not float(probe) >= 0:
        raise ValueError("sasa: radii must be positive and the probe non-negative")
    dirs = sphere_points(n_points)
    radius = (radii + float(probe)).astype(np.float32)
    unit = (4.0 * np.pi * radius.astype(np.float64) ** 2 / int(n_points)).astype(np.float32)
    return torch.from_numpy(radius).to(dev), torch.from_numpy(unit).to(dev), dirs.to(dev).contiguous()


def _res_table(res_ptr, n_atoms):
    """res_ptr (or None) -> the HOST int32 table codlad_sasa reads, or None."""
    if res_ptr is None:
        return None
    tab = np.ascontiguousarray(np.asarray(res_ptr).reshape(-1), dtype=np.int32)
    if tab.shape[0] < 2:
        raise ValueError("sasa: res_ptr needs two entries or more (the atoms of residue r are res_ptr[r] .. res_ptr[r + 1] - 1)")
    if tab[0] < 0 or (np.diff(tab) < 0).any() or tab[-1] > n_atoms:
        raise ValueError(f"sasa: res_ptr must be non-decreasing within [0, {n_atoms}]")
    return tab


def _sasa_launch(xyz, radius, unit_area, dirs, res_tab):
    x = _inputs.structures(xyz, "sasa: xyz", radius.shape[0])
    if x.shape[1] == 0:                                   # an empty atom list matches its count: sasa takes none
        raise ValueError(f"sasa: xyz must be a non-empty [S, n_atoms, 3] tensor, got {tuple(x.shape)}")
    dev = x.device
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
    _inputs.need_cuda(xyz, "sasa: xyz")
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
    _inputs.need_cuda(xyz, "sasa: xyz")
    if radii is not None:
        return _sasa_launch(xyz, *_sasa_atom_tables(radii, probe, n_points, xyz.device), _res_table(top.first_atom, top.n_atoms))
    return _sasa_launch(xyz, *_inputs.cached(top, "_sasa_tables", (float(probe), int(n_points), str(xyz.device)), lambda: (
        *_sasa_atom_tables(vdw_radii(top.element), probe, n_points, xyz.device), _res_table(top.first_atom, top.n_atoms))))


def radius_of_gyration(xyz, sel=None):
    """xyz [S, n_atoms, 3] (device) -> float64 [S] on the device: sqrt(sum |x - c|^2 / m) about the unweighted centroid c
    of the atoms `sel` (default: all), m their number - G of codlad_ens_moments, no kernel of its own.  NaN for a structure
    with a coordinate that is not a number."""
    x = _inputs.structures(xyz, "radius_of_gyration: xyz")
    sel, n_sel = _inputs.selection(sel, x.shape[1], x.device)
    mom = _moments(x, x.shape[0], x.shape[1], sel, n_sel)
    return torch.sqrt(mom[:, 3] / float(n_sel or x.shape[1]))


def contact_map(xyz, sel=None, cutoff=8.0):
    """xyz [S, n_atoms, 3] (device) -> dict: counts int32 [m, m] (device), the number of structures in which atoms
    sel[a] and sel[b] (default: all atoms, m = n_atoms) are closer than `cutoff` (d^2 < fl32(cutoff^2) in fp32); frequency
    float64 [m, m] = counts / S; n_struct = S.  Symmetric, diagonal 0; a distance that is not a number is no contact."""
    x = _inputs.structures(xyz, "contact_map: xyz")
    if not float(cutoff) >= 0:
        raise ValueError(f"contact_map: cutoff must be >= 0, got {cutoff}")
    S, n = x.shape[0], x.shape[1]
    sel, n_sel = _inputs.selection(sel, n, x.device)
    m = n_sel or n
    counts = torch.empty(m, m, dtype=torch.int32, device=x.device)
    rc = _lib.lib().codlad_contact_counts(_lib.ptr(x), S, n, _lib.ptr(sel), n_sel, C.c_float(float(cutoff) ** 2),
                                          _lib.ptr(counts), _lib.stream_ptr(x.device))
    _lib.check(rc, "codlad_contact_counts")
    # a tensor divisor: the correctly rounded quotient (a Python scalar would be turned into a multiplication by 1 / S)
    return dict(counts=counts, frequency=counts.to(torch.float64) / torch.tensor(float(S), dtype=torch.float64, device=x.device),
                n_struct=S)
