"""lDDT against the true frames (codlad_lddt, csrc/lddt_kernels.hip): how close every generated all-atom structure is to the
all-atom frame its CA trace came from - without a superposition, per atom, per residue and per structure."""
import ctypes as C
import math

import numpy as np
import torch

from .. import _lib
from . import _inputs

LDDT_MAX_THRESHOLDS, LDDT_MAX_ATOMS = _lib.LDDT_MAX_THRESHOLDS, _lib.LDDT_MAX_ATOMS
LDDT_THRESHOLDS = (0.5, 1.0, 2.0, 4.0)
# residue name -> the pairs of atom names a 180 degree flip of its symmetric group exchanges, all of them together
LDDT_SYMMETRIC = {"ASP": (("OD1", "OD2"),), "GLU": (("OE1", "OE2"),), "PHE": (("CD1", "CD2"), ("CE1", "CE2")),
                  "TYR": (("CD1", "CD2"), ("CE1", "CE2")), "ARG": (("NH1", "NH2"),), "LEU": (("CD1", "CD2"),),
                  "VAL": (("CG1", "CG2"),)}

__all__ = ["LDDT_MAX_THRESHOLDS", "LDDT_MAX_ATOMS", "LDDT_THRESHOLDS", "LDDT_SYMMETRIC", "lddt_symmetry", "lddt_ref_index",
           "lddt_lists", "lddt"]


def lddt_symmetry(top):
    """int32 numpy [n_atoms]: swap_partner of a dataset_builder.Topology by LDDT_SYMMETRIC - the atom an atom exchanges
    coordinates with when its residue is flipped, itself for every other atom.  A residue that lacks one of the named atoms
    of its type is not symmetric.  Built once per topology."""
    def build():
        partner = np.arange(top.n_atoms, dtype=np.int32)
        for r, nm in enumerate(top.res_names):
            pairs = [(top.atom(r, a), top.atom(r, b)) for a, b in LDDT_SYMMETRIC.get(nm, ())]
            if pairs and min(min(p) for p in pairs) >= 0:
                for a, b in pairs:
                    partner[a], partner[b] = b, a
        return partner
    return _inputs.cached(top, "_lddt_symmetry", "host", build)


def lddt_ref_index(n_struct, n_ref, ref_index=None):
    """int32 numpy [n_struct]: the reference frame of every model.  Default: model s against frame s when there are as many
    frames as models, every model against frame 0 when there is one frame.  ValueError for an entry outside [0, n_ref)."""
    if ref_index is None:
        if n_ref == n_struct:
            return np.arange(n_struct, dtype=np.int32)
        if n_ref == 1:
            return np.zeros(n_struct, dtype=np.int32)
        raise ValueError(f"lddt: {n_struct} structures and {n_ref} reference frames need a ref_index")
    idx = torch.as_tensor(ref_index).detach().cpu().reshape(-1).to(torch.int64).numpy()
    if idx.shape[0] != n_struct:
        raise ValueError(f"lddt: ref_index has {idx.shape[0]} entries for {n_struct} structures")
    if idx.min() < 0 or idx.max() >= n_ref:
        raise ValueError(f"lddt: ref_index has an entry outside [0, {n_ref}), the reference frames")
    return idx.astype(np.int32)


def _tables(res_ptr, n_atoms, sel, swap_partner):
    """The host tables codlad_lddt reads, by POSITION in the selection (include/codlad_hip.h) -> dict of int32 numpy: res [m],
    res_ptr [R + 1] and res_pos [m] (positions by residue), partner [m], moved [n_moved]."""
    ptr = np.asarray(res_ptr).reshape(-1).astype(np.int64)
    if ptr.shape[0] < 2 or ptr[0] != 0 or ptr[-1] != n_atoms or (np.diff(ptr) < 0).any():
        raise ValueError(f"lddt: res_ptr must rise from 0 to n_atoms = {n_atoms} (the atoms of residue r are res_ptr[r] .. res_ptr[r + 1] - 1)")
    R = ptr.shape[0] - 1
    res_atom = np.repeat(np.arange(R), np.diff(ptr))
    atoms = np.arange(n_atoms) if sel is None else np.asarray(sel, dtype=np.int64)
    m = atoms.shape[0]
    pos = np.full(n_atoms, -1, dtype=np.int64)
    pos[atoms] = np.arange(m)
    if (pos[atoms] != np.arange(m)).any():
        raise ValueError("lddt: sel lists an atom twice")
    res = res_atom[atoms]
    partner = np.arange(m)
    if swap_partner is not None:
        sp = np.asarray(swap_partner).reshape(-1).astype(np.int64)
        if sp.shape[0] != n_atoms or sp.min() < 0 or sp.max() >= n_atoms:
            raise ValueError(f"lddt: swap_partner must hold {n_atoms} atom indices")
        if (sp[sp] != np.arange(n_atoms)).any() or (res_atom[sp] != res_atom).any():
            raise ValueError("lddt: swap_partner must exchange atoms in pairs within a residue")
        moved_atom = sp != np.arange(n_atoms)
        # a residue with a moved atom that is not selected is not symmetric
        broken = np.zeros(R, dtype=bool)
        broken[res_atom[moved_atom & (pos < 0)]] = True
        move = moved_atom[atoms] & ~broken[res]
        partner = np.where(move, pos[sp[atoms]], partner)
    order = np.argsort(res, kind="stable")
    out = dict(res=res, res_ptr=np.concatenate([[0], np.cumsum(np.bincount(res, minlength=R))]), res_pos=order, partner=partner,
               moved=np.nonzero(partner != np.arange(m))[0])
    return {k: np.ascontiguousarray(v, dtype=np.int32) for k, v in out.items()}


def _positive(values, what):
    try:
        vals = [float(v) for v in values]
    except (TypeError, ValueError):
        vals = [math.nan]
    if not all(math.isfinite(v) and v > 0 for v in vals):
        raise ValueError(f"lddt: {what} must be positive finite numbers, got {values!r}")
    return vals


def _params(cutoff, thresholds, seq_sep):
    """The checks that need no device -> (cutoff, [thresholds], seq_sep)."""
    thr = _positive(thresholds if np.ndim(thresholds) else [thresholds], "thresholds")
    if not 1 <= len(thr) <= LDDT_MAX_THRESHOLDS:
        raise ValueError(f"lddt: 1 .. {LDDT_MAX_THRESHOLDS} thresholds (CODLAD_LDDT_MAX_THRESHOLDS), got {len(thr)}")
    cutoff, = _positive([cutoff], "cutoff")
    if isinstance(seq_sep, bool) or not isinstance(seq_sep, (int, np.integer)) or seq_sep < 1:
        raise ValueError(f"lddt: seq_sep must be an integer >= 1, got {seq_sep!r}")
    return cutoff, thr, int(seq_sep)


def _launch(x, ref, idx, n_sel, sel, tab, params):
    cutoff, thr, seq_sep = params
    dev = x.device
    S, n, F, T = x.shape[0], x.shape[1], ref.shape[0], len(thr)
    if n > LDDT_MAX_ATOMS:
        raise ValueError(f"lddt: at most {LDDT_MAX_ATOMS} atoms (CODLAD_LDDT_MAX_ATOMS), got {n}")
    m, R, M = tab["res"].shape[0], tab["res_ptr"].shape[0] - 1, tab["moved"].shape[0]
    i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device=dev)                        # noqa: E731
    out = dict(atom_total=i32(S, m), atom_preserved=i32(S, m, T), residue_total=i32(S, R), residue_preserved=i32(S, R, T),
               residue=torch.empty(S, R, dtype=torch.float64, device=dev), counts=torch.empty(S, T + 1, dtype=torch.int64, device=dev),
               swapped=torch.empty(S, R, dtype=torch.uint8, device=dev), finite=torch.empty(S, dtype=torch.uint8, device=dev))
    out["global"] = torch.empty(S, dtype=torch.float64, device=dev)
    scratch = torch.empty(S, R, 2, dtype=torch.int64, device=dev) if M else None    # the decision sums: the call zeroes them
    thr_c = (C.c_float * T)(*thr)
    p = _lib.ptr
    rc = _lib.lib().codlad_lddt(p(x), S, p(ref), F, p(idx), n, p(sel), n_sel, p(tab["res"]), R, p(tab["res_ptr"]), p(tab["res_pos"]),
                                p(tab["partner"]) if M else None, p(tab["moved"]) if M else None, M, C.c_float(cutoff), thr_c, T,
                                int(seq_sep), p(out["atom_total"]), p(out["atom_preserved"]), p(out["residue_total"]),
                                p(out["residue_preserved"]), p(out["residue"]), p(out["counts"]), p(out["global"]),
                                p(out["swapped"]), p(out["finite"]), p(scratch), _lib.stream_ptr(dev))
    _lib.check(rc, "codlad_lddt")
    out["swapped"], out["finite"] = out["swapped"].view(torch.bool), out["finite"].view(torch.bool)
    return out


def _on(dev, tab):
    return {k: torch.from_numpy(v).to(dev) for k, v in tab.items()}


def _checked(xyz, ref, n_atoms, ref_index):
    x = _inputs.structures(xyz, "lddt: xyz", n_atoms)
    y = _inputs.structures(ref, "lddt: ref", n_atoms)
    if y.device != x.device:
        raise ValueError("lddt: xyz and ref are on different devices")
    idx = torch.from_numpy(lddt_ref_index(x.shape[0], y.shape[0], ref_index)).to(x.device)
    return x, y, idx


def lddt_lists(xyz, ref, res_ptr, swap_partner=None, ref_index=None, sel=None, cutoff=15.0, thresholds=LDDT_THRESHOLDS,
               seq_sep=1):
    """lddt for atoms given as lists: res_ptr [R + 1] (the atoms of residue r are res_ptr[r] .. res_ptr[r + 1] - 1, all
    n_atoms of them), swap_partner [n_atoms] (the atom an atom exchanges coordinates with when its residue is flipped,
    itself where there is none; None: no symmetry).  The tables are rebuilt on every call: for a protein use lddt."""
    params = _params(cutoff, thresholds, seq_sep)
    _inputs.need_cuda(xyz, "lddt: xyz")
    n_atoms = int(np.asarray(res_ptr).reshape(-1)[-1]) if np.size(res_ptr) else 0
    x, y, idx = _checked(xyz, ref, n_atoms, ref_index)
    sel_d, n_sel = _inputs.selection(sel, n_atoms, x.device)
    tab = _tables(res_ptr, n_atoms, None if sel_d is None else sel_d.cpu().numpy(), swap_partner)
    return _launch(x, y, idx, n_sel, sel_d, _on(x.device, tab), params)


def lddt(xyz, ref, top, ref_index=None, sel=None, cutoff=15.0, thresholds=LDDT_THRESHOLDS, seq_sep=1, symmetry=True):
    """xyz [S, n_atoms, 3] generated structures and ref [F, n_atoms, 3] true frames (device) of the topology `top`: the
    local distance difference test (Mariani et al. 2013) of structure s against frame ref_index[s] (default: s when F == S,
    0 when F == 1).  sel: the atoms that take part (index list; None: all; sel=top.select("CA") is the CA-only lDDT); an
    atom that is not selected is never read.  Everything per atom is indexed by the position in sel, m = len(sel).

    In float32, one rounding per operation, for every ordered pair of selected atoms i != j whose residue numbers differ by
    seq_sep or more (default 1: only pairs within a residue are left out; chains are not treated specially):
        d_ref = sqrtf((dx*dx + dy*dy) + dz*dz) on the true frame; the pair is INCLUDED iff d_ref < cutoff (strict)
        d_mod the same on the structure; the pair is PRESERVED at k iff fabsf(d_mod - d_ref) < thresholds[k] (strict)
    -> dict of device tensors, R = top.n_residues, T = len(thresholds) (1 .. 8):
      atom_total int32 [S, m]            the included partners of an atom
      atom_preserved int32 [S, m, T]     of those, the preserved ones
      residue_total int32 [S, R], residue_preserved int32 [S, R, T]: their sums over a residue's selected atoms
      counts int64 [S, 1 + T]            total, then preserved at each k, over all selected atoms
      residue float64 [S, R]             sum_k residue_preserved / (T * residue_total): integer sums, one float64 division;
                                         NaN where the residue has no included pair
      global float64 [S]                 the same over all selected atoms
      swapped bool [S, R]                symmetry: the residue was scored with its symmetric atoms exchanged
      finite bool [S]                    False: a selected coordinate of the structure or of its true frame is NaN or +-inf;
                                         then every count is -1, every score NaN, swapped False; the others keep their bits
    symmetry (default on): a residue with a chemically symmetric group (LDDT_SYMMETRIC; all named atoms present and selected)
    is scored both ways against the rest in its original naming, and exchanged iff that keeps STRICTLY more distances over its
    atoms and all k; decided per (structure, residue); the counts are those of a final pass with every chosen exchange.
    Totals never depend on the structure.  Integer counts with one writer each: the bits repeat from call to call and do not
    depend on the other structures of the call.  No host synchronisation unless ref_index is a device tensor."""
    params = _params(cutoff, thresholds, seq_sep)
    x, y, idx = _checked(xyz, ref, top.n_atoms, ref_index)
    dev = x.device
    sel_d, n_sel = _inputs.selection(sel, top.n_atoms, dev)
    partner = lddt_symmetry(top) if symmetry else None
    build = lambda s: _on(dev, _tables(top.first_atom, top.n_atoms, s, partner))                 # noqa: E731
    tab = _inputs.cached(top, "_lddt_tables", (bool(symmetry), str(dev)), lambda: build(None)) if sel_d is None \
        else build(sel_d.cpu().numpy())
    return _launch(x, y, idx, n_sel, sel_d, tab, params)
