"""Restrained clash relaxation (codlad_relax, csrc/relax_kernels.hip): what follows the two checks - atoms that overlap
are pushed apart while every distance within two bonds and every torsion about a rigid bond is held to the input's."""
import ctypes as C

import torch

from .. import _lib
from . import _inputs

RELAX_DEFAULTS = dict(k_r=100.0, k_t=50.0, k_c=30.0, contact_scale=1.6, h0=0.01, h_max=0.1)
RELAX_ENERGIES = ("distance", "torsion", "repulsion")


def ring_bonds(bonds, n_atoms):
    """The bonds (i, j), i < j, whose ends stay connected when the bond is removed: the ring bonds of any bond graph."""
    adj = _inputs.adjacency(bonds, n_atoms)
    pairs = sorted({(min(i, j), max(i, j)) for i, j in torch.as_tensor(bonds).reshape(-1, 2).tolist()})
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
    adj = _inputs.adjacency(bonds, n_atoms)
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


def _pair_tables(csr, order):
    """The two CSRs the kernels read, from csr(order) -> exclusion_csr of the bond graph: restrained pairs, excluded pairs."""
    pair_ptr, pair_j = csr(2)
    excl_ptr, excl = (pair_ptr, pair_j) if order == 2 else csr(order)
    return dict(pair_ptr=pair_ptr, pair_j=pair_j, excl_ptr=excl_ptr, excl=excl)


def relax_tables(top, order=2):
    """The host tables of the relaxation of a dataset_builder.Topology -> dict, built once and kept on the topology object:
      radius float32 [n]                COV_CUTOFF of the element
      pair_ptr, pair_j                  exclusion_csr(bonds, 2, n): the pairs whose distance is restrained
      excl_ptr, excl                    exclusion_csr(bonds, order, n): the pairs that are never repelled
      rigid int64 [B, 2]                the rigid bonds: ring bonds (ring_bonds), the peptide bond C - N, ARG NE - CZ
      quads int32 [Q, 4]                torsion_quads over them; quad_ptr, quad_ref: quad_csr
      fixed bool [n]                    the default fixed mask: the CA atoms (a backmapped structure stays on its CG input)"""
    def build():
        n = top.n_atoms
        radius, _ptr, _words, bonds = _inputs.template_tables(top, order)
        rigid = set(ring_bonds(bonds, n))
        for r, nm in enumerate(top.res_names):
            if r + 1 < top.n_residues and top.chain_ids[r + 1] == top.chain_ids[r]:
                rigid.add((top.atom(r, "C"), top.atom(r + 1, "N")))
            if nm == "ARG":
                rigid.add((top.atom(r, "NE"), top.atom(r, "CZ")))
        have = {tuple(b) for b in bonds.tolist()}
        rigid = sorted(p for p in {(min(p), max(p)) for p in rigid} if p in have)       # a residue that lacks an atom: -1
        quads = torsion_quads(bonds, rigid, n)
        quad_ptr, quad_ref = quad_csr(quads, n)
        return dict(_pair_tables(lambda o: _inputs.template_tables(top, o)[1:3], order), radius=radius,
                    rigid=torch.tensor(rigid, dtype=torch.int64).reshape(-1, 2), quads=quads, quad_ptr=quad_ptr,
                    quad_ref=quad_ref, fixed=torch.from_numpy(top.name == "CA"))
    return _inputs.cached(top, "_relax_tables", (int(order), "host"), build)


def _relax_tables_on(top, order, dev):
    """On `dev`: radius and the two CSRs are the template's uploads (the tensors geometry_check reads), the quads its own."""
    return _inputs.cached(top, "_relax_tables", (int(order), str(dev)), lambda: dict(
        _pair_tables(lambda o: _inputs.template_tables(top, o, dev)[1:3], order), radius=_inputs.template_tables(top, order, dev)[0],
        **{k: relax_tables(top, order)[k].to(dev).contiguous() for k in ("quads", "quad_ptr", "quad_ref")}))


def _relax_lists_inputs(xyz, what, radius, bonds, quads, fixed, order):
    """-> (the checked structures, the device tables built from the lists, the fixed mask or its default: none)."""
    x, radius, bonds = _inputs.list_inputs(xyz, what, radius, bonds)
    n = radius.shape[0]
    quads = torch.as_tensor(quads).reshape(-1, 4).to(torch.int32).cpu()
    quad_ptr, quad_ref = quad_csr(quads, n)
    tab = dict(_pair_tables(lambda o: _inputs.exclusion_csr(bonds, o, n), order), radius=radius, quads=quads,
               quad_ptr=quad_ptr, quad_ref=quad_ref)
    return x, {k: t.to(x.device).contiguous() for k, t in tab.items()}, torch.zeros(n, dtype=torch.bool) if fixed is None else fixed


def _relax_constants(constants, names):
    bad = set(constants) - set(names)
    if bad:
        raise TypeError(f"relax: unknown constant(s) {sorted(bad)} (known: {', '.join(names)})")
    return [C.c_float(float(constants.get(k, RELAX_DEFAULTS[k]))) for k in names]


def _relax_fixed(fixed, x, what):
    fixed = torch.as_tensor(fixed).reshape(-1)
    if fixed.shape[0] != x.shape[1]:
        raise ValueError(f"{what}: the fixed mask has {fixed.shape[0]} atoms, the topology {x.shape[1]}")
    return fixed.to(device=x.device, dtype=torch.bool).to(torch.uint8).contiguous()


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


def _relax_energy_launch(x, xyz0, t, fixed, constants):
    fx = _relax_fixed(fixed, x, "relax_energy")
    x0 = x if xyz0 is None else _inputs.structures(xyz0, "relax_energy: xyz0", x.shape[1])
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


def _relax_launch(x, t, fixed, n_iter, constants):
    fx = _relax_fixed(fixed, x, "relax")
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
    x = _inputs.structures(xyz, "relax_energy: xyz", top.n_atoms)
    return _relax_energy_launch(x, xyz0, _relax_tables_on(top, order, x.device),
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
    x = _inputs.structures(xyz, "relax: xyz", top.n_atoms)
    return _relax_launch(x, _relax_tables_on(top, order, x.device),
                         relax_tables(top, order)["fixed"] if fixed is None else fixed, n_iter, constants)


def relax_lists(xyz, radius, bonds, quads, fixed=None, n_iter=200, order=2, **constants):
    """relax for a topology given as lists: radius [n_atoms], bonds [n_bonds, 2] (each once, i < j), quads [Q, 4] (the
    restrained torsions), fixed bool [n_atoms] (default: none).  The tables are rebuilt on every call."""
    x, t, fixed = _relax_lists_inputs(xyz, "relax", radius, bonds, quads, fixed, order)
    return _relax_launch(x, t, fixed, n_iter, constants)


def relax_energy_lists(xyz, radius, bonds, quads, xyz0=None, fixed=None, order=2, **constants):
    """relax_energy for a topology given as lists (see relax_lists)."""
    x, t, fixed = _relax_lists_inputs(xyz, "relax_energy", radius, bonds, quads, fixed, order)
    return _relax_energy_launch(x, xyz0, t, fixed, constants)
