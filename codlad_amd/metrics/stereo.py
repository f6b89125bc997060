"""Stereochemistry check (codlad_stereo_check, csrc/stereo_kernels.hip): the torsions and chiral volumes of generated
structures and the decisions taken on them - the part of the reference-free judgement the covalent graph cannot see."""
import torch

from .. import _lib
from . import _inputs

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
    def build():
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
        return sites, kind
    return _inputs.cached(top, "_stereo_tables", "host", build)


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
    x = _inputs.structures(xyz, "stereo_check: xyz", top.n_atoms)
    dev = x.device
    sites, kind = _inputs.cached(top, "_stereo_tables", str(dev),
                                 lambda: tuple(t.to(dev).contiguous() for t in stereo_tables(top)))
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
