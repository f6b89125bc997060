"""CA-only input: a coarse-grained trajectory (one bead per residue, on the alpha carbon) -> the batches of the latent
sampling path, with no all-atom structure anywhere.

The sampling path reads `CG_nxyz`, `num_CGs`, `CG_nbr_list`, `OG_CG_nxyz`, `prot_idx` and the `info` tables; all of them
follow from the sequence and the CA coordinates.  `read_cg_pdb` takes both from a (multi-model) PDB file, of which only the
CA records are read, `load_cg_frames` takes the frames from an .xtc instead, `template_topology` gives every residue its
template heavy atoms in the standard file order (what the generated structure will hold) and `cg_batches` builds the batch
dicts exactly as `load_dataset` builds the same keys from atoms.

As on every route, the chain loses its first and last residue: they supply the flanking CAs of the internal-coordinate
construction and are not generated.

Units: Angstrom.
"""
from collections import namedtuple

import numpy as np
import torch

from .dataset_builder import RES2IDX, THREE_LETTER_TO_ONE, CGDataset, Topology
from .ic_tables import PDB_ATOM_ORDER, core_atoms

MAX_FRAMES_PER_BATCH = 96          # as load_dataset: batch_size = min(n_frames, 96)

CgSequence = namedtuple("CgSequence", "res_names res_seqs chain_ids")      # one entry per residue, tuples


def _label(res_name, chain, res_seq):
    return f"{res_name} {res_seq.strip()} of chain {chain.strip() or '-'}"


def read_cg_pdb(path):
    """-> (CgSequence, ca_xyz float32 [n_models, n_res, 3], Angstrom).  Only the CA records are kept, so an all-atom file
    and the same file stripped to its CA lines give the same result.  Conventions of dataset_builder.read_pdb: the first
    alternate location only, chains numbered in order of appearance, the sequence is the first model's and every model must
    list as many residues.  ValueError (naming the residue) for a residue without a template, without a CA or with two."""
    residues, key, chains = [], None, {}     # first model: [name, chain letter, resSeq field, CA count] in file order
    frames, cur, n_records, first = [], [], 0, True
    with open(path) as f:
        for line in f:
            rec = line[:6]
            if rec.startswith("ENDMDL") or rec.startswith("END   ") or rec.strip() == "END":
                if n_records:
                    frames.append(cur)
                    cur, n_records, first, key = [], 0, False, None
                continue
            if rec not in ("ATOM  ", "HETATM"):
                continue
            if line[16] not in (" ", "A"):                  # alternate locations: the first one only
                continue
            n_records += 1
            name, elem = line[12:16].strip(), line[76:78].strip().upper()
            is_ca = name == "CA" and elem in ("", "C")      # not a calcium ion
            if first:
                k = (line[21], line[22:27])
                if k != key:
                    key = k
                    residues.append([line[17:20].strip(), line[21], line[22:27], 0])
                    chains.setdefault(line[21], len(chains))
                residues[-1][3] += is_ca
            if is_ca:
                cur.append((float(line[30:38]), float(line[38:46]), float(line[46:54])))
    if n_records:
        frames.append(cur)
    if not residues:
        raise ValueError(f"{path}: no ATOM records")
    for nm, chain, seq, n_ca in residues:
        if nm not in core_atoms:
            raise ValueError(f"{path}: residue {_label(nm, chain, seq)} has no template (known: {' '.join(sorted(core_atoms))})")
        if n_ca != 1:
            raise ValueError(f"{path}: residue {_label(nm, chain, seq)} has {n_ca} CA atoms, exactly one is needed")
    bad = [m for m, fr in enumerate(frames) if len(fr) != len(residues)]
    if bad:
        raise ValueError(f"{path}: model {bad[0] + 1} has {len(frames[bad[0]])} CA atoms, the first has {len(residues)}")
    seq = CgSequence(tuple(r[0] for r in residues), tuple(int(r[2][:4]) for r in residues),
                     tuple(chains[r[1]] for r in residues))
    return seq, np.asarray(frames, dtype=np.float32)


def load_cg_frames(pdb_path, xtc_path=None):
    """(CgSequence, ca_xyz [F, n_res, 3]) of a --cg_pdb file; with xtc_path the frames come from that trajectory (one atom
    per CA of the PDB file, which then supplies the sequence only)."""
    seq, ca_xyz = read_cg_pdb(pdb_path)
    if xtc_path is not None:
        from .xtc import read_xtc
        xyz = read_xtc(xtc_path)[0]
        if xyz.shape[1] != len(seq.res_names):
            raise ValueError(f"{xtc_path} has {xyz.shape[1]} atoms, {pdb_path} has {len(seq.res_names)} CA atoms: the "
                             "trajectory must hold exactly the CA beads")
        ca_xyz = np.ascontiguousarray(xyz, dtype=np.float32)
    return seq, ca_xyz


def template_topology(res_names, res_seqs=None, chain_ids=None):
    """The Topology a sequence will have once its atoms are generated: every residue with its template heavy atoms in the
    standard PDB file order (PDB_ATOM_ORDER)."""
    unknown = [nm for nm in res_names if nm not in PDB_ATOM_ORDER]
    if unknown:
        raise ValueError(f"residue {unknown[0]} has no template (known: {' '.join(sorted(PDB_ATOM_ORDER))})")
    return Topology(res_names, [PDB_ATOM_ORDER[nm] for nm in res_names], res_seqs, chain_ids)


def chunk_plan(n_frames, max_frames=MAX_FRAMES_PER_BATCH):
    """[(first frame, end frame)] of the batches one trajectory is cut into (as load_dataset's DataLoader cuts it)."""
    bs = min(n_frames, max_frames)
    return [(b, min(b + bs, n_frames)) for b in range(0, n_frames, bs)]


def cg_batches(top, ca_xyz, params, device="cuda"):
    """top: the template Topology of ALL residues (flanking ones included), ca_xyz [F, n_res, 3] -> generator of
    (batch, info): the collated batch dicts of <= 96 frames with exactly the keys the latent sampling path reads (CG_nxyz,
    OG_CG_nxyz, num_CGs, CG_nbr_list, prot_idx - built as build_ic_peptide_dataset builds them, the neighbour list by the
    same CGDataset.generate_neighbor_list) and the info tables of the template atoms.  None of the keys the evaluation
    block needs: there is nothing to compare with."""
    from .dataset_module import CG_collate
    from .protein_module import info_from_residues
    ca_xyz = torch.as_tensor(np.asarray(ca_xyz), dtype=torch.float32)
    if ca_xyz.dim() != 3 or ca_xyz.shape[1] != top.n_residues or ca_xyz.shape[2] != 3:
        raise ValueError(f"ca_xyz {tuple(ca_xyz.shape)} does not hold one CA per residue of the topology ({top.n_residues})")
    if top.n_residues < 3:
        raise ValueError("a chain needs at least 3 residues: the first and the last only flank the generated ones")
    info, _n_cg = info_from_residues(top.res_names, top.atom_names)
    cg_res = torch.tensor([RES2IDX[THREE_LETTER_TO_ONE[nm[:3]]] for nm in top.res_names], dtype=torch.float32).reshape(-1, 1)
    props = {k: [] for k in ("CG_nxyz", "OG_CG_nxyz", "num_CGs", "prot_idx")}
    for f in range(ca_xyz.shape[0]):
        og = torch.cat([cg_res, ca_xyz[f]], dim=-1)
        props["OG_CG_nxyz"].append(og)
        props["CG_nxyz"].append(og[1:-1])
        props["num_CGs"].append(torch.tensor([og.shape[0] - 2]))
        props["prot_idx"].append(torch.tensor([0.0]))
    dataset = CGDataset(props)
    dataset.generate_neighbor_list(atom_cutoff=params["atom_cutoff"], cg_cutoff=params["cg_cutoff"], device=device)
    for a, b in chunk_plan(len(dataset)):
        yield CG_collate([dataset[i] for i in range(a, b)]), info
