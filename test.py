#!/usr/bin/env python3
"""Inference entry point, drop-in for the sampling part of the reference's test.py
(`--experiment latent` and `--experiment recon`), running on the HIP path.  `--help` describes every flag.

Kept from the reference (test.py:894-961): flag names and defaults, checkpoint locations
(`./results/<exp>/protein_weights_{best,last,step_N}.pt` with `net_model` / `ema_model`, VQ-VAE
directories of utils/model_module.py), the call sequence build_model -> create_diffusion ->
p_sample_loop -> get_norm_feature -> latent_decode -> ic_to_xyz, and the output directory.
Different by design: all ensemble members of a batch of frames are sampled in ONE launch set (the
reference loops over them); the C2 prior call that only supplies `mask` (test.py:495) is replaced by
the length mask; mdtraj I/O is replaced by saving coordinates as .npy (and multi-model PDB + .xtc, --save_pdb);
torchdiffeq.odeint by the fused ODE loop; every batch draws its noise from its own generator, so a structure does
not depend on the number of GPUs.
Data: `--pdb_files`, `--data_process --data_files`, `--cg_pdb` (CA-only, no true atoms: no Evaluation block) or
`--synthetic` (no PED/PDB/Atlas files ship with the reference).
Additions with no counterpart in the reference: the samplers (--sampler, --timestep_spacing, --fix_residues), the
scores of a checkpoint (--experiment bpd / fmloss), --relax, and the analyses of the written structures: the rows of
ANALYSES below, each of which says in one place where it applies, what it launches, writes and prints.  Everything
a batch launches is enqueued before its one torch.cuda.synchronize() and read back after it.
"""
import argparse
import os
import pickle
import time
import types

import numpy as np
import torch

from codlad_amd import metrics, synth
from codlad_amd.diffusion_and_flow import PinLatents, create_diffusion
from codlad_amd.models.latent_model import MPNN_models
from codlad_amd.utils.dataset_module import CG_collate, get_norm_feature
from codlad_amd.utils.model_module import build_vae, get_vae_model, load_decoder_state
from codlad_amd.utils.utils_ic import ic_to_xyz


def build_model(args):
    if "mpnn" not in args.backbone:
        raise NotImplementedError(f"backbone {args.backbone!r}: only mpnn_diffusion is built")
    return MPNN_models[args.backbone](input_size=args.latent_size, unconditional=not args.cond,
                                      diffusion=args.model, self_condition=args.self_condition)


def load_denoiser(args, device, load=True):
    """load=False (ranks > 0 of a multi-GPU run): the module with its constructor's initialisation and NO file
    access - rank 0's weights arrive by broadcast (`parallel.broadcast_module_state`)."""
    model = build_model(args)
    if not load:
        return model.to(device).eval()
    if args.synthetic_weights:
        model.load_state_dict(synth.denoiser_state_dict(1234, self_condition=args.self_condition,
                                                        flow=args.model != "diffusion"), strict=True)
    else:
        tag = {"best": "best", "last": "last"}.get(args.model_step, f"step_{args.model_step}")
        ckpt = torch.load(f"./results/{args.exp}/protein_weights_{tag}.pt", map_location="cpu")
        sd = ckpt["net_model" if args.ckpt_type == "net" else "ema_model"]
        try:
            model.load_state_dict(sd, strict=True)
        except RuntimeError:
            model.load_state_dict({k[7:]: v for k, v in sd.items()}, strict=True)
    return model.to(device).eval()


def parse_fix_residues(spec):
    """--fix_residues SPEC, e.g. "3-20,41" -> sorted 1-based residue positions (ranges inclusive).  Raises ValueError on
    an empty, malformed, non-positive or reversed spec."""
    if spec is None or not spec.strip():
        raise ValueError("--fix_residues: empty residue spec")
    pos = set()
    for part in spec.split(","):
        part = part.strip()
        lo, sep, hi = part.partition("-")
        if not lo.strip().isdigit() or (sep and not hi.strip().isdigit()):
            raise ValueError(f"--fix_residues: {part!r} is not a position or a range a-b of 1-based positions")
        a, b = int(lo), int(hi) if sep else int(lo)
        if a < 1 or b < a:
            raise ValueError(f"--fix_residues: {part!r} is out of range (positions start at 1, ranges run upwards)")
        pos.update(range(a, b + 1))
    return sorted(pos)


def fix_residue_mask(positions, L, n_samples, device=None):
    """[n_samples, L] bool: True at the pinned positions of a structure of L CG residues (flanking caps excluded)."""
    if positions[-1] > L:
        raise ValueError(f"--fix_residues: position {positions[-1]} is out of range for a structure of {L} residues")
    mask = torch.zeros(n_samples, L, dtype=torch.bool, device=device)
    mask[:, torch.tensor(positions, device=device) - 1] = True
    return mask


def check_fix_residues(args):
    """Where --fix_residues applies: DDPM latent sampling decoded by a VQ-VAE whose encoder supplies the known latents,
    on input that carries atoms (--pdb_files, --data_process pickles, --synthetic).  -> the parsed positions or None."""
    if getattr(args, "fix_residues", None) is None:
        return None
    if args.experiment != "latent" or args.model != "diffusion":
        raise SystemExit("--fix_residues needs --experiment latent --model diffusion (residue pinning is a denoised_fn of "
                         "the DDPM sampler; the flow-matching ODE path has no such hook)")
    if args.vae_type not in ("N6", "K3", "K4"):
        raise SystemExit(f"--fix_residues needs a VQ-VAE (N6 / K3 / K4) to encode the known residues, not {args.vae_type!r}")
    if not (args.synthetic or getattr(args, "pdb_files", None) or args.data_process):
        raise SystemExit("--fix_residues needs input with atoms: --pdb_files, --data_process --data_files or --synthetic")
    try:
        return parse_fix_residues(args.fix_residues)
    except ValueError as e:
        raise SystemExit(str(e))


CG_NEEDS_ATOMS = {"recon": "encodes the input's atoms", "genzprot": "is evaluated against the input's atoms",
                  "bpd": "scores the latents of the input's atoms", "fmloss": "scores the latents of the input's atoms"}


def check_cg_input(args):
    """Where --cg_pdb / --cg_xtc / --geometry_check apply.  A CA-only input has no atoms: it feeds latent sampling (every
    sampler, every flow model) and nothing that encodes, pins or compares with atoms.  Sets args.geometry_check (implied by
    --cg_pdb) and returns it."""
    cg, xtc = getattr(args, "cg_pdb", None), getattr(args, "cg_xtc", None)
    want = bool(getattr(args, "geometry_check", False)) or bool(cg)
    if xtc and not cg:
        raise SystemExit("--cg_xtc needs --cg_pdb: the PDB file supplies the sequence of the trajectory's CA beads")
    if xtc and len(cg) != 1:
        raise SystemExit(f"--cg_xtc goes with a single --cg_pdb file (the sequence of that trajectory), not {len(cg)}")
    if cg:
        if args.synthetic or getattr(args, "pdb_files", None) or args.data_process:
            raise SystemExit("--cg_pdb is an input route of its own: not together with --pdb_files, --data_process or --synthetic")
        if args.experiment != "latent":
            raise SystemExit(f"--cg_pdb needs --experiment latent: {args.experiment!r} "
                             f"{CG_NEEDS_ATOMS.get(args.experiment, 'needs atoms')}, and a CA-only input has none")
        if getattr(args, "fix_residues", None) is not None:
            raise SystemExit("--cg_pdb cannot be combined with --fix_residues: the pinned latents are encoded from the input's "
                             "atoms, and a CA-only input has none")
        if getattr(args, "superpose", "none") == "ref":
            raise SystemExit("--cg_pdb cannot be combined with --superpose ref: there is no true structure to superpose on "
                             "(use --superpose first)")
    elif want:
        refuse_out_of_scope(args, GEOMETRY)
    args.geometry_check = want
    return want


REQUIRED, USED = "required", "used"        # what an analysis needs of the input route's topology; None: nothing


def refuse_out_of_scope(args, row):
    """The scope refusals every analysis (and --relax) shares, each with its own verb: structures are generated (not with
    --experiment bpd / fmloss) and, for a row that requires the topology, the input route knows it (--data_process pickles
    carry none).  The refusals of --cg_pdb itself are check_cg_input's; a row that requires the topology leaves them to it."""
    early = row.topology == REQUIRED and not row.late
    if early and getattr(args, "cg_pdb", None):
        return
    experiment = getattr(args, "experiment", "latent")
    if experiment in ("bpd", "fmloss"):
        raise SystemExit(f"{row.flag} {row.does}: --experiment {experiment} generates none")
    if early and args.data_process and not args.synthetic:
        raise SystemExit(f"{row.flag} needs the topology of the structures: --data_process pickles carry none "
                         "(use --pdb_files, --cg_pdb or --synthetic)")


def topology_of(name, row):
    """The Topology of the written residues of one output file, as `row` needs it: a row that requires one is refused on an
    input route that knows none, one that merely uses it gets None there, and so does a row that needs none."""
    if row.topology and name in _GEOMETRY_TOP:
        return _GEOMETRY_TOP[name]
    if row.topology == REQUIRED:
        raise SystemExit(f"{row.flag}: the topology of {name} is not known on this input route")
    return None


def check_saxs_hydration(args):
    """Where --saxs_hydration applies: only with --saxs; without its two numbers it fits them, which needs --saxs_data.
    Returns None (off), () (fit c1 and c2) or (c1, c2)."""
    v = getattr(args, "saxs_hydration", None)
    if v is None:
        return None
    if not getattr(args, "saxs", 0):
        raise SystemExit("--saxs_hydration needs --saxs: it is the hydration shell and the contrast of the profile --saxs computes")
    if len(v) not in (0, 2):
        raise SystemExit(f"--saxs_hydration takes C1 and C2 or nothing (then both are fitted to --saxs_data), got {len(v)} number(s)")
    if not v and not getattr(args, "saxs_data", None):
        raise SystemExit("--saxs_hydration without C1 and C2 fits them: that needs the curve of --saxs_data")
    if v and not (v[0] > 0 and np.isfinite(v).all()):
        raise SystemExit(f"--saxs_hydration: C1 scales the excluded volume and must be positive, C2 a number, got {v[0]} {v[1]}")
    args.saxs_hydration = tuple(float(c) for c in v)
    return args.saxs_hydration


def check_saxs_reweight(args):
    """Where --saxs_reweight applies: with --saxs and --saxs_data; every THETA a positive finite number.  Returns the
    thetas as a tuple, () = off."""
    v = getattr(args, "saxs_reweight", None)
    if v is None:
        args.saxs_reweight = ()
        return ()
    if not getattr(args, "saxs", 0):
        raise SystemExit("--saxs_reweight needs --saxs: it reweights the structures against the profiles --saxs computes")
    if not getattr(args, "saxs_data", None):
        raise SystemExit("--saxs_reweight needs --saxs_data: the curve the weighted mean is to agree with")
    if not v:
        raise SystemExit("--saxs_reweight takes one THETA or more (the confidence in the prior; try 1000 100 10 1)")
    for t in v:
        if not (t > 0 and t == t and t != float("inf")):
            raise SystemExit(f"--saxs_reweight: every THETA must be a positive finite number, got {t}")
    args.saxs_reweight = tuple(float(t) for t in v)
    return args.saxs_reweight


def compare_truth(name, batch, flag="--compare"):
    """The true coordinates --compare and --lddt measure against: batch["nxyz"][:, 1:], [frames * n_atoms, 3]; SystemExit when
    the input route has none (--cg_pdb)."""
    if "nxyz" not in batch:
        raise SystemExit(f"{flag}: {name} has no true frames to compare with (nxyz; a CA-only input such as --cg_pdb has none)")
    return batch["nxyz"][:, 1:]


def compare_no_atom_masked(batch):
    """True when mask_xyz_list (a boolean mask or an index list over the atoms) masks nothing: the torsions of the true frames
    are then those of real atoms."""
    m = batch.get("mask_xyz_list")
    if m is None:
        return True
    m = torch.as_tensor(m)
    return not bool(m.any()) if m.dtype == torch.bool else m.numel() == 0


def lddt_selection(batch, n_frames, n_atoms):
    """The atoms --lddt scores: those mask_xyz_list (a boolean mask or an index list over frames * n_atoms) masks in no frame,
    as an index list; None when nothing is masked."""
    m = batch.get("mask_xyz_list")
    if m is None:
        return None
    m = torch.as_tensor(m).cpu()
    masked = torch.zeros(n_frames * n_atoms, dtype=torch.bool)
    masked[m.reshape(-1) if m.dtype == torch.bool else m.reshape(-1).long()] = True
    masked = masked.reshape(n_frames, n_atoms).any(0)
    return None if not bool(masked.any()) else torch.nonzero(~masked).reshape(-1).tolist()


def pca_selection(name, n_atoms, atoms, ca):
    """The atoms --pca runs over for one output file: the CA indices `ca` (atoms "ca") or None for all -> sel; SystemExit
    when they are not known or hold more coordinates than one covariance takes."""
    if atoms == "ca":
        if not ca:
            raise SystemExit(f"--pca: the CA atoms of {name} are not known on this input route (use --pca_atoms all)")
        sel = list(ca)
    else:
        sel = None
    m = n_atoms if sel is None else len(sel)
    if 3 * m > metrics.PCA_MAX_DIM:
        raise SystemExit(f"--pca: {name} has 3 x {m} = {3 * m} coordinates over the chosen atoms, at most {metrics.PCA_MAX_DIM} "
                         f"(--pca_atoms ca runs over the CA atoms)")
    return sel


def read_saxs_data(path):
    """--saxs_data: three whitespace-separated columns q (1/A), I, sigma; `#` starts a comment -> three float64 arrays."""
    rows = []
    with open(path) as f:
        for no, line in enumerate(f, 1):
            cols = line.split("#", 1)[0].split()
            if not cols:
                continue
            try:
                if len(cols) != 3:
                    raise ValueError
                rows.append([float(c) for c in cols])
            except ValueError:
                raise SystemExit(f"--saxs_data {path}, line {no}: three columns of numbers are needed (q, I, sigma)") from None
    if len(rows) < 2:
        raise SystemExit(f"--saxs_data {path}: two rows or more are needed")
    q, I, sigma = np.array(rows, dtype=np.float64).T
    return q, I, sigma


def check_sampler(args):
    """--sampler / --eta / --timestep_spacing: DDIM and DPM-Solver++ apply to latent sampling with the diffusion model; a
    nonzero eta is a DDIM setting; the log-SNR spacing is a respacing of the diffusion model's steps."""
    sampler, eta = getattr(args, "sampler", "ddpm"), getattr(args, "eta", 0.0)
    spacing = getattr(args, "timestep_spacing", "uniform")
    if sampler not in ("ddpm", "ddim", "dpmpp"):
        raise SystemExit(f"--sampler must be ddpm or ddim (or dpmpp), not {sampler!r}")
    if eta < 0:
        raise SystemExit(f"--eta must be >= 0, got {eta}")
    if spacing not in ("uniform", "logsnr"):
        raise SystemExit(f"--timestep_spacing must be uniform or logsnr, not {spacing!r}")
    if spacing == "logsnr":
        if args.model != "diffusion":
            raise SystemExit(f"--timestep_spacing logsnr needs --model diffusion: {args.model!r} is a flow-matching model, "
                             "whose ODE solver chooses its own steps")
        if getattr(args, "num_sampling_steps", 2) < 2:
            raise SystemExit("--timestep_spacing logsnr needs --num_sampling_steps >= 2 (the first and the last base step)")
    if sampler != "ddim" and eta != 0:
        raise SystemExit("--eta applies to --sampler ddim only (the DDPM sampler and DPM-Solver++ have no eta)")
    if sampler == "ddpm":
        return
    if args.experiment != "latent":
        raise SystemExit(f"--sampler {sampler} samples latents: it needs --experiment latent, not {args.experiment!r} "
                         "(recon encodes the input, genzprot samples the conditional prior)")
    if args.model != "diffusion":
        raise SystemExit(f"--sampler {sampler} needs --model diffusion: {args.model!r} is a flow-matching model, sampled by "
                         "its ODE solver")


def respacing_spec(args):
    """The create_diffusion respacing spec of --num_sampling_steps under --timestep_spacing."""
    return ("logsnr" if getattr(args, "timestep_spacing", "uniform") == "logsnr" else "") + str(args.num_sampling_steps)


def check_bpd(args, world):
    """--experiment bpd: the variational bound of the batch's own latents under the diffusion model."""
    if args.experiment != "bpd":
        return
    if world > 1:
        raise SystemExit("--experiment bpd runs on one rank: gathering its per-step tables across ranks is not built "
                         f"(WORLD_SIZE={world})")
    if args.model != "diffusion":
        raise SystemExit(f"--experiment bpd needs --model diffusion: {args.model!r} is a flow-matching model, which has no "
                         "variational bound")
    if args.vae_type not in ("N6", "K3", "K4"):
        raise SystemExit(f"--experiment bpd needs a VQ-VAE (N6 / K3 / K4) to encode the structures, not {args.vae_type!r}")
    if not (args.synthetic or getattr(args, "pdb_files", None) or args.data_process):
        raise SystemExit("--experiment bpd needs input with atoms: --pdb_files, --data_process --data_files or --synthetic")


FMLOSS_MODELS = ("fm", "icfm", "vpfm")


def check_fmloss(args, world):
    """--experiment fmloss: the flow-matching regression loss of the batch's own latents, per time."""
    if args.experiment != "fmloss":
        return
    if world > 1:
        raise SystemExit("--experiment fmloss runs on one rank: gathering its per-time tables across ranks is not built "
                         f"(WORLD_SIZE={world})")
    if args.model == "diffusion":
        raise SystemExit("--experiment fmloss needs a flow-matching model (--model fm / icfm / vpfm): 'diffusion' is a "
                         "diffusion model, which is scored with --experiment bpd")
    if args.model not in FMLOSS_MODELS:
        raise SystemExit(f"--experiment fmloss needs --model fm / icfm / vpfm: the matcher of {args.model!r} is not built "
                         "(otcfm needs the POT package's exact transport plan, sbcfm a score head the model does not have)")
    if args.vae_type not in ("N6", "K3", "K4"):
        raise SystemExit(f"--experiment fmloss needs a VQ-VAE (N6 / K3 / K4) to encode the structures, not {args.vae_type!r}")
    if not (args.synthetic or getattr(args, "pdb_files", None) or args.data_process):
        raise SystemExit("--experiment fmloss needs input with atoms: --pdb_files, --data_process --data_files or --synthetic")
    if fmloss_steps(args) < 1:
        raise SystemExit(f"--experiment fmloss needs --num_steps >= 1, got {fmloss_steps(args)}")
    if getattr(args, "fm_sigma", 0.0) < 0:
        raise SystemExit(f"--fm_sigma must be >= 0, got {args.fm_sigma}")


def fmloss_steps(args):
    """K of --experiment fmloss: --num_steps (the reference's flag of that name, default 40)."""
    return int(args.num_steps)


def load_vae(args, device, load=True):
    """The VQ-VAE; with its e3nn encoder when the run needs it (`--experiment recon` encodes the batch's atoms, so does
    --fix_residues for the latents it pins and `--experiment bpd` for the latents it scores)."""
    enc = args.experiment in ("recon", "bpd", "fmloss") or args.fix_residues is not None
    if not load:
        return build_vae(args.vae_type, with_encoder=enc).to(device).eval()
    if args.synthetic_weights:
        vae = build_vae(args.vae_type, with_encoder=enc)
        sd = synth.vqvae_state_dict(args.vae_type, args.data_type, 4321)
        if enc:
            sd.update({"encoder." + k: v for k, v in synth.encoder_state_dict(778).items()})
            sd.update({k: v for k, v in vae.state_dict().items() if k.endswith(".offset")})
        load_decoder_state(vae, sd)
        return vae.to(device).eval()
    vae, _params = get_vae_model(args.vae_type, device=device, modelnum=args.modelnum, with_encoder=enc)
    return vae.to(device).eval()


def load_cvae(args, device, load=True):
    """The conditional VAE (`--cvae_type C2`, reference test.py:317-320): its CG prior conditions `--cond` models and IS
    the generator of `--experiment genzprot`."""
    if not load:
        return build_vae(args.cvae_type).to(device).eval()
    if args.synthetic_weights:
        cvae = build_vae(args.cvae_type)
        sd = {k: v for k, v in cvae.state_dict().items()}
        sd.update({"prior_net." + k: v for k, v in synth.prior_state_dict(777).items()})
        sd.update({"encoder." + k: v for k, v in synth.encoder_state_dict(779).items()})
        sd.update(synth.decoder_state_dict(4322, angle=False))
        load_decoder_state(cvae, sd)
        return cvae.to(device).eval()
    cvae, _params = get_vae_model(args.cvae_type, device=device)
    return cvae.to(device).eval()


_TOPOLOGY = {}                     # output name -> (residue names, atom names per residue) where known (--save_pdb)
_GEOMETRY_TOP = {}                 # output name -> Topology of the written (interior) residues (--geometry_check)
MAX_FRAMES_PER_BATCH = 96          # reference utils/dataset_module.py:220-226: batch_size = min(n_frames, 96)


def chunk_plan(n_frames, max_frames=MAX_FRAMES_PER_BATCH):
    """[(first frame, end frame)] of the batches one data file is cut into."""
    bs = min(n_frames, max_frames)
    return [(b, min(b + bs, n_frames)) for b in range(0, n_frames, bs)]


def output_name(name, chunk, n_chunks):
    """File stem of one batch's coordinates.  A data file of more than 96 frames is cut into several batches
    (possibly dealt to different ranks): each gets its own, index-tagged file, so no batch overwrites another;
    a single-batch file keeps the plain name."""
    return name if n_chunks == 1 else f"{name}_b{chunk:05d}"


def iter_batches(args):
    """Yields (output name, batch dict, info)."""
    if args.synthetic:
        lengths = {"PED": (46, 87, 92, 129), "PDB": (60, 120, 200), "Atlas": (39, 155, 505)}[args.data_type]
        for i, L in enumerate(lengths):
            prot = synth.make_protein(L, 1000 + i, n_frames=args.synthetic_frames,
                                      phospho=args.vae_type != "N6")
            plan = chunk_plan(args.synthetic_frames)
            names = [synth.IDX2THR[int(z)] for z in prot["z_full"]]
            geom_top = None
            if any(row.topology and row.on(args) for row in (RELAX,) + ANALYSES):
                from codlad_amd.utils.cg_input import template_topology
                geom_top = template_topology(names[1:-1])             # one Topology (and one set of device tables) per protein
            for c, (a, b) in enumerate(plan):
                out = output_name(f"synthetic_L{L}", c, len(plan))
                _TOPOLOGY[out] = (names, [synth.PDB_ATOM_ORDER[nm] for nm in names])
                if geom_top is not None:
                    _GEOMETRY_TOP[out] = geom_top
                batch = synth.make_batch(prot, range(a, b))
                # the encoder reads the all-atom side of the batch (recon; the known latents of --fix_residues); --compare and
                # --lddt its true coordinates
                if getattr(args, "experiment", "latent") in ("recon", "bpd", "fmloss") or getattr(args, "fix_residues", None) is not None \
                        or any(row.truth and row.on(args) for row in ANALYSES):
                    batch.update(synth.make_atoms(prot, range(a, b), seed=1000 + i))
                yield out, batch, prot["info"]
        return
    if getattr(args, "pdb_files", None):
        # reference test.py:424-436 -> load_dataset(f"{dir}/{name}", params): a multi-model PDB ensemble, here without
        # mdtraj (utils/dataset_builder.py; internal coordinates by codlad_xyz_to_ic).  Cut-offs: the VAE's modelparams
        # (the shipped ones: atom 9.0, CG 21.0, bond order 2), overridable on the command line.
        from codlad_amd.utils.dataset_module import load_dataset
        params = {"atom_cutoff": args.atom_cutoff, "cg_cutoff": args.cg_cutoff, "edgeorder": args.edgeorder}
        for path in args.pdb_files:
            stem = path[:-4] if path.endswith(".pdb") else path
            loader, info_dict, _n_atoms, _n_cgs, _z, top = load_dataset(stem, params, device="cuda")
            n_batches = len(loader)
            for c, batch in enumerate(loader):
                out = output_name(os.path.basename(stem), c, n_batches)
                _TOPOLOGY[out] = (["GLY"] + top.res_names + ["GLY"], [["CA"]] + top.atom_names + [["CA"]])
                _GEOMETRY_TOP[out] = top
                yield out, batch, info_dict[0]
        return
    if getattr(args, "cg_pdb", None):
        # a CA-only trajectory: sequence + CA frames -> template topology -> the batch keys of the latent path, built as
        # load_dataset builds them from atoms (utils/cg_input.py); one Topology per file, shared by its batches
        from codlad_amd.utils.cg_input import cg_batches, load_cg_frames, template_topology
        params = {"atom_cutoff": args.atom_cutoff, "cg_cutoff": args.cg_cutoff, "edgeorder": args.edgeorder}
        for path in args.cg_pdb:
            stem = os.path.basename(path[:-4] if path.endswith(".pdb") else path)
            try:
                seq, ca_xyz = load_cg_frames(path, getattr(args, "cg_xtc", None))
                top = template_topology(*seq)
            except ValueError as e:
                raise SystemExit(f"--cg_pdb: {e}")
            inner = top.subset_residues(1, top.n_residues - 1)
            units = list(cg_batches(top, ca_xyz, params, device="cuda"))
            for c, (batch, info) in enumerate(units):
                out = output_name(stem, c, len(units))
                _TOPOLOGY[out] = (top.res_names, top.atom_names)
                _GEOMETRY_TOP[out] = inner
                yield out, batch, info
        return
    if not args.data_process:
        raise SystemExit("xtc loading is not built: use --pdb_files (multi-model PDB), --data_process --data_files ... or --synthetic")
    for path in args.data_files:
        with open(path, "rb") as f:
            testset, info = pickle.load(f)
        plan = chunk_plan(len(testset))
        for c, (a, b) in enumerate(plan):
            yield output_name(os.path.basename(path), c, len(plan)), CG_collate([testset[i] for i in range(a, b)]), info


EVAL_KEYS = ("nxyz", "num_atoms", "bond_edge_list", "nbr_list", "bb_NO_list", "interaction_list", "pi_pi_list", "ic",
             "mask", "mask_xyz_list")


class Evaluation:
    """The evaluation block of the reference's loop (test.py:566-668, 707-785) on the device: per batch and ensemble
    member the reconstruction / coordinate / bond-graph / clash / interaction losses (codlad_eval_metrics, one launch)
    and the bond-graph validity (codlad_bond_graph_counts); per data file the summary the reference prints."""

    def __init__(self):
        self.rows, self.valid, self.ged, self.rmsd = [], [], [], []
        self.recon, self.true = [], None

    def add(self, batch, ic_recon, xyz_recon, n_atoms):
        xyz = batch["nxyz"][:, 1:].clone()
        xr = xyz_recon.reshape(-1, 3).clone()
        mask_xyz = batch["mask_xyz_list"]
        xyz[mask_xyz] *= 0                                   # test.py:585-586
        xr[mask_xyz] *= 0
        r = metrics.all_results(ic_recon, batch["ic"], batch["mask"], xr, xyz, batch["bond_edge_list"], batch["nbr_list"],
                                batch["bb_NO_list"], batch["interaction_list"], batch["pi_pi_list"])
        _hv, av, _hg, ag = metrics.valid_ratio_and_cut_off_result(xyz, xr, batch["num_atoms"], batch["nxyz"][:, 0].cpu())
        self.rows.append({k: float(v) for k, v in r.items()})
        self.valid += av
        self.ged += ag
        a, b = xr.reshape(-1, n_atoms, 3), xyz.reshape(-1, n_atoms, 3)
        self.rmsd.append((a - b).pow(2).sum(-1).mean(-1).sqrt().mean().item())      # unaligned all-atom RMSD, test.py:661
        self.recon.append(a)                                 # stay on the device: report superposes them there
        self.true = b

    def report(self, name, args):
        mean = lambda k: float(np.mean([r[k] for r in self.rows]))  # noqa: E731
        stats = {"data_name": name, "data_type": args.data_type, "num_ensemble": args.num_ensemble,
                 "experiment": args.experiment, "test_all_recon": float(np.mean(self.rmsd)),
                 "test_xyz": mean("loss_xyz"), "test_graph": mean("loss_graph"), "test_nbr": mean("loss_nbr"),
                 "test_inter": mean("loss_inter"), "test_pi_pi": mean("loss_pi_pi"),
                 "test_all_valid_ratio": float(np.mean(self.valid)), "test_all_ged": float(np.mean(self.ged)),
                 "diversity": metrics.compute_div(self.recon, self.true) if len(self.recon) > 1 else 0}
        print_frame("result test_stats:", (), stats, "result test_stats:")
        return stats


CA_CONTACT_CUTOFF = 8.0            # A: the usual CA contact definition of --observables


def observables(xyz, top, n_points):
    """--observables for the structures xyz [S, n_atoms, 3] (device) of the topology `top` -> dict of device tensors:
    sasa (metrics.sasa's dict), rg float64 [S], contacts (metrics.contact_map's dict over the CA atoms)."""
    ca = top.select("CA")
    if not len(ca):
        raise SystemExit("--observables: the topology has no CA atoms")
    return dict(sasa=metrics.sasa(xyz, top, n_points=n_points), rg=metrics.radius_of_gyration(xyz),
                contacts=metrics.contact_map(xyz, sel=ca, cutoff=CA_CONTACT_CUTOFF))


def saxs_hydrated(xyz, top, q, hydration, data=None):
    """--saxs_hydration: metrics.saxs_partials of the written structures, (c1, c2) as given or fitted to `data` on the
    ensemble-mean partials (metrics.saxs_hydration_fit, the default grid) -> saxs_profile's dict with the hydrated
    profiles of every structure at those parameters, and `partials`, `hydration` = what saxs_report prints."""
    hp = metrics.saxs_partials(xyz, top, q=q)
    info = {}
    if hydration:
        c1, c2 = hydration
    else:
        fit = metrics.saxs_hydration_fit(hp["mean"], hp["q"], hp["water"], data[1], data[2])
        if int(fit["index"]) < 0:
            raise SystemExit("--saxs_hydration: no point of the (c1, c2) grid has a finite chi^2 (is any structure finite?)")
        c1, c2 = float(fit["c1"]), float(fit["c2"])
        plain = metrics.saxs_fit(hp["mean"][0], data[0], data[1], data[2])
        info = {"saxs_scale": float(fit["scale"]), "saxs_chi2": float(fit["chi2"]), "saxs_chi2_unhydrated": float(plain["chi2"])}
    info = {"saxs_c1": c1, "saxs_c2": c2, **info}
    combine = lambda P: metrics.saxs_combine(P, hp["q"], hp["water"], c1, c2)                    # noqa: E731
    return dict(q=hp["q"], I=combine(hp["P"]), mean=combine(hp["mean"]), finite=hp["finite"], n_finite=hp["n_finite"],
                partials=hp["P"], hydration=info)


def ca_indices(topology):
    """Positions of the CA atoms among the written atoms of a (residue names, atom names per residue) topology (the
    flanking residues are not written, protein_module.write_pdb)."""
    idx, serial = [], 0
    for present in topology[1][1:-1]:
        for a in present:
            if a == "CA":
                idx.append(serial)
            serial += 1
    return idx


def superpose_models(xyz, mode, ref=None, sel=None):
    """--superpose: the ensemble xyz [E, B, n_atoms, 3] (device) with every model moved rigidly onto model 0 of its frame's
    ensemble ("first", model 0 itself is left as it is) or onto the true structure ref [B, n_atoms, 3] ("ref"); the fit uses
    the atoms `sel` (default: all), all atoms move.  "none" returns xyz itself."""
    if mode == "none":
        return xyz
    E, B, n = xyz.shape[:3]
    if mode == "first":
        if E == 1:
            return xyz
        moved = metrics.superpose(xyz[1:].reshape(-1, n, 3), xyz[0].repeat(E - 1, 1, 1), sel=sel)
        return torch.cat((xyz[:1], moved.reshape(E - 1, B, n, 3).to(xyz.dtype)))
    if mode != "ref":
        raise ValueError(f"--superpose must be none, first or ref, not {mode!r}")
    if ref is None:
        raise ValueError("--superpose ref needs the true coordinates of the batch (nxyz): this input has none")
    ref = ref.reshape(B, n, 3)
    return metrics.superpose(xyz.reshape(-1, n, 3), ref.repeat(E, 1, 1), sel=sel).reshape(E, B, n, 3).to(xyz.dtype)


def print_frame(opening, headline, stats, closing):
    """One printed report: the opening title, the headline lines, every statistic on a line of its own, the closing title."""
    print(f"############## vvvvvvvvv {opening}")
    for line in headline:
        print(line)
    for k, v in stats.items():
        print(k, v)
    print(f"############## ^^^^^^^^^ {closing}")


def save_arrays(save_dir, name, files):
    """<save_dir>/<name>_<suffix>.npy for every (suffix, device tensor or array) of `files`; None is not written."""
    for suffix, a in files:
        if a is not None:
            np.save(os.path.join(save_dir, f"{name}_{suffix}.npy"), a.cpu().numpy() if torch.is_tensor(a) else a)


def positive(v):
    return bool(np.isfinite(v) and v > 0)


class Written:
    """The coordinates one batch writes, as the rows of ANALYSES read them."""

    def __init__(self, args, name, batch, xyz, saxs_data):
        self.args, self.name, self.batch, self.saxs_data = args, name, batch, saxs_data
        self.xyz = xyz                                           # [E, B, n_atoms, 3]
        self.n_atoms = xyz.shape[2]
        self.pool = xyz.reshape(-1, self.n_atoms, 3)             # [E * B, n_atoms, 3]: members x frames, one pool

    def ca(self):
        """The CA atoms among the written ones, None where the input route does not name the atoms."""
        return ca_indices(_TOPOLOGY[self.name]) if self.name in _TOPOLOGY else None

    def truth(self, flag):
        return compare_truth(self.name, self.batch, flag).reshape(-1, self.n_atoms, 3)


class Analysis:
    """One analysis of the written coordinates: everything the script knows about it.  The class attributes say which flag
    it belongs to and what it needs of the input route; from them follow its scope refusals (refuse_out_of_scope), whether
    the synthetic route builds a Topology and the true atoms (iter_batches) and the per-file refusal where the topology is
    not known (topology_of)."""
    flag = None              # "--geometry_check": args.geometry_check holds its value
    does = None              # the verb of its scope refusals
    topology = None          # REQUIRED, USED (when the input route knows one) or None
    late = False             # True: the check lets the pickle route pass, topology_of refuses it file by file
    truth = False            # True: it reads the true frames of the batch
    takes = None             # (what a value must be, in the refusal's words; value -> bool)
    off = False              # what the check leaves in args, and returns, when the flag was not given
    writes = ()              # (file suffix, result -> device tensor, array or None = not this time): <name>_<suffix>.npy

    def value(self, args):
        """What the command line gave: the one place that puts up with a namespace that lacks the attribute."""
        return getattr(args, self.flag[2:], None)

    def on(self, args):
        return bool(self.value(args))

    def check(self, args):
        """Refuses a value out of range and a run it does not apply to; normalises args.<flag> and returns it."""
        v = self.value(args)
        if v is None or v is False:
            setattr(args, self.flag[2:], self.off)
            return self.off
        if self.takes and not self.takes[1](v):
            raise SystemExit(f"{self.flag} takes {self.takes[0]}, got {v}")
        refuse_out_of_scope(args, self)
        return v

    def run(self, w, top):
        """Launches the analysis on w.pool (top: topology_of's answer) -> its result dict, still on the device."""
        raise NotImplementedError

    def report(self, w, res):
        """-> print_frame's arguments: opening title, headline lines, statistics, closing title."""
        raise NotImplementedError

    def extras(self, w, res, save_dir):
        """What follows the report, outside the timed span."""


class Relax(Analysis):
    """--relax N is no row of ANALYSES: it changes the coordinates the rows read (relax_structures).  It is allowed exactly
    where a row that requires the topology is, so its check is a row's; 0 = off."""
    flag, does, topology, off = "--relax", "relaxes generated structures", REQUIRED, 0
    takes = "a number of iterations >= 0", lambda n: n >= 0


class Geometry(Analysis):
    """--geometry_check: every member of every frame against the template bond graph, one launch."""
    flag, does, topology = "--geometry_check", "judges generated structures", REQUIRED
    check = staticmethod(check_cg_input)                         # implied by --cg_pdb: the input route's check holds it
    writes = (("geometry", lambda geo: geo["counts"]),           # [E * B, 5]
              ("geometry_min", lambda geo: geo["min_dist"]))

    def run(self, w, top):
        return metrics.geometry_check(w.pool, top, order=w.args.edgeorder, near_dist=w.args.atom_cutoff)

    def report(self, w, geo):
        c = geo["counts"].to(torch.float64)
        near = c[:, 3]
        ratio = torch.where(near > 0, c[:, 4] / near.clamp(min=1), torch.zeros_like(near))
        stats = {"data_name": w.name, "structures": int(c.shape[0]), "atoms": int(w.n_atoms),
                 "geometry_valid_ratio": float(geo["valid"].to(torch.float64).mean()),          # non-finite ones are not valid
                 "geometry_non_finite": int(torch.isnan(geo["min_dist"]).sum()),
                 "geometry_broken_bonds": float(c[:, 0].mean()), "geometry_spurious_bonds": float(c[:, 1].mean()),
                 "geometry_clashes": float(c[:, 4].mean()), "geometry_clash_over_near": float(ratio.mean()),
                 "geometry_min_dist": float(geo["min_dist"].min())}
        return "geometry check (template topology, no true structure):", (), stats, "geometry check"


class Stereo(Analysis):
    """--stereo_check: what the covalent graph cannot see, one launch."""
    flag, does, topology = "--stereo_check", "judges generated structures", REQUIRED
    writes = (("stereo", lambda ste: ste["counts"]),             # [E * B, 6]
              ("stereo_flags", lambda ste: ste["flags"]),        # [E * B, R]
              ("torsions", lambda ste: ste["values"]))           # [E * B, R, 9]

    def run(self, w, top):
        return metrics.stereo_check(w.pool, top)

    def report(self, w, ste):
        c = ste["counts"].to(torch.int64)
        bad = c.sum(1) - c[:, metrics.STEREO_COUNTS.index("cis_pro")]                # what fails stereo_ok, per structure
        worst = int(bad.argmax())
        stats = {"data_name": w.name, "structures": int(c.shape[0]), "residues": int(ste["flags"].shape[1]),
                 "stereo_ok_ratio": float(ste["stereo_ok"].to(torch.float64).mean())}
        stats.update({f"stereo_total_{k}": int(c[:, i].sum()) for i, k in enumerate(metrics.STEREO_COUNTS)})
        stats["stereo_worst_structure"] = worst
        stats["stereo_worst_counts"] = " ".join(f"{k}={int(c[worst, i])}" for i, k in enumerate(metrics.STEREO_COUNTS))
        return "stereo check (chirality, peptide bonds; geometry, not accuracy):", (), stats, "stereo check"


class Observables(Analysis):
    """--observables N_POINTS: SASA with N_POINTS test points per atom, Rg, CA contacts; 0 = off."""
    flag, does, topology, off = "--observables", "describes generated structures", REQUIRED, 0
    takes = f"a number of test points per atom in 1 .. {metrics.SASA_MAX_POINTS}", lambda n: 1 <= n <= metrics.SASA_MAX_POINTS
    writes = (("sasa_residue", lambda obs: obs["sasa"]["residue"]),          # [E * B, R]
              ("rg", lambda obs: obs["rg"]),                                 # [E * B]
              ("ca_contacts", lambda obs: obs["contacts"]["frequency"]))     # [R, R]

    def run(self, w, top):
        return observables(w.pool, top, w.args.observables)

    def report(self, w, obs):
        def mean_sd(t):
            t = t.to(torch.float64)
            return float(t.mean()), float(t.std(unbiased=False))

        fin = obs["sasa"]["finite"]
        stats = {"data_name": w.name, "structures": int(fin.shape[0]), "observables_non_finite": int((~fin).sum())}
        for key, t in (("rg", obs["rg"]), ("sasa_total", obs["sasa"]["total"])):
            t = t[fin]
            stats[f"{key}_mean"], stats[f"{key}_sd"] = mean_sd(t) if t.numel() else (float("nan"), float("nan"))
        freq = obs["contacts"]["frequency"]
        stats["ca_contacts_per_residue"] = float(freq.sum() / freq.shape[0])
        line = f"Rg {stats['rg_mean']:.3f} +- {stats['rg_sd']:.3f}   SASA {stats['sasa_total_mean']:.1f} +- {stats['sasa_total_sd']:.1f}"
        return "ensemble observables (SASA in A^2, Rg in A, CA contacts at 8 A):", (line,), stats, "ensemble observables"


class Saxs(Analysis):
    """--saxs N_Q: the Debye profile of every structure on N_Q points, or on the q grid of --saxs_data; 0 = off.  With
    --saxs_hydration the hydrated profiles; --saxs_reweight follows the report, outside the timed span."""
    flag, does, topology, off = "--saxs", "describes generated structures", REQUIRED, 0
    takes = f"a number of q values in 1 .. {metrics.SAXS_MAX_Q}", lambda n: 1 <= n <= metrics.SAXS_MAX_Q
    writes = (("saxs", lambda sx: sx["I"]),                              # float64 [E * B, N_Q]
              ("saxs_q", lambda sx: sx["q"]),                            # float32 [N_Q]
              ("saxs_partials", lambda sx: sx.get("partials")),          # float64 [E * B, 6, N_Q]
              ("saxs_weights", lambda sx: sx.get("weights")),            # float64 [n_theta, E * B]
              ("saxs_reweighted", lambda sx: sx.get("reweighted")))      # float64 [n_theta, N_Q]

    def check(self, args):
        if self.value(args) is None and getattr(args, "saxs_data", None):
            raise SystemExit("--saxs_data needs --saxs: the curve is compared with the profile --saxs computes")
        return super().check(args)

    def run(self, w, top):
        q = w.saxs_data[0] if w.saxs_data is not None else np.linspace(0.0, 0.5, w.args.saxs)
        if w.args.saxs_hydration is not None:
            return saxs_hydrated(w.pool, top, q, w.args.saxs_hydration, w.saxs_data)
        return metrics.saxs_profile(w.pool, top, q=q)

    def report(self, w, sx):
        q, mean = sx["q"].cpu().numpy(), sx["mean"].cpu().numpy()
        fin, data = sx["finite"], w.saxs_data
        stats = {"data_name": w.name, "structures": int(fin.shape[0]), "saxs_non_finite": int((~fin).sum()), "saxs_I0": float(mean[0])}
        picks = sorted({len(q) // 4, len(q) // 2, len(q) - 1})
        for k in picks:
            stats[f"saxs_mean_q{float(q[k]):.4f}"] = float(mean[k])
        if data is not None and "saxs_scale" not in sx.get("hydration", {}):
            fit = metrics.saxs_fit(sx["mean"], data[0], data[1], data[2])
            stats["saxs_scale"], stats["saxs_chi2"] = float(fit["scale"]), float(fit["chi2"])
        stats.update(sx.get("hydration", {}))
        line = f"I({float(q[0]):.4f}) {stats['saxs_I0']:.6g}   " + "   ".join(f"I({float(q[k]):.4f}) {float(mean[k]):.6g}" for k in picks)
        return "SAXS profile (Debye sum, ensemble mean; q in 1/A):", (line,), stats, "SAXS profile"

    def extras(self, w, sx, save_dir):
        """--saxs_reweight: metrics.saxs_reweight of the profiles sx["I"] (hydrated under --saxs_hydration) against the curve
        at every theta; prints the L-curve (chi^2 before and after, phi_eff, scale, status per theta) and leaves the weights
        [n_theta, S] and the reweighted mean profiles [n_theta, N_Q] in sx."""
        thetas, data = w.args.saxs_reweight, w.saxs_data
        if not thetas:
            return
        rw = metrics.saxs_reweight(sx["I"], data[0], data[1], data[2], list(thetas), finite=sx["finite"])
        col = {k: rw[k].cpu().numpy() for k in ("chi2_prior", "chi2", "phi_eff", "scale", "status", "n_iter", "rounds", "scale_converged")}
        lines = []
        for t, theta in enumerate(thetas):
            status = metrics.REWEIGHT_STATUS[int(col["status"][t])] + ("" if col["scale_converged"][t] else ", scale not converged")
            lines.append(f"theta {theta:g}   chi2 {col['chi2_prior'][t]:.6g} -> {col['chi2'][t]:.6g}   phi_eff {col['phi_eff'][t]:.4f}   "
                         f"scale {col['scale'][t]:.6g}   {status} ({int(col['n_iter'][t])} Newton steps, {int(col['rounds'][t])} rounds)")
        print_frame("SAXS reweighting (maximum entropy; chi^2 at the fitted scale, before -> after):", lines, {}, "SAXS reweighting")
        sx["weights"], sx["reweighted"] = rw["w"].cpu().numpy(), rw["mean"].cpu().numpy()


class PairDistribution(Analysis):
    """--pr DR: the typed pair-distance histogram in bins of DR A; 0 = off."""
    flag, does, topology, off = "--pr", "describes generated structures", REQUIRED, 0.0
    takes = "a bin width in A, a positive number", positive
    writes = (("pr", lambda pr: pr["P"]),                                # float64 [E * B, BINS]
              ("pr_r", lambda pr: pr["r"]))                              # float64 [BINS]

    def run(self, w, top):
        try:
            return metrics.pair_distribution(w.pool, top, dr=w.args.pr)
        except ValueError as e:                               # more bins than the kernel holds: a wider bin is the way out
            raise SystemExit(f"--pr {w.args.pr}: {e}") from None

    def report(self, w, pr):
        fin = pr["finite"]
        d_max, rg = pr["d_max"][fin].cpu().numpy(), pr["rg"][fin].cpu().numpy()
        msd = lambda v: (float(v.mean()), float(v.std())) if v.size else (float("nan"), float("nan"))    # noqa: E731
        stats = {"data_name": w.name, "structures": int(fin.shape[0]), "pr_non_finite": int((~fin).sum()),
                 "pr_overflow": int(pr["overflow"].sum()), "pr_bins": int(pr["r"].shape[0]),
                 "pr_d_max_mean": msd(d_max)[0], "pr_d_max_sd": msd(d_max)[1], "pr_rg_mean": msd(rg)[0], "pr_rg_sd": msd(rg)[1]}
        line = (f"D_max {stats['pr_d_max_mean']:.2f} +- {stats['pr_d_max_sd']:.2f}   Rg {stats['pr_rg_mean']:.3f} +- "
                f"{stats['pr_rg_sd']:.3f}   structures with overflow {stats['pr_overflow']}")
        return "pair distribution P(r) (typed pair-distance histogram; A):", (line,), stats, "pair distribution P(r)"


class Cluster(Analysis):
    """--cluster CUTOFF: Daura / GROMOS clusters at the RMSD CUTOFF in A over --cluster_atoms; 0 = off."""
    flag, does, off = "--cluster", "describes generated structures", 0.0
    takes = "an RMSD cut-off in A, a positive number", positive
    writes = (("cluster_labels", lambda cl: cl["labels"]),               # int32 [E * B], -1 = not finite
              ("cluster_centres", lambda cl: cl["centres"]),             # int32 [K]: indices into the pool
              ("cluster_sizes", lambda cl: cl["sizes"]))                 # int32 [K]

    def run(self, w, top):
        sel = None
        if w.args.cluster_atoms == "ca":
            sel = w.ca()
            if not sel:
                raise SystemExit(f"--cluster: the CA atoms of {w.name} are not known on this input route (use --cluster_atoms all)")
        return metrics.cluster(w.pool, w.args.cluster, sel=sel)

    def report(self, w, cl):
        pop = cl["populations"].cpu().numpy()
        cr = cl["centre_rmsd"][cl["labels"] >= 0]
        stats = {"data_name": w.name, "structures": int(cl["labels"].shape[0]), "cluster_non_finite": int((cl["labels"] < 0).sum()),
                 "clusters": int(cl["n_clusters"]), "cluster_top5_share": float(pop[:5].sum()) if pop.size else float("nan"),
                 "cluster_centre_rmsd_mean": float(cr.mean()) if cr.numel() else float("nan")}
        line = (f"{stats['clusters']} clusters of {stats['structures']} structures   share of the largest five "
                f"{stats['cluster_top5_share']:.3f}   mean RMSD to the centre {stats['cluster_centre_rmsd_mean']:.3f}")
        return "clustering (Daura / GROMOS; RMSD in A):", (line,), stats, "clustering"

    def extras(self, w, cl, save_dir):
        if w.args.save_pdb and w.name in _TOPOLOGY and cl["n_clusters"]:
            from codlad_amd.utils.protein_module import write_pdb
            centres = w.pool[cl["centres"].to(torch.int64)].cpu().numpy()
            write_pdb(os.path.join(save_dir, f"cluster_centres_{w.name}.pdb"), centres, *_TOPOLOGY[w.name])


class Pca(Analysis):
    """--pca K: mean structure, RMSF and the K largest principal components over --pca_atoms; 0 = off."""
    flag, does, off = "--pca", "describes generated structures", 0
    takes = "the number of components, 1 .. 64", lambda k: 1 <= k <= 64
    writes = (("pca_mean", lambda pc: pc["mean"]),                       # float64 [m, 3]
              ("pca_eigenvalues", lambda pc: pc["eigenvalues"]),         # float64 [K], descending
              ("pca_components", lambda pc: pc["components"]),           # float64 [K, m, 3]
              ("pca_projections", lambda pc: pc["projections"]),         # float64 [E * B, K]
              ("rmsf", lambda pc: pc["rmsf"]))                           # float64 [m]

    def run(self, w, top):
        sel = pca_selection(w.name, w.n_atoms, w.args.pca_atoms, w.ca())
        pc = metrics.pca(w.pool, n_components=min(w.args.pca, 3 * (len(sel) if sel else w.n_atoms)), sel=sel)
        return dict(pc, sel=sel)

    def report(self, w, pc):
        ex = pc["explained"].cpu().numpy()
        fl = pc["rmsf"].cpu().numpy()
        stats = {"data_name": w.name, "structures": int(pc["finite"].shape[0]), "pca_non_finite": int((~pc["finite"]).sum()),
                 "pca_fit_iterations": int(pc["n_iter"]), "pca_fit_status": pc["status"], "pca_eig_iterations": int(pc["eig_iter"]),
                 "pca_eig_status": pc["eig_status"], "pca_total_variance": float(pc["total_variance"]),
                 "pca_explained_first3": [float(v) for v in ex[:3]], "rmsf_mean": float(fl.mean()), "rmsf_max": float(fl.max())}
        line = (f"fit in {stats['pca_fit_iterations']} iterations ({stats['pca_fit_status']})   total variance "
                f"{stats['pca_total_variance']:.3f}   explained by the first three " +
                " ".join(f"{v:.3f}" for v in stats["pca_explained_first3"]) +
                f"   RMSF mean {stats['rmsf_mean']:.3f} max {stats['rmsf_max']:.3f}")
        return "essential dynamics (mean structure, RMSF, PCA; A and A^2):", (line,), stats, "essential dynamics"

    def extras(self, w, pc, save_dir):
        if w.args.save_pdb and w.name in _TOPOLOGY and pc["sel"] is None:
            from codlad_amd.utils.protein_module import write_pdb
            write_pdb(os.path.join(save_dir, f"pca_mean_{w.name}.pdb"), pc["mean"].cpu().numpy()[None].astype(np.float32),
                      *_TOPOLOGY[w.name])


class Compare(Analysis):
    """--compare N_BINS: the written structures as one ensemble against the file's true frames; the torsions only where
    the topology is known and the batch masks no atom; --compare_cluster CUTOFF adds the cluster populations; 0 = off."""
    flag, does, topology, truth, off = "--compare", "compares generated structures with the true ones", USED, True, 0
    takes = f"the number of distance bins, 1 .. {metrics.COMPARE_MAX_BINS}", lambda k: 1 <= k <= metrics.COMPARE_MAX_BINS
    writes = (("compare_js_dist", lambda cmp: cmp["js_dist"]),               # float64 [R, R]
              ("compare_js_torsion", lambda cmp: cmp.get("js_torsion")))     # float64 [R, 7]

    def check(self, args):
        c = getattr(args, "compare_cluster", None)
        if c is not None and not positive(c):
            raise SystemExit(f"--compare_cluster takes an RMSD cut-off in A, a positive number, got {c}")
        if c is not None and self.value(args) is None:
            raise SystemExit("--compare_cluster needs --compare")
        return super().check(args)

    def run(self, w, top):
        truth = w.truth("--compare")
        sel = w.ca()
        if not sel or len(sel) < 2:
            raise SystemExit(f"--compare: the CA atoms of {w.name} are not known on this input route")
        top = top if top is not None and compare_no_atom_masked(w.batch) else None
        return metrics.ensemble_compare(w.pool, truth, top=top, sel=sel, n_bins=w.args.compare, cluster_cutoff=w.args.compare_cluster)

    def report(self, w, cmp):
        stats = {"data_name": w.name, "compare_generated": cmp["n_a"], "compare_true": cmp["n_b"], "compare_r_max": cmp["r_max"],
                 "compare_js_dist_mean": float(cmp["js_dist_mean"]), "compare_js_dist_median": float(cmp["js_dist_median"]),
                 "compare_js_rg": float(cmp["js_rg"]), "compare_w1_rg": float(cmp["w1_rg"])}
        line = (f"compare {w.name}: distance JS mean {stats['compare_js_dist_mean']:.4f} median {stats['compare_js_dist_median']:.4f}   "
                f"Rg JS {stats['compare_js_rg']:.4f} W1 {stats['compare_w1_rg']:.3f} A")
        if "js_torsion_mean" in cmp:
            per = [float(v) for v in cmp["js_torsion_mean"].cpu()]
            stats.update({f"compare_js_{n}": v for n, v in zip(metrics.TORSION_NAMES, per)})
            line += "   torsion JS " + " ".join(f"{n} {v:.4f}" for n, v in zip(metrics.TORSION_NAMES, per))
        else:
            line += "   torsions skipped (the topology is not known, or the batch masks atoms)"
        if "js_cluster" in cmp:
            stats.update(compare_js_cluster=float(cmp["js_cluster"]), compare_clusters=cmp["n_clusters"])
            line += f"   cluster JS {stats['compare_js_cluster']:.4f} ({cmp['n_clusters']} clusters)"
        return ("generated against true ensemble (Jensen-Shannon divergences in bits, 0 = same distribution):", (line,), stats,
                "generated against true ensemble")


class Lddt(Analysis):
    """--lddt: member k of frame f against true frame f; atoms the batch masks in a frame take no part."""
    flag, does, topology, truth = "--lddt", "scores generated structures against the true ones", REQUIRED, True
    late = True                                                          # as ever
    writes = (("lddt", lambda ld: ld["global"]),                         # float64 [E * B]
              ("lddt_residue", lambda ld: ld["residue"]))                # float64 [E * B, R]

    def run(self, w, top):
        truth = w.truth("--lddt")
        return metrics.lddt(w.pool, truth, top, ref_index=torch.arange(truth.shape[0]).repeat(w.xyz.shape[0]),
                            sel=lddt_selection(w.batch, truth.shape[0], w.n_atoms))

    def report(self, w, ld):
        g, res = ld["global"].cpu().numpy(), ld["residue"].cpu().numpy()
        scored = res[~np.isnan(res)]
        stats = {"data_name": w.name, "lddt_mean": float(np.nanmean(g)), "lddt_median": float(np.nanmedian(g)), "lddt_min": float(np.nanmin(g)),
                 "lddt_residues_below_0.7": float((scored < 0.7).mean()) if scored.size else float("nan"),
                 "lddt_swapped_residues": int(ld["swapped"].sum()), "lddt_not_finite": int((~ld["finite"]).sum())}
        line = (f"lddt {w.name}: global mean {stats['lddt_mean']:.4f} median {stats['lddt_median']:.4f} min {stats['lddt_min']:.4f}   "
                f"residues below 0.7: {100.0 * stats['lddt_residues_below_0.7']:.1f} %   swapped symmetric residues: "
                f"{stats['lddt_swapped_residues']}")
        return "lDDT of the generated structures against their true frames (1 = every local distance kept):", (line,), stats, "lDDT"


class Dssp(Analysis):
    """--dssp: the DSSP state of every residue of every structure, and the share of each state per residue."""
    flag, does, topology = "--dssp", "describes generated structures", REQUIRED
    writes = (("dssp", lambda sec: sec["ss"]),                           # uint8 [E * B, R]
              ("dssp_propensity", lambda sec: sec["propensity"]))        # float64 [R, 8]

    def run(self, w, top):
        sec = metrics.dssp(w.pool, top)
        return dict(sec, propensity=metrics.ss_propensity(sec["ss"]))

    def report(self, w, sec):
        """The mean share of helix (H + G + I), strand (E + B) and coil (the rest) over residues and finite structures."""
        fin = sec["finite"]
        stats = {"data_name": w.name, "structures": int(fin.shape[0]), "dssp_non_finite": int((~fin).sum())}
        share = sec["propensity"].mean(dim=0)                                       # [8]: NaN when no structure is finite
        codes = {c: i for i, c in enumerate(metrics.DSSP_CODES)}
        stats["helix"] = float(share[codes["H"]] + share[codes["G"]] + share[codes["I"]])
        stats["strand"] = float(share[codes["E"]] + share[codes["B"]])
        stats["coil"] = float(share[codes[" "]] + share[codes["T"]] + share[codes["S"]])
        line = f"helix {stats['helix']:.3f}   strand {stats['strand']:.3f}   coil {stats['coil']:.3f}"
        return "secondary structure (DSSP, mean share of residues):", (line,), stats, "secondary structure"


RELAX = Relax()
GEOMETRY, STEREO, OBSERVABLES, SAXS, PR = Geometry(), Stereo(), Observables(), Saxs(), PairDistribution()
CLUSTER, PCA, COMPARE, LDDT, DSSP = Cluster(), Pca(), Compare(), Lddt(), Dssp()
# the order of the launches before a batch's synchronisation, and of what is written and printed after it
ANALYSES = (GEOMETRY, STEREO, OBSERVABLES, SAXS, PR, CLUSTER, PCA, COMPARE, LDDT, DSSP)

# the checks by the names they have always had (check_cg_input is --geometry_check's)
check_stereo, check_relax, check_observables, check_saxs, check_pr = STEREO.check, RELAX.check, OBSERVABLES.check, SAXS.check, PR.check
check_cluster, check_pca, check_compare, check_dssp = CLUSTER.check, PCA.check, COMPARE.check, DSSP.check


def check_lddt(args):
    """--lddt's check; nothing to return, the flag has no value."""
    LDDT.check(args)


def check_args(args):
    """Every refusal that needs no GPU, before anything is loaded.  The order decides which refusal a command line with two
    faults gets; it is the run order but for --relax, which stands third."""
    check_cg_input(args)
    for check in (check_stereo, check_relax, check_observables, check_saxs, check_saxs_hydration, check_saxs_reweight, check_pr,
                  check_cluster, check_pca, check_compare, check_lddt, check_dssp, check_sampler):
        check(args)


def relax_structures(args, name, xyz):
    """--relax: every member of every frame xyz [E, B, n_atoms, 3], each on its own, CAs fixed -> (the relaxed coordinates,
    which everything after sees; metrics.relax's dict with the decoder's coordinates and their geometry check)."""
    top = topology_of(name, RELAX)
    flat = xyz.reshape(-1, xyz.shape[2], 3)
    geo0 = metrics.geometry_check(flat, top, order=args.edgeorder, near_dist=args.atom_cutoff)
    rel = metrics.relax(flat, top, n_iter=args.relax, order=args.edgeorder)
    return rel["xyz"].reshape(xyz.shape), dict(rel, unrelaxed=xyz, geo0=geo0)


def report_relax(w, rel, geo, save_dir):
    """What --relax writes and prints of one output file; geo: --geometry_check's result of the relaxed coordinates when
    that is on, else it is computed here."""
    args, geo0 = w.args, rel["geo0"]
    save_arrays(save_dir, w.name, (("xyz_unrelaxed", rel["unrelaxed"]),
                                   # [E * B, 3] float64: total energy before, after, accepted steps
                                   ("relax", torch.stack((rel["energy0"], rel["energy"], rel["n_accepted"].to(torch.float64)), 1))))
    geo1 = geo if geo is not None else GEOMETRY.run(w, topology_of(w.name, RELAX))
    print(f"relax {w.name}: {args.relax} iterations, {float(rel['n_accepted'].to(torch.float64).mean()):.1f} accepted, "
          f"energy {float(rel['energy0'].mean()):.3f} -> {float(rel['energy'].mean()):.3f}, clashes "
          f"{int(geo0['clash'].sum())} -> {int(geo1['clash'].sum())}, min_dist {float(geo0['min_dist'].min()):.3f} -> "
          f"{float(geo1['min_dist'].min()):.3f}", flush=True)


def unit_generator(args, batch_id, device):
    """The noise source of one batch (a data file's <= 96 frames x num_ensemble members): seeded by the run's seed
    and the batch's position in the data set alone, so a structure is sampled from the same numbers on 1 or 8 GPUs."""
    gen = torch.Generator(device=device)
    gen.manual_seed(args.seed + args.sample_index + batch_id)
    return gen


def run_sampling(model, args, x, mask=None, batch=None):
    """Flow-matching sampling, reference test.py:214-250: integrate dx/dt = model(x, t) from t = 0 (noise) to 1 over
    t_span = linspace(0, 1, --steps) with --method / --atol / --rtol; torchdiffeq.odeint is replaced by
    codlad_amd.diffusion_and_flow.ode.odeint (euler / midpoint / rk4 / dopri5), which runs a ModelVelocity over the HIP
    model fused (the numbers of the step-wise path).  --compute_nfe: the model evaluations of the batch, as the
    reference's NFECount reports them."""
    from codlad_amd.diffusion_and_flow.ode import ModelVelocity, odeint
    t_span = torch.linspace(0, 1, args.steps).to(x.device)
    func = ModelVelocity(model, mask=mask, batch=batch)
    if args.ode_stepwise:           # any callable that is not a ModelVelocity steps through odeint
        func = lambda t, x_in, f=func: f(t, x_in)       # noqa: E731
    traj, stats = odeint(func, x, t_span, rtol=args.rtol, atol=args.atol, method=args.method, return_stats=True)
    if args.compute_nfe:
        print(f"NFE: {stats['n_eval']} model evaluations ({args.method}: {stats['n_accept']} steps accepted, "
              f"{stats['n_reject']} rejected)", flush=True)
    return traj[-1]


def init_distributed(rank, world):
    """One process per GPU under torch.distributed.run: this rank's device, and the process group when there are several
    -> (device, backend)."""
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    backend = os.environ.get("CODLAD_DIST_BACKEND", "nccl")   # "gloo": rehearsal of N > 1 on a one-GPU box
    dev_index = local_rank if backend == "nccl" else local_rank % torch.cuda.device_count()
    torch.cuda.set_device(dev_index)
    device = f"cuda:{dev_index}"
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if backend == "nccl":
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device(device))
        else:
            dist.init_process_group(backend, rank=rank, world_size=world)
    return device, backend


def load_models(args, device, rank, world):
    """The networks the experiment runs -> namespace of vae, model, cvae, diffusion (None where it has none).  Only rank 0
    reads checkpoints; the other ranks receive its weights (reference: one process, test.py:264-286)."""
    nets = types.SimpleNamespace(vae=load_vae(args, device, load=rank == 0), model=None, cvae=None, diffusion=None)
    if args.experiment == "genzprot":
        nets.cvae = load_cvae(args, device, load=rank == 0)
    if args.experiment in ("latent", "bpd", "fmloss"):
        nets.model = load_denoiser(args, device, load=rank == 0)
        if args.model == "diffusion":
            nets.diffusion = create_diffusion(respacing_spec(args), noise_schedule=args.noise_schedule,
                                              predict_xstart=args.predict_xstart,
                                              rescale_learned_sigmas=args.rescale_learned_sigmas,
                                              # reference test.py:297-303
                                              self_condition=hasattr(nets.model, "self_condition") and args.self_condition)
            if args.timestep_spacing == "logsnr" and rank == 0:
                print(f"--timestep_spacing logsnr: {nets.diffusion.num_timesteps} of {args.num_sampling_steps} requested steps kept "
                      "(steps on the same base step merge)", flush=True)
    elif args.experiment not in ("recon", "genzprot"):
        raise NotImplementedError(f"experiment {args.experiment!r}: latent, recon, genzprot, bpd and fmloss are built")
    if world > 1:
        from codlad_amd import parallel
        mods = [m for m in (nets.model, nets.vae, nets.cvae) if m is not None]
        parallel.broadcast_module_state(*mods, src=0)
        # every rank packs the same parameters into its device blobs; prove it (and leave a record of the rank
        # count and backend the collective ran on)
        sums = [m.engine().weights.checksum() for m in mods]
        parallel.verify_checksums(sums, what="weights broadcast from rank 0")
    return nets


def deal_units(args, rank, world, fixed):
    """This rank's batches as (id, output name, batch, info); the id is the batch's position in the data set, the same on
    every world size.  Batches (independent units) are dealt to the ranks longest-first."""
    units = [(g,) + u for g, u in enumerate(iter_batches(args))]
    if world > 1:
        from codlad_amd.parallel import shard_units, unit_cost
        costs = [int(b["num_CGs"].shape[0]) * unit_cost(int(b["num_CGs"][0])) for _g, _n, b, _i in units]
        units = [units[u] for u in shard_units(costs, world)[rank]]
    if fixed is not None:
        short = min(int(b["num_CGs"][0]) for _g, _n, b, _i in units) if units else None
        if short is not None and fixed[-1] > short:
            raise SystemExit(f"--fix_residues: position {fixed[-1]} is out of range (the shortest structure has {short} residues)")
    return units


def encode_latents(args, vae, batch):
    """The frames' own latents: the VQ-VAE encoder on the batch's atoms, un-quantized, normalised as the samples are
    de-normalised before they are decoded."""
    return get_norm_feature(vae.get_latent_wovq(batch)[0], args.vae_type, norm_channel=args.norm,
                            norm_single=args.norm_single, norm_in=True, dataname=args.data_type)


def score_bpd(args, nets, name, batch, mask, gen, save_dir, st):
    """--experiment bpd: the frames' own latents scored by the variational bound over the respaced steps, one fused loop."""
    B, L, diffusion = mask.shape[0], mask.shape[1], nets.diffusion
    x0 = encode_latents(args, nets.vae, batch).contiguous()
    r = diffusion.calc_bpd_loop(nets.model.forward, x0, clip_denoised=False, model_kwargs=dict(y=None, mask=mask, batch=dict(batch)),
                                step_noise=diffusion._draw_noise(x0, generator=gen))
    torch.cuda.synchronize()
    dt = time.time() - st
    save_arrays(save_dir, name, [(f"bpd_{key}", r[key]) for key in ("vb", "mse", "xstart_mse")])   # [N, T], column k = step T-1-k (the IDDPM layout)
    print(f"{name}: {B} frames, L={L}, T={diffusion.num_timesteps}: total_bpd {float(r['total_bpd'].mean()):.6f} "
          f"prior_bpd {float(r['prior_bpd'].mean()):.6e}: {dt:.2f}s ({B / dt:.1f} structures/s)", flush=True)


def score_fmloss(args, nets, name, batch, mask, gen, save_dir, st):
    """--experiment fmloss: the frames' own latents are the data end x1 of the path; the source end x0 and the path's noise
    per time come from the batch's generator; times are the midpoints (k + 0.5) / K, never 0 or 1, where the target
    matcher's flow divides by 1 - t.  One fused sweep."""
    from codlad_amd.diffusion_and_flow.flow import create_flow_matcher
    B, L, K = mask.shape[0], mask.shape[1], fmloss_steps(args)
    ts = [(k + 0.5) / K for k in range(K)]
    x1 = encode_latents(args, nets.vae, batch).contiguous()
    x0 = torch.randn(x1.shape, device=x1.device, dtype=x1.dtype, generator=gen)
    eps = torch.stack([torch.randn(x1.shape, device=x1.device, dtype=x1.dtype, generator=gen) for _ in range(K)])
    r = create_flow_matcher(args.model, args.fm_sigma).loss_sweep(
        nets.model.forward, x0, x1, ts, step_noise=eps, loss_type=args.loss, model_kwargs=dict(y=None, mask=mask, batch=dict(batch)))
    torch.cuda.synchronize()
    dt = time.time() - st
    save_arrays(save_dir, name, [(f"fmloss_{args.loss}", r["per_sample"])])                        # [N, K]
    print(f"{name}: {B} frames, L={L}, K={K}, {args.model} sigma={args.fm_sigma}: mean {args.loss} "
          f"{float(r['loss'].mean()):.6f}: {dt:.2f}s ({B / dt:.1f} structures/s)", flush=True)
    for tv, v in zip(ts, r["loss"].tolist()):
        print(f"  t={tv:.4f} {args.loss} {v:.6f}", flush=True)


def sample_latents(args, nets, batch, mask, gen, fixed):
    """The latents the decoder is handed, [B * E, L, latent]: E ensemble members of every frame = the batch repeated E times
    along the sample axis."""
    B, (n, L) = int(batch["num_CGs"].shape[0]), mask.shape
    E, device = n // B, str(mask.device)
    if args.experiment == "recon":
        # reference test.py:501: the VQ-VAE's own encoder on the batch's atoms, un-quantized (latent_decode
        # quantizes); deterministic, so the E ensemble members of a frame are equal, as in the reference's loop
        return nets.vae.get_latent_wovq(batch)[0].repeat(E, 1, 1)
    if args.experiment == "genzprot":
        # reference test.py:495-498, 559: a sample of the conditional prior per member
        return torch.cat([nets.cvae.get_latent_cg(batch, generator=gen)[0] for _ in range(E)], 0)
    z = torch.randn(n, L, args.latent_size, device=device, generator=gen)
    kwargs = dict(y=None, mask=mask, batch=dict(batch))
    if args.model == "diffusion":
        diffusion, pin = nets.diffusion, None
        if fixed is not None:
            # the VQ-VAE encoder's latents of the batch pin the chosen residues of every ensemble member (a PinLatents
            # denoised_fn: fused into the loop)
            pin = PinLatents(encode_latents(args, nets.vae, batch).repeat(E, 1, 1).contiguous(), fix_residue_mask(fixed, L, n, device))
        if args.sampler == "dpmpp":
            samples = diffusion.dpm_solver_sample_loop(nets.model.forward, z.shape, z, clip_denoised=False, denoised_fn=pin,
                                                       device=device, model_kwargs=kwargs)
        elif args.sampler == "ddim":
            samples = diffusion.ddim_sample_loop(nets.model.forward, z.shape, z, clip_denoised=False, denoised_fn=pin,
                                                 model_kwargs=kwargs, device=device, eta=args.eta,
                                                 step_noise=diffusion._draw_noise(z, generator=gen))
        else:
            samples = diffusion.p_sample_loop(nets.model.forward, z.shape, z, clip_denoised=False, denoised_fn=pin,
                                              model_kwargs=kwargs, device=device, step_noise=diffusion._draw_noise(z, generator=gen))
    else:                                               # --model fm / icfm / otcfm ...: ODE sampling
        samples = run_sampling(nets.model, args, z, mask=mask, batch=kwargs["batch"])
    return get_norm_feature(samples, args.vae_type, norm_channel=args.norm, norm_single=args.norm_single,
                            norm_in=False, dataname=args.data_type)


def decode(args, nets, name, batch, info, samples, mask, save_dir):
    """Latents -> coordinates, member by member -> (xyz [E, B, n_atoms, 3], the Evaluation of the batch or None where the
    input has no true atoms).  --save_codes writes the VQ codes on the way."""
    B, (n, L) = int(batch["num_CGs"].shape[0]), mask.shape
    decoder_model = nets.cvae if args.experiment == "genzprot" else nets.vae
    if args.save_codes and getattr(decoder_model, "quantize", None) is not None:
        # the VQ code of every residue of every member, [B * E, L]: what the decoder is handed (latent_decode quantizes)
        save_arrays(save_dir, name, [("codes", decoder_model.quantize(samples, mask=mask)[1].reshape(n, L))])
    og = batch["OG_CG_nxyz"].reshape(-1, L + 2, 4)
    xyz_all = []
    evaluation = Evaluation() if all(k in batch for k in EVAL_KEYS) else None
    for e in range(n // B):
        _, ic_recon = decoder_model.latent_decode(samples[e * B:(e + 1) * B], mask[:B], batch)
        xyz_all.append(ic_to_xyz(og, ic_recon.reshape(-1, L, 13, 3), info))
        if evaluation is not None:                               # reference test.py:589-594, per ensemble member
            evaluation.add(batch, ic_recon, xyz_all[-1], xyz_all[-1].shape[1])
    return torch.stack(xyz_all), evaluation


def save_trajectory(w, save_dir):
    """--save_pdb: reference test.py:787-796 writes the generated ensemble through mdtraj (.xtc + .pdb); here both directly,
    frames of member 0 first (multi-model PDB in Angstrom, .xtc in nm as the format has it), superposed as --superpose says."""
    from codlad_amd.utils.protein_module import write_pdb
    from codlad_amd.utils.xtc import write_xtc
    mode, topology = w.args.superpose, _TOPOLOGY[w.name]
    if mode == "ref" and "nxyz" not in w.batch:
        raise SystemExit("--superpose ref needs the true coordinates of the batch (nxyz); this input has none: "
                         "use --superpose first")
    out = superpose_models(w.xyz, mode, ref=w.batch["nxyz"][:, 1:] if mode == "ref" else None,
                           sel=(ca_indices(topology) or None) if mode != "none" else None)
    frames = out.reshape(-1, w.n_atoms, 3).cpu().numpy()
    write_pdb(os.path.join(save_dir, f"generated_traj_{w.name}.pdb"), frames, *topology)
    write_xtc(os.path.join(save_dir, f"generated_traj_{w.name}.xtc"), frames)


def main(args):
    check_args(args)
    saxs_data = read_saxs_data(args.saxs_data) if args.saxs_data else None
    if not torch.cuda.is_available():
        raise SystemExit("test.py (codlad_amd) needs an MI355X: there is no CPU path")
    # one process per GPU under torch.distributed.run: every rank samples and decodes its own batches, rank 0 reports the totals
    rank, world = int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1"))
    check_bpd(args, world)
    check_fmloss(args, world)
    device, backend = init_distributed(rank, world)
    torch.set_grad_enabled(False)
    # the global streams are seeded like the reference's (test.py:256) but NOT used for the latents: every batch
    # draws its noise from its own generator (unit_generator), so the numbers a structure gets do not depend on the
    # world size or on which rank the batch was dealt to
    torch.manual_seed(args.seed + args.sample_index)
    np.random.seed(args.seed + args.sample_index)
    if args.cfg_scale > 1.0:
        raise NotImplementedError("cfg_scale > 1 calls model.forward_with_cfg, which the reference model "
                                  "does not define (dead path)")
    fixed = check_fix_residues(args)
    nets = load_models(args, device, rank, world)
    save_dir = f"./logs/generated_samples_{args.sample_index}_{args.model_step}/{args.exp}_{args.data_type}"
    os.makedirs(save_dir, exist_ok=True)
    total, t_all = 0, time.time()
    for g, name, batch, info in deal_units(args, rank, world, fixed):
        gen = unit_generator(args, g, device)
        batch = {k: (v.to(device) if hasattr(v, "to") else v) for k, v in batch.items()}
        B = int(batch["num_CGs"].shape[0])
        L = int(batch["num_CGs"][0])
        E = args.num_ensemble
        st = time.time()
        mask = torch.ones(B * E, L, dtype=torch.bool, device=device)
        if args.experiment in ("bpd", "fmloss"):
            (score_bpd if args.experiment == "bpd" else score_fmloss)(args, nets, name, batch, mask[:B], gen, save_dir, st)
            total += B
            continue
        samples = sample_latents(args, nets, batch, mask, gen, fixed)
        xyz, evaluation = decode(args, nets, name, batch, info, samples, mask, save_dir)
        rel = None
        if args.relax:
            xyz, rel = relax_structures(args, name, xyz)
        w = Written(args, name, batch, xyz, saxs_data)
        # one launch set per row that is on, in table order; everything is read back after the one synchronisation
        results = [(row, row.run(w, topology_of(name, row))) for row in ANALYSES if row.on(args)]
        torch.cuda.synchronize()
        dt = time.time() - st
        total += B * E
        if evaluation is not None:
            evaluation.report(name, args)
        if rel is not None:
            report_relax(w, rel, dict(results).get(GEOMETRY), save_dir)
        save_arrays(save_dir, name, [("xyz_recon", xyz)])
        for row, res in results:
            print_frame(*row.report(w, res))
            row.extras(w, res, save_dir)
            save_arrays(save_dir, name, [(suffix, get(res)) for suffix, get in row.writes])
        if args.save_pdb and name in _TOPOLOGY:
            save_trajectory(w, save_dir)
        print(f"{name}: {B} frames x {E} members, L={L}, {w.n_atoms} atoms: {dt:.2f}s "
              f"({B * E / dt:.1f} structures/s)", flush=True)
    if world > 1:
        import torch.distributed as dist
        tot = torch.tensor([total], dtype=torch.int64, device=device if backend == "nccl" else "cpu")
        dist.all_reduce(tot)
        total = int(tot)
        dist.destroy_process_group()
    if rank == 0:
        print(f"done: {total} structures on {world} GPU(s) in {time.time() - t_all:.1f}s -> {save_dir}")


def build_parser():
    """The command line: names and defaults as in the reference (test.py:894-961), then the additions."""
    p = argparse.ArgumentParser("parameters")
    # names and defaults as in the reference (test.py:894-961)
    p.add_argument("--seed", type=int, default=42)
    p.add_argument("--exp", default="experiment_cifar_default")
    p.add_argument("--cond", action="store_true", default=False)
    p.add_argument("--backbone", type=str, default="mpnn_diffusion")
    p.add_argument("--latent_size", type=int, default=3)
    p.add_argument("--cfg_scale", type=float, default=1.0)
    p.add_argument("--model_step", type=str, default="best")
    p.add_argument("--vae_type", type=str, default="N6")
    p.add_argument("--cvae_type", type=str, default="C2")
    p.add_argument("--model", type=str, default="diffusion")
    p.add_argument("--num_sampling_steps", type=int, default=250)
    p.add_argument("--norm", action="store_true", default=True)
    p.add_argument("--norm_single", action="store_true", default=False)
    p.add_argument("--data_type", type=str, default="PED")
    p.add_argument("--data_process", action="store_true", default=False)
    p.add_argument("--num_ensemble", type=int, default=1)
    p.add_argument("--modelnum", type=int, default=-1)
    p.add_argument("--self_condition", action="store_true", default=False)
    p.add_argument("--predict_xstart", action="store_true", default=False)
    p.add_argument("--rescale_learned_sigmas", action="store_true", default=False)
    p.add_argument("--noise_schedule", type=str, default="linear", choices=["linear", "squaredcos_cap_v2"])
    p.add_argument("--experiment", type=str, default="latent", choices=["genzprot", "recon", "latent", "bpd", "fmloss"])
    p.add_argument("--ckpt_type", type=str, default="net")
    p.add_argument("--sample_index", type=int, default=0)
    p.add_argument("--compute_nfe", action="store_true",
                   help="ODE sampling: print the number of model evaluations of every batch")
    for ignored, kw in (("--iteration", dict(type=int, default=1000)),
                        ("--n_sample", dict(type=int, default=50000)), ("--dataset", dict(default="cifar10")),
                        ("--num_steps", dict(type=int, default=40)), ("--batch_size", dict(type=int, default=200)),
                        ("--feature_path", dict(type=str, default="./datasets/features_N6")),
                        ("--gcn_layernorm", dict(action="store_true", default=True)),
                        ("--forward_inf", dict(action="store_true", default=False))):
        p.add_argument(ignored, **kw)
    p.add_argument("--atol", type=float, default=1e-5)
    p.add_argument("--rtol", type=float, default=1e-5)
    p.add_argument("--method", type=str, default="dopri5")
    p.add_argument("--steps", type=int, default=2)
    # additions
    p.add_argument("--data_files", nargs="*", default=[], help="with --data_process: pickles of (list of frame dicts, info)")
    p.add_argument("--loss", type=str, default="l2", choices=["l2", "l1", "huber", "smooth_l1", "log_cosh"],
                   help="--experiment fmloss: the regression loss reported (the reference's train_latent.py --loss)")
    p.add_argument("--fm_sigma", type=float, default=0.0, help="--experiment fmloss: the matcher's sigma")
    p.add_argument("--synthetic", action="store_true", help="synthetic PED/PDB/Atlas-shaped proteins")
    p.add_argument("--synthetic_frames", type=int, default=10)
    p.add_argument("--synthetic_weights", action="store_true", help="seeded random weights (no checkpoints ship)")
    p.add_argument("--ode_stepwise", action="store_true",
                   help="ODE sampling: one model call per stage from the host instead of the fused loop (same numbers)")
    p.add_argument("--save_pdb", action="store_true", help="also write the generated ensemble as a multi-model PDB and an .xtc trajectory")
    p.add_argument("--superpose", default="none", choices=["none", "first", "ref"],
                   help="with --save_pdb: write the models rigidly superposed on model 0 of the same frame's ensemble (first) or "
                        "on the true structure (ref; needs input with atoms); the fit uses the CA atoms; _xyz_recon.npy is "
                        "never altered")
    p.add_argument("--save_codes", action="store_true", help="also save the VQ code index of every residue, [structures, L] (VQ-VAE decoders)")
    p.add_argument("--pdb_files", nargs="*", default=None,
                   help="multi-model PDB ensembles to build the test set from (the reference's load_dataset, without mdtraj)")
    p.add_argument("--cg_pdb", nargs="+", default=None, metavar="FILE",
                   help="backmap CA-only (coarse-grained) input: multi-model PDB files of which only the CA records are read "
                        "(sequence + CA frames; the atoms written are the residue templates').  The chain loses its first and "
                        "last residue: they supply only the flanking CAs.  --experiment latent only; implies --geometry_check")
    p.add_argument("--cg_xtc", default=None, metavar="FILE",
                   help="with a single --cg_pdb: take the CA frames from this .xtc (one atom per CA of the PDB file, which then "
                        "supplies the sequence only)")
    p.add_argument("--geometry_check", action="store_true",
                   help="judge every generated structure against its template topology, with no true structure (broken and "
                        "spurious covalent bonds, clashes, smallest non-bonded distance): saves <name>_geometry.npy "
                        "[structures, 5] = broken, spurious, bonded, near, clash and <name>_geometry_min.npy, prints a summary. "
                        "'valid' is a statement about geometry, not about accuracy")
    p.add_argument("--stereo_check", action="store_true",
                   help="also judge the stereochemistry of every generated structure (allowed wherever --geometry_check is): "
                        "saves <name>_stereo.npy [structures, 6] = inverted_ca, inverted_side, cis_pro, cis_nonpro, twisted, "
                        "undefined (residues), <name>_stereo_flags.npy [structures, residues] and <name>_torsions.npy "
                        "[structures, residues, 9] = phi, psi, omega, chi1-4 (degrees), v_ca, v_side (A^3); prints a summary. "
                        "Geometry, not accuracy")
    p.add_argument("--relax", nargs="?", type=int, const=200, default=None, metavar="N",
                   help="relax every generated structure before it is checked and written (allowed wherever --geometry_check "
                        "is): N iterations (default 200) of restrained steepest descent on the device push overlapping atoms "
                        "apart, CAs fixed, bonded geometry and rigid torsions held to the decoder's (metrics.relax).  The "
                        "checks, <name>_xyz_recon.npy and --save_pdb see the relaxed coordinates; saves the decoder's as "
                        "<name>_xyz_unrelaxed.npy and <name>_relax.npy [structures, 3] = energy before, after, accepted steps")
    p.add_argument("--observables", nargs="?", type=int, const=960, default=None, metavar="N_POINTS",
                   help="also describe the written ensemble on the device (allowed wherever --geometry_check is; after --relax "
                        "when both are given): solvent-accessible surface area with N_POINTS test points per atom (default "
                        "960; metrics.sasa), radius of gyration, CA contacts at 8 A.  Prints mean +- sd of Rg and of the total "
                        "SASA; saves <name>_sasa_residue.npy [structures, R], <name>_rg.npy [structures] and "
                        "<name>_ca_contacts.npy [R, R] = the fraction of structures with the two CAs closer than 8 A")
    p.add_argument("--saxs", nargs="?", type=int, const=51, default=None, metavar="N_Q",
                   help="also compute the small-angle X-ray scattering profile of every written structure on the device "
                        "(allowed wherever --observables is; after --relax when both are given): the Debye sum over all atom "
                        "pairs with united-atom form factors in a displaced solvent (metrics.saxs_profile) on N_Q points of "
                        "[0, 0.5] 1/A (default 51).  Prints I(0) and the ensemble mean at three q values; saves <name>_saxs.npy "
                        "float64 [structures, N_Q] and <name>_saxs_q.npy")
    p.add_argument("--saxs_data", default=None, metavar="FILE",
                   help="an experimental curve for --saxs: three whitespace-separated columns q (1/A), I, sigma, `#` starts a "
                        "comment.  Its q values replace the grid of --saxs (there is no interpolation); the scale and the "
                        "reduced chi^2 of the ensemble mean against it are printed")
    p.add_argument("--saxs_reweight", nargs="*", type=float, default=None, metavar="THETA",
                   help="with --saxs and --saxs_data: reweight the written structures so that their weighted mean profile agrees "
                        "with the curve while staying close to uniform weights (maximum entropy / BME, metrics.saxs_reweight; the "
                        "scale of the intensities is fitted along), once per THETA: a large THETA keeps the ensemble as it is, a "
                        "small one trusts the data.  Prints chi^2 before and after, the kept share phi_eff, the scale and the "
                        "status per THETA - the L-curve to pick THETA from; saves <name>_saxs_weights.npy float64 [n_theta, "
                        "structures] and <name>_saxs_reweighted.npy [n_theta, N_Q].  With --saxs_hydration the hydrated profiles "
                        "are reweighted")
    p.add_argument("--saxs_hydration", nargs="*", type=float, default=None, metavar="C",
                   help="with --saxs: add the hydration shell and the excluded-volume scale to the profile (metrics.saxs_partials, "
                        "saxs_combine): C1 C2 = the scale of the atomic volumes (1 = as --saxs alone) and the weight of the bound "
                        "water on the solvent-exposed atoms (0 = none).  Without the two numbers both are fitted to --saxs_data on "
                        "FoXS's grid (c1 0.95 .. 1.05, c2 -2 .. 4) for the ensemble mean; c1, c2, the scale and chi^2 are printed "
                        "beside the chi^2 of the unhydrated mean.  <name>_saxs.npy then holds the hydrated profiles; also saves "
                        "<name>_saxs_partials.npy float64 [structures, 6, N_Q] (tt, td, dd, ts, ds, ss)")
    p.add_argument("--pr", nargs="?", type=float, const=0.5, default=None, metavar="DR",
                   help="compute the pair distribution P(r) of every written structure on the device (allowed wherever "
                        "--observables is; after --relax when both are given): the typed pair-distance histogram in bins of DR A "
                        "(default 0.5) up to the contour-length bound of the topology, weighted with the forward amplitudes "
                        "(metrics.pair_distribution).  Prints D_max, the real-space Rg and the number of structures with pairs "
                        "beyond the bound; saves <name>_pr.npy float64 [structures, BINS] and <name>_pr_r.npy (the bin centres)")
    p.add_argument("--cluster", type=float, default=None, metavar="CUTOFF",
                   help="cluster the written structures of every data file, members x frames as one pool, on the device (Daura / "
                        "GROMOS, metrics.cluster; after --relax when both are given): structures within the RMSD CUTOFF in A "
                        "of a centre, after superposition, form its cluster.  Prints the number of clusters, the share of the "
                        "largest five and the mean RMSD to the centre; saves <name>_cluster_labels.npy int32 [structures] "
                        "(-1 = a structure that is not finite), <name>_cluster_centres.npy (indices into the pool) and "
                        "<name>_cluster_sizes.npy; with --save_pdb also cluster_centres_<name>.pdb, one model per centre")
    p.add_argument("--pca", type=int, nargs="?", const=10, default=None, metavar="K",
                   help="essential dynamics of the written structures of every data file, members x frames as one pool, on the "
                        "device (metrics.pca; after --relax when both are given): the mean structure after mutual superposition, "
                        "the RMSF about it and the K (default 10, at most 64) largest principal components of the covariance of "
                        "the superposed coordinates.  Prints the iterations of the fit, the total variance, the share the first "
                        "three components explain and the mean and largest RMSF; saves <name>_pca_mean.npy [m, 3], "
                        "<name>_pca_eigenvalues.npy [K], <name>_pca_components.npy [K, m, 3], <name>_pca_projections.npy "
                        "[structures, K] and <name>_rmsf.npy [m]; with --save_pdb and --pca_atoms all also pca_mean_<name>.pdb")
    p.add_argument("--compare", type=int, nargs="?", const=50, default=None, metavar="N_BINS",
                   help="compare the written structures of every data file, members x frames as one ensemble, with the file's "
                        "true frames on the device (metrics.ensemble_compare; after --relax when both are given): the "
                        "Jensen-Shannon divergence of every CA-CA distance distribution on N_BINS bins (default 50), of Rg and, "
                        "when the topology is known and no atom is masked, of phi, psi, omega and chi1-4 per residue.  Prints one "
                        "line; saves <name>_compare_js_dist.npy [R, R] and <name>_compare_js_torsion.npy [R, 7]")
    p.add_argument("--compare_cluster", type=float, default=None, metavar="CUTOFF",
                   help="with --compare: cluster generated and true structures as one pool at the RMSD CUTOFF in A (CA atoms) and "
                        "print the Jensen-Shannon divergence of the two cluster populations (ENCORE's CES)")
    p.add_argument("--lddt", action="store_true",
                   help="score the written structures of every data file against the file's true frames on the device "
                        "(metrics.lddt; after --relax when both are given): member k of frame f against true frame f, all "
                        "atoms the batch does not mask, symmetric side chains in the better naming; prints the mean / median / "
                        "minimum global lDDT, the share of residues below 0.7 and the number of swapped residues; saves "
                        "<name>_lddt.npy [structures] and <name>_lddt_residue.npy [structures, R]")
    p.add_argument("--pca_atoms", choices=("ca", "all"), default="ca",
                   help="the atoms --pca superposes and analyses: the CA atoms (default) or every written atom (refused when "
                        "3 x atoms > 4096)")
    p.add_argument("--cluster_atoms", choices=("ca", "all"), default="ca",
                   help="the atoms --cluster superposes and measures: the CA atoms (default) or every written atom")
    p.add_argument("--dssp", action="store_true",
                   help="also assign the secondary structure of every written structure on the device (allowed wherever "
                        "--geometry_check is; after --relax when both are given): Kabsch-Sander hydrogen bonds and the DSSP "
                        "states (metrics.dssp).  Prints the mean helix (H+G+I), strand (E+B) and coil shares; saves "
                        "<name>_dssp.npy uint8 [structures, R] (0 .. 7 = ' HBEGITS', 255 = a structure that is not finite) and "
                        "<name>_dssp_propensity.npy float64 [R, 8] = the share of finite structures with each state")
    p.add_argument("--atom_cutoff", type=float, default=9.0)
    p.add_argument("--cg_cutoff", type=float, default=21.0)
    p.add_argument("--edgeorder", type=int, default=2)
    p.add_argument("--fix_residues", default=None, metavar="SPEC",
                   help="keep the latents of these residues (1-based CG positions, flanking caps excluded, e.g. 3-20,41) "
                        "as the VQ-VAE encodes them from the input's atoms and sample the rest conditioned on them "
                        "(--experiment latent --model diffusion, VQ-VAE N6 / K3 / K4)")
    p.add_argument("--sampler", default="ddpm", choices=["ddpm", "ddim", "dpmpp"],
                   help="latent sampler of --model diffusion: the ancestral DDPM loop (default), DDIM or DPM-Solver++(2M) "
                        "(deterministic, multistep; use it with --timestep_spacing logsnr) over the same --num_sampling_steps "
                        "respacing")
    p.add_argument("--timestep_spacing", default="uniform", choices=["uniform", "logsnr"],
                   help="how --num_sampling_steps steps are placed among the base steps: uniformly in t (default, the "
                        "reference's respacing) or uniformly in log-SNR (steps on the same base step merge); --model diffusion only")
    p.add_argument("--eta", type=float, default=0.0,
                   help="DDIM noise scale (0 = the deterministic sampler, 1 = the DDPM posterior variance); --sampler ddim only")
    return p


if __name__ == "__main__":
    main(build_parser().parse_args())
