"""Host-side driver of the HIP sampling path: ragged job tables, workspaces and the calls into
libcodlad_hip.so.  PyTorch is used for device memory and streams only; every computation on the
path is a kernel of the library (there is no CPU or eager fallback).

A *structure* is one CA trace (one frame of one protein); a *sample* is one latent trajectory on a
structure.  Ensemble members of a frame are several samples on the same structure: they share the
k-NN graph and the initial edge embedding h_E0, which is computed once per structure instead of
once per denoiser call as the reference does (reference models/latent_model.py:208).
"""
import ctypes as C
import os

import numpy as np
import torch

from . import _lib
from .weights import DEFAULT_PRECISION, DenoiserWeights, DecoderWeights

H = 128
KNN = 64
MODS = 6016


def _require_cuda(t, what):
    if not t.is_cuda:
        raise RuntimeError(f"{what} must live on the GPU: this path has no CPU implementation")


def edge_rows(blocks, split=False):
    """Edge state as the kernels keep it in HBM ([..., 2 halves, 32 chunks, 32 edges, 4], include/codlad_hip.h)
    -> [..., 64 edges, 128 features].  split: the blocks are h_E0 / h_E of a split-fp16 contraction mode, whose 16-byte
    slots hold fp16 halves (slot 8 b + 4 s + h: the `hi` halves of features 32 b + 16 s + 4 h + {0..3, 8..11}, slot
    8 b + 4 s + 2 + h their `lo` halves); the values returned are hi + lo."""
    lead = blocks.shape[:-4]
    if not split:
        return blocks.permute(*range(len(lead)), -4, -2, -3, -1).reshape(*lead, 64, -1)
    hv = blocks.contiguous().view(torch.float16).view(*lead, 2, 4, 2, 2, 2, 32, 8)      # half, b, s, hi|lo, h, edge, 8
    val = hv[..., 0, :, :, :].float() + hv[..., 1, :, :, :].float()                       # [.., half, b, s, h, edge, 8]
    n = len(lead)
    val = val.permute(*range(n), n, n + 4, n + 1, n + 2, n + 3, n + 5)                    # [.., half, edge, b, s, h, 8]
    out = torch.empty(*lead, 2, 32, 4, 2, 16, dtype=torch.float32, device=blocks.device)  # feature = 32 b + 16 s + (0..15)
    for h in range(2):
        out[..., 4 * h:4 * h + 4] = val[..., h, 0:4]
        out[..., 8 + 4 * h:8 + 4 * h + 4] = val[..., h, 4:8]
    return out.reshape(*lead, 64, 128)


class Structures:
    """Flat structure-node arrays + the step-invariant graph/features of every structure."""

    def __init__(self, xyz_list, z_list, device):
        self.lens = [int(x.shape[0]) for x in xyz_list]
        assert all(L >= 1 for L in self.lens)
        self.offsets = np.concatenate([[0], np.cumsum(self.lens)]).astype(np.int64)
        self.n_snodes = int(self.offsets[-1])
        self.xyz = torch.cat([x.reshape(-1, 3).float() for x in xyz_list]).contiguous().to(device)
        self.z = torch.cat([z.reshape(-1).to(torch.int32) for z in z_list]).contiguous().to(device)
        info = np.empty((self.n_snodes, 2), dtype=np.int32)
        for f, L in enumerate(self.lens):
            info[self.offsets[f]:self.offsets[f + 1], 0] = self.offsets[f]
            info[self.offsets[f]:self.offsets[f + 1], 1] = L
        self.snode_info = torch.from_numpy(info).to(device)
        self.E_idx = None
        self.h_E0 = None
        self.E1 = None        # [2] x edge blocks: hoisted layer-0 edge terms (optional)
        self.features_tag = None   # contraction mode + block exponents E1 was computed with (Denoiser.features_tag)


class Job:
    """Samples on structures: node tables + per-step workspace."""

    def __init__(self, structures, sample_struct, device, edge_state=None):
        """edge_state: a [n_nodes, 64, 128] view to use as this job's edge state instead of a buffer of its own (the
        parts of a split job live in their parent's)."""
        st = structures
        self.structures = st
        self.device = device
        self._parts = {}
        self.sample_struct = [int(s) for s in sample_struct]
        lens = [st.lens[f] for f in self.sample_struct]
        self.sample_lens = lens
        self.sample_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        self.n_nodes = int(self.sample_off[-1])
        info = np.empty((self.n_nodes, 4), dtype=np.int32)
        z_host = st.z.cpu().numpy()
        for s, f in enumerate(self.sample_struct):
            a, b = self.sample_off[s], self.sample_off[s + 1]
            L = lens[s]
            info[a:b, 0] = np.arange(st.offsets[f], st.offsets[f] + L)
            info[a:b, 1] = a
            info[a:b, 2] = min(KNN, L)
            info[a:b, 3] = z_host[st.offsets[f]:st.offsets[f] + L]
        assert info[:, 3].min() >= 0 and info[:, 3].max() < 30, "residue type outside W_s vocabulary"
        self.node_info = torch.from_numpy(info).to(device)
        n = self.n_nodes
        f32 = dict(dtype=torch.float32, device=device)
        self.hV = torch.empty(n, H, **f32)
        self.hVenc = torch.empty(n, H, **f32)
        self.S = torch.empty(4, n, H, **f32)      # planes 1-3: per-half, per-lane-half partial sums of small jobs
        self.PQ = torch.empty(4, n, H, **f32)
        self.hE = torch.empty(n, KNN, H, **f32) if edge_state is None else edge_state
        assert tuple(self.hE.shape) == (n, KNN, H) and self.hE.is_contiguous()
        self.status = torch.zeros(1, dtype=torch.int32, device=device)   # sticky flags (CODLAD_STATUS_*)
        # non-empty 32-edge tiles {node, half}: small jobs deal the edge kernels' work out per tile
        halves = np.where(info[:, 2] > 32, 2, 1)
        tiles = np.empty((int(halves.sum()), 2), dtype=np.int32)
        tiles[:, 0] = np.repeat(np.arange(n, dtype=np.int32), halves)
        first = np.cumsum(halves) - halves
        tiles[:, 1] = np.arange(tiles.shape[0], dtype=np.int32) - np.repeat(first, halves).astype(np.int32)
        self.tile_list = torch.from_numpy(tiles).to(device)
        ws = _lib.Workspace()
        ws.hV, ws.hVenc, ws.S, ws.PQ, ws.hE, ws.status, ws.tile_list = (
            _lib.ptr(t) for t in (self.hV, self.hVenc, self.S, self.PQ, self.hE, self.status, self.tile_list))
        ws.n_tiles = tiles.shape[0]
        # XCD chunks of the per-node edge kernels, balanced by tile cost (paired last tiles, include/codlad_hip.h)
        self.xcd_bounds = torch.from_numpy(_lib.edge_plan(info[:, 2])[0]).to(device)
        ws.xcd_bounds = _lib.ptr(self.xcd_bounds)
        self.ws = ws

    def workspace_bytes(self):
        return 4 * (self.hV.numel() * 2 + self.S.numel() + self.PQ.numel() + self.hE.numel())

    def desc(self):
        """The codlad_job of this job on its structures as they are now (new_structures allocates E_idx / h_E0 / E1 after
        Structures.__init__): build it per engine call.  Every pointer in it belongs to a tensor that this job or its
        structures hold, and it holds the workspace; the caller holds it until the foreign call has returned."""
        st = self.structures
        d = _lib.JobDesc()
        d.node_info, d.n_nodes = _lib.ptr(self.node_info), self.n_nodes
        d.E_idx, d.h_E0, d.E1, d.n_snodes = _lib.ptr(st.E_idx), _lib.ptr(st.h_E0), _lib.ptr(st.E1), st.n_snodes
        d.ws = C.pointer(self.ws)
        return d

    def sub_job(self, members, start):
        """The ragged sub-job of the samples `members` -> (job, node indices of its samples in this job).  It keeps its edge
        state in this job's buffer, from node `start` (32 KB per node: nothing else of a workspace is large; the small
        tables are its own), so a job and its sub-jobs are never in flight together, and sub-jobs that are occupy
        disjoint ranges."""
        n = int(sum(self.sample_lens[m] for m in members))
        sub = Job(self.structures, [self.sample_struct[m] for m in members], self.device,
                  edge_state=self.hE[start:start + n])
        idx = np.concatenate([np.arange(self.sample_off[m], self.sample_off[m + 1]) for m in members])
        return sub, torch.from_numpy(idx).to(self.device)

    def parts(self, k=2):
        """This job's samples dealt alternately into k independent jobs (the same mix of lengths in each) -> [(job, node
        indices of its samples in this job)], sub-jobs side by side in this job's edge state."""
        if k not in self._parts:
            subs, start = [], 0
            for p in range(k):
                subs.append(self.sub_job(range(p, len(self.sample_struct), k), start))
                start += subs[-1][0].n_nodes
            self._parts[k] = subs
        return self._parts[k]


class Denoiser:
    """mpnn_diffusion on the GPU."""

    def __init__(self, state_dict, device, precision=DEFAULT_PRECISION, block_exponents=True, self_condition=False,
                 out_dim=6):
        """state_dict None: the layout of a model with the given flags and NO weights - what a rank that loads no
        checkpoint starts from; `parallel.broadcast_weights(den.weights)` then fills it with rank 0's."""
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("codlad_amd runs on an MI355X only; no CPU path exists")
        self.lib = _lib.lib()
        if state_dict is None:
            self.weights = DenoiserWeights.empty(self.device, self_condition, out_dim, precision)
        else:
            self.weights = DenoiserWeights(state_dict, self.device, precision, block_exponents=block_exponents)
        self._mods_cache = {}
        self._mods_generation = self.weights.generation

    # -- step-invariant part -------------------------------------------------------------------
    def new_structures(self, xyz_list, z_list, hoist_layer0=True):
        """Tables of a set of structures uploaded and the buffers of their step-invariant part
        allocated; `compute_features` fills them (split so that a caller can time the kernels apart
        from the uploads, bench.py)."""
        st = Structures(xyz_list, z_list, self.device)
        st.E_idx = torch.empty(st.n_snodes, KNN, dtype=torch.int32, device=self.device)
        st.h_E0 = torch.empty(st.n_snodes, 2, H // 4, KNN // 2, 4, dtype=torch.float32, device=self.device)
        if hoist_layer0:
            st.E1 = torch.empty(2, st.n_snodes, 2, H // 4, KNN // 2, 4, dtype=torch.float32, device=self.device)
        return st

    def compute_features(self, st):
        """k-NN graph + h_E0 per structure (codlad_features_prepass), and - when the structures were
        made with hoist_layer0 - the two layer-0 contractions of h_E0, which are the same in every
        step and for every ensemble member (costs 2x the h_E0 memory).  Only enqueues kernels."""
        rc = self.lib.codlad_features_prepass(C.byref(self.weights.struct), _lib.ptr(st.xyz),
                                              _lib.ptr(st.snode_info), st.n_snodes, max(st.lens),
                                              _lib.ptr(st.E_idx), _lib.ptr(st.h_E0),
                                              _lib.stream_ptr(self.device))
        _lib.check(rc, "codlad_features_prepass")
        if st.E1 is not None:
            rc = self.lib.codlad_layer0_edge_terms(C.byref(self.weights.struct), _lib.ptr(st.snode_info),
                                                   st.n_snodes, _lib.ptr(st.h_E0), _lib.ptr(st.E1),
                                                   _lib.stream_ptr(self.device))
            _lib.check(rc, "codlad_layer0_edge_terms")
        st.features_tag = self.features_tag()
        return st

    @property
    def split_edge_state(self):
        """True when h_E0 / h_E are kept as fp16 hi / lo halves (the split-fp16 modes), see edge_rows."""
        return self.weights.precision != "f32"

    def features_tag(self):
        """What the hoisted layer-0 terms E1 depend on besides the structure: in the split-fp16 modes they carry
        encoder layer 0's block exponents (E1[0] = 2^e1 W1e h_E0, E1[1] = 2^e11 W11e h_E0), in the fp32 mode none."""
        # generation: h_E0 and E1 are functions of the weights too, so a broadcast (rebind) makes them stale
        if self.weights.precision == "f32":
            return ("f32", self.weights.generation)
        ex = self.weights.exponents["enc0"]
        return ("split", self.weights.precision, ex["e1"], ex["e11"], self.weights.generation)

    def _fresh_features(self, st):
        if st.features_tag != self.features_tag():     # e.g. set_precision() after the structures were prepared
            self.compute_features(st)

    def prepare_structures(self, xyz_list, z_list, hoist_layer0=True):
        return self.compute_features(self.new_structures(xyz_list, z_list, hoist_layer0))

    def make_job(self, structures, sample_struct):
        return Job(structures, sample_struct, self.device)

    def step_mods(self, t_values, refresh=False, as_float=False):
        """[len(t_values), 6016] adaLN modulation vectors; cached per timestep list (refresh: run the
        kernel again even if cached).  Integer timesteps (diffusion) or fractional ones (flow matching: any
        non-integer value switches the whole list to the float entry point; as_float: take it in any case - the rows of
        whole numbers are the same bits through either)."""
        fractional = as_float or any(float(t) != int(t) for t in t_values)
        key = tuple(float(t) for t in t_values) if fractional else tuple(int(t) for t in t_values)
        if self._mods_generation != self.weights.generation:      # the weights changed under the cache (broadcast)
            self._mods_cache.clear()
            self._mods_generation = self.weights.generation
        if refresh or key not in self._mods_cache:
            mods = torch.empty(len(key), MODS, dtype=torch.float32, device=self.device)
            if fractional:
                tv = torch.tensor(key, dtype=torch.float32, device=self.device)
                rc = self.lib.codlad_step_mods_f(C.byref(self.weights.struct), _lib.ptr(tv), len(key),
                                                 _lib.ptr(mods), _lib.stream_ptr(self.device))
            else:
                tv = torch.tensor(key, dtype=torch.int64, device=self.device)
                rc = self.lib.codlad_step_mods(C.byref(self.weights.struct), _lib.ptr(tv), len(key),
                                               _lib.ptr(mods), _lib.stream_ptr(self.device))
            _lib.check(rc, "codlad_step_mods")
            if len(self._mods_cache) > 64:
                self._mods_cache.clear()
            self._mods_cache[key] = mods
        return self._mods_cache[key]

    # -- per call ------------------------------------------------------------------------------
    @property
    def self_condition(self):
        return self.weights.self_condition

    def _run(self, name, desc, *args):
        """lib.<name>(the weights, a Job.desc(), *args, the current stream), its return code checked under that name."""
        rc = getattr(self.lib, name)(C.byref(self.weights.struct), C.byref(desc), *args, _lib.stream_ptr(self.device))
        _lib.check(rc, name)

    def _n_streams(self, job, streams):
        """`streams` of sample / sample_ode / bpd: None = 2 from SPLIT_MIN_NODES nodes and two samples up, else 1."""
        if streams is not None:
            return streams
        return 2 if job.n_nodes >= self.SPLIT_MIN_NODES and len(job.sample_struct) >= 2 else 1

    def check_status(self, job):
        """Wait for the job's stream and raise if a forward produced inf / NaN (in the split-fp16 modes:
        also if an operand left the fp16 range, include/codlad_hip.h CODLAD_STATUS_NONFINITE)."""
        _lib.check(self.lib.codlad_status_check(_lib.ptr(job.status), _lib.stream_ptr(self.device)),
                   "codlad_status_check")

    def forward(self, job, x, t_value, x_self_cond=None, check=True):
        """One denoiser call: x [n_nodes,3] -> [n_nodes,6] (eps | variance logits).  x_self_cond
        [n_nodes,3]: previous pred_xstart, for a self-conditioned model only (None = zeros).
        check: synchronise and raise on a non-finite output."""
        _require_cuda(x, "x")
        x = x.contiguous().float()
        assert x.shape == (job.n_nodes, 3)
        if x_self_cond is not None:
            if not self.self_condition:
                raise ValueError("x_self_cond given to a model built without self_condition")
            _require_cuda(x_self_cond, "x_self_cond")
            x_self_cond = x_self_cond.contiguous().float()
            assert x_self_cond.shape == x.shape
        mods = self.step_mods([t_value])
        out = torch.empty(job.n_nodes, self.weights.out_dim, dtype=torch.float32, device=self.device)
        self._fresh_features(job.structures)
        self._run("codlad_denoiser_forward", job.desc(), _lib.ptr(x), _lib.ptr(x_self_cond), _lib.ptr(mods), _lib.ptr(out))
        if check:
            self.check_status(job)
        return out

    # A job of this many nodes or more runs as two half-jobs on two HIP streams (round 4; measured on BASELINE
    # configuration 2, 35 400 nodes: +2.5 %): the node kernel of such a job occupies ~140 of the 256 CUs and every kernel
    # has a tail, which the other half's edge kernels fill.  Every unit's result is independent of what shares its job
    # (tests hold that to the bit), so the split changes nothing but the schedule.  Three and more parts lose.
    # Where it starts to pay (tools/mall_probe.py, structures of 87 residues, one box): 34 800 nodes +2.0 %, 17 400 +2.1 %,
    # 8 700 +9.6 % (each half then takes the small-job node kernel), 5 220 -1.9 %, 3 480 +5.5 %, 1 740 -8 %.
    SPLIT_MIN_NODES = int(os.environ.get("CODLAD_SAMPLE_SPLIT_MIN_NODES", 8192))

    SAMPLE_KINDS = ("ddpm", "ddim", "ddim_reverse", "dpmpp")

    def sample(self, job, x_T, noise, tables, check=True, coef=None, streams=None, pin=None, kind="ddpm", x_start_out=None):
        """Full ancestral loop.  x_T [n_nodes,3]; noise [T,n_nodes,3] in loop order (first entry
        is used at step T-1); tables = diffusion_and_flow.schedule.Tables.  Returns x_0.
        check: after the loop, synchronise and raise if any step's output was not finite.
        coef: the [T, 8] step table when it is not the default sampler's (SpacedDiffusion.coefficients).
        streams: 1 = the whole job on the current stream; 2 = two half-jobs on two streams; None = 2 from
        SPLIT_MIN_NODES nodes up (and at least two samples).
        pin: (x0 [n_nodes,3], mask [n_nodes] bool / uint8 / int32) - residue pinning: at every step the pred_xstart of a
        masked node is replaced by its x0 before the clamp (codlad_sample_loop_pinned).
        kind: "ddpm" (the ancestral loop above), "ddim" (the DDIM loop, codlad_ddim_loop; coef = a Tables.ddim_coefficients
        table, default eta = 0), "ddim_reverse" (DDIM inversion: x_T holds x_0, the result is x_T; noise must be None) or
        "dpmpp" (DPM-Solver++(2M), codlad_dpm_loop; coef = a Tables.dpm_solver_coefficients table, default order 2;
        deterministic: noise must be None).
        x_start_out: a test aid (tests/test_dispatch_thresholds.py): a [n_nodes,3] float32 tensor to use as the loop's
        x_start buffer, which then holds the last step's pred_xstart.  The loop is the same with or without it:
        self-conditioning follows the model, not this pointer."""
        if kind not in self.SAMPLE_KINDS:
            raise ValueError(f"kind must be one of {self.SAMPLE_KINDS}, got {kind!r}")
        reverse = kind == "ddim_reverse"
        noiseless = reverse or kind == "dpmpp"
        T = tables.num_timesteps
        _require_cuda(x_T, "x_T")
        if noiseless:
            if noise is not None:
                raise ValueError(("the reverse DDIM loop" if reverse else "the DPM-Solver++ loop") +
                                 " is deterministic: noise must be None")
        else:
            _require_cuda(noise, "noise")
            assert noise.shape == (T, job.n_nodes, 3)
        assert x_T.shape == (job.n_nodes, 3)
        if x_start_out is not None:
            _require_cuda(x_start_out, "x_start_out")
            assert x_start_out.shape == x_T.shape and x_start_out.dtype == torch.float32 and x_start_out.is_contiguous()
        if pin is not None:
            pin = self._pin_arrays(pin, job.n_nodes)
        streams = self._n_streams(job, streams)
        if streams > 1:
            parts = job.parts(streams)
            pins = None if pin is None else [(pin[0][i], pin[1][i]) for _p, i in parts]
            noises = [None if noiseless else noise[:, i] for _p, i in parts]
            starts = None if x_start_out is None else [torch.empty(p.n_nodes, 3, dtype=torch.float32, device=self.device)
                                                        for p, _i in parts]
            outs = self.sample_many([p for p, _i in parts], [x_T[i] for _p, i in parts], noises,
                                    tables, check=check, coef=coef, pins=pins, kind=kind, x_start_outs=starts)
            x0 = torch.empty(job.n_nodes, 3, dtype=torch.float32, device=self.device)
            for k, ((_p, i), o) in enumerate(zip(parts, outs)):
                x0[i] = o
                if starts is not None:
                    x_start_out[i] = starts[k]
            return x0
        if coef is None:
            coef = (tables.step_coefficients() if kind == "ddpm" else tables.dpm_solver_coefficients() if kind == "dpmpp"
                    else tables.ddim_coefficients(reverse=reverse))
        fixed_var = bool(int(coef[0, 7]) & 2)
        if self.weights.out_dim != (3 if fixed_var else 6):
            raise ValueError(f"the {kind.upper()} loop needs a model with 6 outputs (mean | variance logits), or 3 with a "
                             "fixed-variance sampler (create_diffusion(learn_sigma=False)); a flow-matching model is sampled "
                             "with codlad_amd.diffusion_and_flow.ode.odeint")
        x = x_T.detach().clone().contiguous().float()
        noise = None if noiseless else noise.contiguous().float()
        mods = self.step_mods(tables.timestep_map)
        mode = int(coef[0, 7])                                  # the host's mode word (codlad_ddim_loop checks it)
        coef = torch.from_numpy(coef).to(self.device)
        self._fresh_features(job.structures)
        # pred_xstart, step to step: the self-conditioning input, and the history of the multistep solver
        x_start = x_start_out if x_start_out is not None else (
            torch.empty_like(x) if self.self_condition or kind == "dpmpp" else None)
        loop = [_lib.ptr(t) for t in (x, x_start, noise, mods, coef)] + [T]
        pin_ptrs = [_lib.ptr(t) for t in (pin or (None, None))]
        if kind == "dpmpp":
            self._run("codlad_dpm_loop", job.desc(), *(_lib.ptr(t) for t in (x, x_start, mods, coef)), T, mode, *pin_ptrs)
        elif kind != "ddpm":
            self._run("codlad_ddim_loop", job.desc(), *loop, mode, int(reverse), *pin_ptrs)
        elif pin is None:
            self._run("codlad_sample_loop", job.desc(), *loop)
        else:
            self._run("codlad_sample_loop_pinned", job.desc(), *loop, *pin_ptrs)
        if check:
            self.check_status(job)
        return x

    def sample_many(self, jobs, x_Ts, noises, tables, check=True, coef=None, pins=None, kind="ddpm", x_start_outs=None):
        """Several independent jobs at once, each on its own HIP stream: the node kernel of a 35 000-node job occupies 139 of
        the 256 CUs and every kernel has a tail - with a second job in flight another job's edge kernels run there (two
        half-jobs of BASELINE configuration 2: 1.03 x; more than two parts lose).  Every job carries its
        own workspace and the library keeps no state between jobs, so the results are those of `sample` job by job.
        pins: None, or one `pin` of `sample` (or None) per job.  kind as for `sample` (noises: None per job for
        "ddim_reverse" and "dpmpp").  x_start_outs: None, or one `x_start_out` of `sample` (or None) per job."""
        pins = [None] * len(jobs) if pins is None else list(pins)
        starts = [None] * len(jobs) if x_start_outs is None else list(x_start_outs)
        assert len(pins) == len(jobs) == len(starts)
        for job in jobs:                                  # features and the step tables once, on the caller's stream
            self._fresh_features(job.structures)
        self.step_mods(tables.timestep_map)
        # the pin arrays too: copies on the caller's stream, which the side streams wait for - and held until those have been
        # joined: the block of a mask released earlier goes to the next job's mask while a side stream still reads it
        pins = [None if pin is None else self._pin_arrays(pin, job.n_nodes) for job, pin in zip(jobs, pins)]

        def one(job, x_T, noise, pin, start):
            return self.sample(job, x_T, noise, tables, check=False, coef=coef, streams=1, pin=pin, kind=kind,
                               x_start_out=start)

        outs = self._on_streams([lambda a=a: one(*a) for a in zip(jobs, x_Ts, noises, pins, starts)], len(jobs))
        if check:
            for job in jobs:
                self.check_status(job)
        return outs

    # -- ODE sampling of the flow-matching models ---------------------------------------------------
    ODE_STAGES = {"euler": 1, "midpoint": 2, "rk4": 4}

    def _ode_fixed(self, job, y0, method, dts, mods):
        """One codlad_ode_loop call on the current stream -> traj [len(dts) + 1, n_nodes, 3]."""
        f32 = dict(dtype=torch.float32, device=self.device)
        y0 = y0.contiguous().float()
        traj = torch.empty(len(dts) + 1, job.n_nodes, 3, **f32)
        scratch = torch.empty(5, job.n_nodes, 3, **f32)
        dt = (C.c_float * len(dts))(*dts)
        self._run("codlad_ode_loop", job.desc(), _lib.ptr(y0), _lib.ptr(traj), _lib.ptr(mods), _lib.ODE_METHODS[method], dt,
                  len(dts), _lib.ptr(scratch))
        return traj

    def sample_ode(self, job, y0, ts, method="dopri5", rtol=1e-7, atol=1e-9, check=True, streams=None, max_steps=100000,
                   first_step=None):
        """The ODE sampler of a flow-matching model (3 outputs), fused: y0 [n_nodes, 3] at ts[0] -> (traj [len(ts),
        n_nodes, 3], {"n_eval", "n_accept", "n_reject"}).  ts: strictly monotonic host floats; x_self_cond of a
        self-conditioned model is zeros, as the reference's run_sampling calls it.
        euler / midpoint / rk4 (the 3/8 rule): one codlad_ode_loop call over the whole grid, increasing or decreasing;
        streams as for `sample` (None = two half-jobs on two streams from SPLIT_MIN_NODES nodes up; every unit's result
        is that of the unit alone, to the bit).
        dopri5: the error norm runs over the WHOLE state, so all samples of the job share one step size, as a batch does
        under torchdiffeq; it therefore always runs on one stream (`streams` is not read), and a sample's result depends
        on what shares its job.  One codlad_ode_dopri5_attempt per attempted step, then one small copy of the state block
        (with the job's status word in it) back to the host.  A non-finite error norm or model output stops the loop with
        a RuntimeError that names the time.  Increasing grids only.  first_step: the initial step size (torchdiffeq's
        option of that name) instead of Hairer's estimate, which costs a second evaluation and is always checked."""
        from .diffusion_and_flow import ode
        ts = [float(v) for v in ts]
        _require_cuda(y0, "y0")
        assert y0.shape == (job.n_nodes, 3)
        if self.weights.out_dim != 3:
            raise ValueError("sample_ode needs a flow-matching model (3 outputs: the velocity); a diffusion model is "
                             "sampled with Denoiser.sample")
        ode.check_grid(ts, method)
        self._fresh_features(job.structures)
        if method == "dopri5":
            return self._sample_dopri5(job, y0, ts, rtol, atol, check, max_steps, first_step)
        stages = self.ODE_STAGES[method]
        mods = self.step_mods(ode.stage_times(method, ts))
        dts = [b - a for a, b in zip(ts, ts[1:])]
        stats = {"n_eval": stages * len(dts), "n_accept": len(dts), "n_reject": 0}
        streams = self._n_streams(job, streams)
        if streams <= 1:
            traj = self._ode_fixed(job, y0, method, dts, mods)
            if check:
                self.check_status(job)
            return traj, stats
        parts = job.parts(streams)
        outs = self._on_streams([lambda p=p, i=i: self._ode_fixed(p, y0[i], method, dts, mods) for p, i in parts], streams)
        traj = torch.empty(len(ts), job.n_nodes, 3, dtype=torch.float32, device=self.device)
        for (_p, i), o in zip(parts, outs):
            traj[:, i] = o
        if check:
            self._check_all([p for p, _i in parts])
        return traj, stats

    def _sample_dopri5(self, job, y0, ts, rtol, atol, check, max_steps, first_step):
        from .diffusion_and_flow import ode
        f32 = dict(dtype=torch.float32, device=self.device)
        n = job.n_nodes

        def f(t, y, check=True):                        # the evaluations before the first attempt
            try:
                return self.forward(job, y, float(t), check=check)
            except RuntimeError as e:
                if "not finite" not in str(e):
                    raise
                raise RuntimeError(f"dopri5: the model output is not finite at t = {float(t)!r}") from e

        y = y0.detach().clone().contiguous().float()
        k = [f(ode._tt(ts[0], y), y, check or first_step is None)] + [torch.empty(n, 3, **f32) for _ in range(6)]
        h = ode._initial_step(f, ts[0], y, k[0], rtol, atol) if first_step is None else float(first_step)
        n_first = 2 if first_step is None else 1
        y1, xin = torch.empty(n, 3, **f32), torch.empty(n, 3, **f32)
        mods = torch.empty(6, MODS, **f32)
        norm = torch.empty(_lib.ODE_NORM_WORDS, dtype=torch.float64, device=self.device)
        host = _lib.OdeState()
        host.t, host.h = ts[0], h
        state = torch.frombuffer(bytearray(bytes(host)), dtype=torch.uint8).to(self.device)
        bufs = _lib.OdeDopri5Bufs()
        bufs.y, bufs.y1, bufs.xin, bufs.mods, bufs.state, bufs.norm = (
            _lib.ptr(t_) for t_ in (y, y1, xin, mods, state, norm))
        for j in range(7):
            bufs.k[j] = k[j].data_ptr()
        desc = job.desc()
        traj = torch.empty(len(ts), n, 3, **f32)
        traj[0] = y
        nxt, attempts = 1, 0
        while nxt < len(ts):
            attempts += 1
            if attempts > max_steps:
                raise RuntimeError("dopri5: max_steps exceeded")
            t_before = host.t
            self._run("codlad_ode_dopri5_attempt", desc, C.byref(bufs), C.c_double(ts[nxt]), C.c_float(rtol), C.c_float(atol))
            host = _lib.OdeState.from_buffer_copy(state.cpu().numpy().tobytes())   # the one readback: copy + synchronise
            if host.nonfinite or (check and host.status):
                job.status.zero_()
                raise RuntimeError(f"dopri5: the model output or the error norm is not finite in the step from t = "
                                   f"{t_before!r} (h = {host.hh!r}), attempt {attempts}: "
                                   f"{n_first + 6 * attempts} model evaluations so far")
            if host.accepted and host.t >= ts[nxt]:
                traj[nxt] = y
                nxt += 1
        return traj, {"n_eval": n_first + 6 * attempts, "n_accept": int(host.n_accept), "n_reject": int(host.n_reject)}

    # -- forward-only loss evaluation -------------------------------------------------------------
    @staticmethod
    def loss_table(tables, coef=None):
        """(device-ready [T, 16] fp32 numpy table, T): `coef` or the default sampler's Tables.loss_coefficients()."""
        coef = tables.loss_coefficients() if coef is None else coef
        coef = np.ascontiguousarray(coef, dtype=np.float32)
        if coef.shape != (tables.num_timesteps, tables.LOSS_COLUMNS):
            raise ValueError(f"coef must be a Tables.loss_coefficients table [{tables.num_timesteps}, "
                             f"{tables.LOSS_COLUMNS}], got {coef.shape}")
        return coef

    @staticmethod
    def sample_offsets(lens, device):
        """Device int32 [n_samples + 1]: first node of every sample, the node ranges of the loss kernels."""
        off = np.concatenate([[0], np.cumsum(np.asarray(lens, dtype=np.int64))])
        if (np.diff(off) < 1).any() or off[-1] >= 2 ** 31 // 3:
            raise ValueError("every sample needs at least one node (and all of them fit 32-bit element indices)")
        return torch.from_numpy(off.astype(np.int32)).to(device)

    @staticmethod
    def _timesteps(t, n_samples, T, device):
        """t: one value or one per sample -> (list of ints, shared value or None, device int32 [n_samples] or None)."""
        if isinstance(t, torch.Tensor):
            t = t.reshape(-1).tolist()
        ts = [int(t)] * n_samples if np.ndim(t) == 0 else [int(v) for v in t]
        if len(ts) != n_samples:
            raise ValueError(f"t must be one value or one per sample ({n_samples}), got {len(ts)}")
        if min(ts) < 0 or max(ts) >= T:
            raise ValueError(f"t must lie in [0, {T}), got {min(ts)} .. {max(ts)}")
        if len(set(ts)) == 1:
            return ts, ts[0], None
        return ts, None, torch.tensor(ts, dtype=torch.int32, device=device)

    @staticmethod
    def q_affine(kind, a, b, lens, t, coef):
        """The forward process on flat [n, 3] latents, samples of `lens` nodes each, t one value or one per sample, coef a
        Tables.loss_coefficients table.  kind "q_sample": sqrt_acp * a + sqrt(1 - acp) * b (b = noise; None: the mean of
        q_mean_variance) -> (x_t, 1 - acp, log(1 - acp)); "q_posterior": post_coef1 * a + post_coef2 * b (a = x_start,
        b = x_t) -> (mean, posterior_variance, posterior_log_variance_clipped); the last two broadcast to a's shape."""
        _require_cuda(a, "x_start")
        a = a.contiguous().float()
        if b is not None:
            _require_cuda(b, "noise" if kind == "q_sample" else "x_t")
            b = b.contiguous().float()
            if b.shape != a.shape:
                raise ValueError(f"{kind}: operands differ in shape, {tuple(a.shape)} and {tuple(b.shape)}")
        if a.numel() != 3 * int(sum(lens)):
            raise ValueError(f"{kind}: {a.numel()} values for {int(sum(lens))} nodes of 3 channels")
        T = coef.shape[0]
        _ts, shared, t_dev = Denoiser._timesteps(t, len(lens), T, a.device)
        off = Denoiser.sample_offsets(lens, a.device)
        coef_dev = torch.from_numpy(np.ascontiguousarray(coef, dtype=np.float32)).to(a.device)
        out, var, logvar = torch.empty_like(a), torch.empty_like(a), torch.empty_like(a)
        fn = {"q_sample": _lib.lib().codlad_q_sample, "q_posterior": _lib.lib().codlad_q_posterior}[kind]
        rc = fn(_lib.ptr(a), _lib.ptr(b), _lib.ptr(coef_dev), T, _lib.ptr(off), len(lens), _lib.ptr(t_dev),
                0 if shared is None else shared, _lib.ptr(out), _lib.ptr(var), _lib.ptr(logvar), _lib.stream_ptr(a.device))
        _lib.check(rc, f"codlad_{kind}")
        return out, var, logvar

    LOSS_KEYS = ("kl", "nll", "vb", "mse", "xstart_mse", "eps_mse")

    @staticmethod
    def _loss_outputs(n_samples, n_nodes, device, noise):
        res = {k: torch.empty(n_samples, dtype=torch.float32, device=device) for k in Denoiser.LOSS_KEYS
               if noise is not None or k not in ("mse", "eps_mse")}
        res["pred_xstart"] = torch.empty(n_nodes, 3, dtype=torch.float32, device=device)
        terms = _lib.LossTerms()
        for k, v in res.items():
            setattr(terms, k, v.data_ptr())
        return res, terms

    @staticmethod
    def vb_terms(model_out, x_start, x_t, noise, lens, t, coef):
        """_vb_terms_bpd / training_losses / calc_bpd_loop terms from a given model output (codlad_vb_terms): flat [n, 3]
        latents, model_out [n, 6] ([n, 3] under the table's fixed-variance bit), samples of `lens` nodes, t one value or
        one per sample -> {kl, nll, vb, xstart_mse [n_samples], pred_xstart [n, 3]; mse, eps_mse when noise is given}."""
        _require_cuda(x_start, "x_start")
        x_start = x_start.contiguous().float()
        n = int(sum(lens))
        coef = np.ascontiguousarray(coef, dtype=np.float32)
        _check_step_operands(x_start.reshape(n, 3), model_out, coef[0, :8], x_t=x_t, noise=noise)
        T = coef.shape[0]
        _ts, shared, t_dev = Denoiser._timesteps(t, len(lens), T, x_start.device)
        off = Denoiser.sample_offsets(lens, x_start.device)
        coef_dev = torch.from_numpy(coef).to(x_start.device)
        nz = None if noise is None else noise.contiguous().float()
        res, terms = Denoiser._loss_outputs(len(lens), n, x_start.device, nz)
        rc = _lib.lib().codlad_vb_terms(_lib.ptr(model_out.contiguous().float()), _lib.ptr(x_start),
                                        _lib.ptr(x_t.contiguous().float()), _lib.ptr(nz), _lib.ptr(coef_dev), T,
                                        _lib.ptr(off), len(lens), _lib.ptr(t_dev), 0 if shared is None else shared,
                                        C.byref(terms), _lib.stream_ptr(x_start.device))
        _lib.check(rc, "codlad_vb_terms")
        return res

    def _job_offsets(self, job):
        if getattr(job, "sample_off_dev", None) is None:
            job.sample_off_dev = self.sample_offsets(job.sample_lens, self.device)
        return job.sample_off_dev

    def q_sample(self, job, x_start, t, noise, tables, coef=None):
        """x_t [n_nodes, 3] = q_sample(x_start, t, noise) on the job's samples; t one respaced step or one per sample."""
        assert x_start.shape == (job.n_nodes, 3) and noise.shape == (job.n_nodes, 3)
        return self.q_affine("q_sample", x_start, noise, job.sample_lens, t, self.loss_table(tables, coef))[0]

    def _t_group_job(self, job, members, start):
        """Job.sub_job of the samples `members` from node `start`, cached on the job, which keeps the tensors alive: that
        pays when a grouping recurs (a fixed evaluation schedule, a shared timestep pattern per batch); with random
        timesteps it rarely does, so the cache is kept small."""
        cache = job.__dict__.setdefault("_t_groups", {})
        key = (start, tuple(members))
        if key not in cache:
            if len(cache) >= 64:
                cache.clear()
            cache[key] = job.sub_job(members, start)
        return cache[key]

    def _check_all(self, jobs):
        """check_status on every job - each one's sticky word is read and reset - and then the first failure raised."""
        first = None
        for jb in jobs:
            try:
                self.check_status(jb)
            except RuntimeError as e:
                first = first or e
        if first is not None:
            raise first

    def _on_streams(self, tasks, n_streams=2):
        """Runs the callables round-robin on up to n_streams side streams -> their results.  The side streams first wait for
        the caller's, so they see what it has enqueued (features, step tables, pin arrays); the caller's then waits for them."""
        if not hasattr(self, "_streams"):
            self._streams = []
        n_streams = min(n_streams, len(tasks))
        while len(self._streams) < n_streams:
            self._streams.append(torch.cuda.Stream(device=self.device))
        cur = torch.cuda.current_stream(self.device)
        for st in self._streams[:n_streams]:
            st.wait_stream(cur)
        outs = []
        for k, task in enumerate(tasks):
            with torch.cuda.stream(self._streams[k % n_streams]):
                outs.append(task())
        for st in self._streams[:n_streams]:
            cur.wait_stream(st)
        return outs

    def _loss_forward(self, job, x_start, x_t, noise, t, coef_dev, T, mods, x_self_cond, want_model_out):
        res, terms = self._loss_outputs(len(job.sample_struct), job.n_nodes, self.device, noise)
        if want_model_out:
            res["model_out"] = torch.empty(job.n_nodes, self.weights.out_dim, dtype=torch.float32, device=self.device)
        self._run("codlad_loss_forward", job.desc(), _lib.ptr(x_start), _lib.ptr(x_t), _lib.ptr(noise), _lib.ptr(x_self_cond),
                  _lib.ptr(mods[t]), _lib.ptr(coef_dev), T, t, _lib.ptr(self._job_offsets(job)), len(job.sample_struct),
                  _lib.ptr(res.get("model_out")), C.byref(terms))
        return res

    def _check_loss_model(self, coef):
        fixed_var = bool(int(coef[0, 7]) & 2)
        if self.weights.out_dim != (3 if fixed_var else 6):
            raise ValueError("the loss needs a model with 6 outputs (mean | variance logits), or 3 with a fixed-variance "
                             "diffusion (create_diffusion(learn_sigma=False))")

    def loss_terms(self, job, x_start, t, noise, tables, coef=None, x_t=None, x_self_cond=None, check=True,
                   want_model_out=False):
        """One denoiser forward on x_t = q_sample(x_start, t, noise) and the loss terms per sample (codlad_loss_forward):
        {kl, nll, vb, mse, xstart_mse, eps_mse [n_samples], pred_xstart [n_nodes, 3] (, model_out)}; mse is
        training_losses' (target by the mean type), xstart_mse / eps_mse are calc_bpd_loop's.
        t: one respaced step, or one per sample: the samples are then grouped by equal t and every group runs as a ragged
        sub-job at its t, on two streams; a sample's result does not depend on what shares its job, so the result is, bit
        for bit, that of calling each group alone.  x_t: given instead of computed (noise may then be None: no mse /
        eps_mse).  coef: the Tables.loss_coefficients table when it is not the default diffusion's."""
        coef = self.loss_table(tables, coef)
        self._check_loss_model(coef)
        T, S = tables.num_timesteps, len(job.sample_struct)
        _require_cuda(x_start, "x_start")
        x_start = x_start.contiguous().float()
        assert x_start.shape == (job.n_nodes, 3)
        if noise is not None:
            _require_cuda(noise, "noise")
            noise = noise.contiguous().float()
            assert noise.shape == x_start.shape
        if x_t is None:
            if noise is None:
                raise ValueError("loss_terms needs noise or x_t")
            x_t = self.q_sample(job, x_start, t, noise, tables, coef)
        else:
            _require_cuda(x_t, "x_t")
            x_t = x_t.contiguous().float()
            assert x_t.shape == x_start.shape
        if x_self_cond is not None:
            if not self.self_condition:
                raise ValueError("x_self_cond given to a model built without self_condition")
            _require_cuda(x_self_cond, "x_self_cond")
            x_self_cond = x_self_cond.contiguous().float()
            assert x_self_cond.shape == x_start.shape
        ts, shared, _t_dev = self._timesteps(t, S, T, self.device)
        self._fresh_features(job.structures)
        mods = self.step_mods(tables.timestep_map)
        coef_dev = torch.from_numpy(coef).to(self.device)
        if shared is not None:
            res = self._loss_forward(job, x_start, x_t, noise, shared, coef_dev, T, mods, x_self_cond, want_model_out)
            if check:
                self.check_status(job)
            return res
        groups = [(tv, [m for m in range(S) if ts[m] == tv]) for tv in sorted(set(ts))]
        subs, start = [], 0
        for _tv, members in groups:
            subs.append(self._t_group_job(job, members, start))
            start += subs[-1][0].n_nodes
        pick = lambda a, i: None if a is None else a[i]            # noqa: E731
        tasks = [lambda tv=tv, sub=sub, i=i: self._loss_forward(sub, x_start[i], x_t[i], pick(noise, i), tv, coef_dev, T,
                                                                mods, pick(x_self_cond, i), want_model_out)
                 for (tv, _m), (sub, i) in zip(groups, subs)]
        outs = self._on_streams(tasks)
        res = {}
        for (_tv, members), (sub, i), o in zip(groups, subs, outs):
            m = torch.tensor(members, dtype=torch.int64, device=self.device)
            for k, v in o.items():
                per_node = k in ("pred_xstart", "model_out")
                if k not in res:
                    res[k] = torch.empty((job.n_nodes if per_node else S,) + tuple(v.shape[1:]), dtype=v.dtype,
                                         device=self.device)
                res[k][i if per_node else m] = v
        if check:
            self._check_all([sub for sub, _i in subs])
        return res

    def bpd(self, job, x_start, noise, tables, streams=None, coef=None, check=True):
        """The variational bound in bits per dimension over all T steps, fused (codlad_bpd_loop; the IDDPM release's
        calc_bpd_loop): x_start [n_nodes, 3], noise [T, n_nodes, 3] in loop order (entry 0 at step T-1) ->
        {total_bpd, prior_bpd [n_samples]; vb, mse, xstart_mse [T, n_samples], row i = respaced step i}.
        streams as for `sample`: None = two half-jobs on two streams from SPLIT_MIN_NODES nodes up."""
        coef = self.loss_table(tables, coef)
        self._check_loss_model(coef)
        T, S = tables.num_timesteps, len(job.sample_struct)
        _require_cuda(x_start, "x_start")
        _require_cuda(noise, "noise")
        assert x_start.shape == (job.n_nodes, 3) and noise.shape == (T, job.n_nodes, 3)
        streams = self._n_streams(job, streams)
        self._fresh_features(job.structures)
        mods = self.step_mods(tables.timestep_map)
        coef_dev = torch.from_numpy(coef).to(self.device)

        def run(jb, x0, eps):
            x0, eps = x0.contiguous().float(), eps.contiguous().float()
            n = len(jb.sample_struct)
            f32 = dict(dtype=torch.float32, device=self.device)
            out = {k: torch.empty(T, n, **f32) for k in ("vb", "mse", "xstart_mse")}
            out.update({k: torch.empty(n, **f32) for k in ("prior_bpd", "total_bpd")})
            x_t = torch.empty_like(x0)
            self._run("codlad_bpd_loop", jb.desc(), _lib.ptr(x0), _lib.ptr(eps), _lib.ptr(x_t), _lib.ptr(mods), _lib.ptr(coef_dev),
                      T, _lib.ptr(self._job_offsets(jb)), n,
                      *(_lib.ptr(out[k]) for k in ("vb", "mse", "xstart_mse", "prior_bpd", "total_bpd")))
            return out

        if streams <= 1:
            res = run(job, x_start, noise)
            if check:
                self.check_status(job)
            return res
        parts = job.parts(streams)
        outs = self._on_streams([lambda p=p, i=i: run(p, x_start[i], noise[:, i]) for p, i in parts], streams)
        f32 = dict(dtype=torch.float32, device=self.device)
        res = {k: torch.empty(T, S, **f32) for k in ("vb", "mse", "xstart_mse")}
        res.update({k: torch.empty(S, **f32) for k in ("prior_bpd", "total_bpd")})
        for p, o in enumerate(outs):
            for k, v in o.items():
                res[k][..., p::streams] = v
        if check:
            self._check_all([p for p, _i in parts])
        return res

    # -- forward-only loss evaluation of the flow-matching models ---------------------------------
    FM_LOSS_KEYS = ("l2", "l1", "huber", "smooth_l1", "log_cosh")

    @staticmethod
    def _fm_kind(kind, sigma):
        if kind not in _lib.FM_KINDS:
            raise ValueError(f"kind must be one of {tuple(_lib.FM_KINDS)}, got {kind!r}")
        if isinstance(sigma, bool) or not isinstance(sigma, (int, float)):
            raise TypeError(f"sigma must be a number, got {type(sigma).__name__}")
        if not sigma >= 0:
            raise ValueError(f"sigma must be >= 0, got {sigma}")
        return _lib.FM_KINDS[kind], float(sigma)

    @staticmethod
    def _fm_times(t, n_samples, device):
        """t in [0, 1]: one value or one per sample -> (list of floats as fp32 holds them, shared value or None, device
        float32 [n_samples] or None)."""
        if isinstance(t, torch.Tensor):
            t = t.reshape(-1).tolist()
        ts = [t] * n_samples if np.ndim(t) == 0 else list(t)
        ts = [float(np.float32(v)) for v in ts]
        if len(ts) != n_samples:
            raise ValueError(f"t must be one value or one per sample ({n_samples}), got {len(ts)}")
        if not all(0.0 <= v <= 1.0 for v in ts):
            raise ValueError(f"t must lie in [0, 1], got {min(ts)} .. {max(ts)}")
        if len(set(ts)) == 1:
            return ts, ts[0], None
        return ts, None, torch.tensor(ts, dtype=torch.float32, device=device)

    @staticmethod
    def _fm_operand(a, name, like):
        if a is None:
            return None
        _require_cuda(a, name)
        a = a.contiguous().float()
        if like is not None and a.shape != like.shape:
            raise ValueError(f"{name} {tuple(a.shape)} does not match x1 {tuple(like.shape)}")
        return a

    @staticmethod
    def fm_path(kind, sigma, x0, x1, eps, lens, t):
        """The probability path of a conditional flow matcher on flat [n, 3] latents (codlad_fm_path), samples of `lens`
        nodes, t in [0, 1] one value or one per sample -> (xt, ut).  kind "icfm" (ConditionalFlowMatcher), "target"
        (TargetConditionalFlowMatcher; x0 is not read, may be None) or "vp" (VariancePreservingConditionalFlowMatcher);
        eps may be None for icfm / vp at sigma = 0."""
        kind_id, sigma = Denoiser._fm_kind(kind, sigma)
        x1 = Denoiser._fm_operand(x1, "x1", None)
        n = int(sum(lens))
        if x1.numel() != 3 * n:
            raise ValueError(f"fm_path: {x1.numel()} values for {n} nodes of 3 channels")
        x0, eps = Denoiser._fm_operand(x0, "x0", x1), Denoiser._fm_operand(eps, "eps", x1)
        if kind != "target" and x0 is None:
            raise ValueError(f"fm_path: the {kind} matcher needs x0")
        if eps is None and (kind == "target" or sigma != 0):
            raise ValueError("fm_path: eps may be None only for icfm / vp at sigma = 0")
        _ts, shared, t_dev = Denoiser._fm_times(t, len(lens), x1.device)
        off = Denoiser.sample_offsets(lens, x1.device)
        xt, ut = torch.empty_like(x1), torch.empty_like(x1)
        rc = _lib.lib().codlad_fm_path(_lib.ptr(x0), _lib.ptr(x1), _lib.ptr(eps), _lib.ptr(off), len(lens), _lib.ptr(t_dev),
                                       0.0 if shared is None else shared, kind_id, sigma, _lib.ptr(xt), _lib.ptr(ut),
                                       _lib.stream_ptr(x1.device))
        _lib.check(rc, "codlad_fm_path")
        return xt, ut

    @staticmethod
    def _fm_outputs(shape, device):
        res = {k: torch.empty(*shape, dtype=torch.float32, device=device) for k in Denoiser.FM_LOSS_KEYS}
        out = _lib.FmLossOut()
        for k, v in res.items():
            setattr(out, k, v.data_ptr())
        return res, out

    @staticmethod
    def fm_terms(model_out, ut, lens):
        """loss_fn's five regression losses per sample from a given model output (codlad_fm_terms): flat [n, 3] model_out
        and ut, samples of `lens` nodes -> {l2, l1, huber, smooth_l1, log_cosh [n_samples]}, each the mean over the
        sample's elements."""
        _require_cuda(model_out, "model_out")
        _require_cuda(ut, "ut")
        model_out, ut = model_out.contiguous().float(), ut.contiguous().float()
        n = int(sum(lens))
        if tuple(model_out.shape) != (n, 3) or tuple(ut.shape) != (n, 3):
            raise ValueError(f"fm_terms: model_out and ut must be [{n}, 3], got {tuple(model_out.shape)} and {tuple(ut.shape)}")
        off = Denoiser.sample_offsets(lens, ut.device)
        res, out = Denoiser._fm_outputs((len(lens),), ut.device)
        rc = _lib.lib().codlad_fm_terms(_lib.ptr(model_out), _lib.ptr(ut), _lib.ptr(off), len(lens), C.byref(out),
                                        _lib.stream_ptr(ut.device))
        _lib.check(rc, "codlad_fm_terms")
        return res

    def _check_fm_model(self):
        if self.weights.out_dim != 3:
            raise ValueError("the flow-matching losses need a flow-matching model (3 outputs: the velocity); a diffusion "
                             "model is scored with Denoiser.loss_terms / Denoiser.bpd")

    def _fm_loss_forward(self, job, xt, ut, mods_t, want_model_out):
        res, out = self._fm_outputs((len(job.sample_struct),), self.device)
        if want_model_out:
            res["model_out"] = torch.empty(job.n_nodes, 3, dtype=torch.float32, device=self.device)
        self._run("codlad_fm_loss_forward", job.desc(), _lib.ptr(xt), _lib.ptr(ut), _lib.ptr(mods_t),
                  _lib.ptr(self._job_offsets(job)), len(job.sample_struct), _lib.ptr(res.get("model_out")), C.byref(out))
        return res

    def fm_loss_terms(self, job, x1, t, kind="icfm", sigma=0.0, x0=None, eps=None, check=True, want_model_out=False):
        """The path of the matcher (`fm_path`) at time t, one denoiser forward on xt and loss_fn's five losses per sample
        (codlad_fm_loss_forward): {l2, l1, huber, smooth_l1, log_cosh [n_samples], xt, ut [n_nodes, 3] (, model_out)}.
        t: one time in [0, 1], or one per sample: the samples are then grouped by equal time and every group runs as a
        ragged sub-job at its time, on two streams, as `loss_terms` groups by timestep; a sample's result does not depend
        on what shares its job, so the result is, bit for bit, that of calling each group alone.  All distinct times go
        through one codlad_step_mods_f call.  A batch of N distinct random times therefore costs N small forwards: for a
        loss over time, `fm_loss_sweep` (one time shared by all samples per forward) is the fast path.  A self-conditioned
        model is conditioned on zeros."""
        self._check_fm_model()
        S = len(job.sample_struct)
        xt, ut = self.fm_path(kind, sigma, x0, x1, eps, job.sample_lens, t)
        ts, shared, _t_dev = self._fm_times(t, S, self.device)
        self._fresh_features(job.structures)
        distinct = sorted(set(ts))
        mods = self.step_mods(distinct, as_float=True)
        if shared is not None:
            res = self._fm_loss_forward(job, xt, ut, mods[0], want_model_out)
            res.update(xt=xt, ut=ut)
            if check:
                self.check_status(job)
            return res
        groups = [(tv, [m for m in range(S) if ts[m] == tv]) for tv in distinct]
        subs, start = [], 0
        for _tv, members in groups:
            subs.append(self._t_group_job(job, members, start))
            start += subs[-1][0].n_nodes
        tasks = [lambda g=g, sub=sub, i=i: self._fm_loss_forward(sub, xt[i], ut[i], mods[g], want_model_out)
                 for g, (sub, i) in enumerate(subs)]
        outs = self._on_streams(tasks)
        res = {"xt": xt, "ut": ut}
        for (_tv, members), (sub, i), o in zip(groups, subs, outs):
            m = torch.tensor(members, dtype=torch.int64, device=self.device)
            for k, v in o.items():
                per_node = k == "model_out"
                if k not in res:
                    res[k] = torch.empty((job.n_nodes if per_node else S,) + tuple(v.shape[1:]), dtype=v.dtype,
                                         device=self.device)
                res[k][i if per_node else m] = v
        if check:
            self._check_all([sub for sub, _i in subs])
        return res

    def fm_loss_sweep(self, job, x1, ts, kind="icfm", sigma=0.0, x0=None, eps=None, streams=None, check=True):
        """loss_fn's five losses over a sweep of times, fused (codlad_fm_loss_loop): for every ts[k] in [0, 1], shared by all
        samples, the path with eps[k] (eps [K, n_nodes, 3]; None for icfm / vp at sigma = 0), one forward and the terms ->
        {l2, l1, huber, smooth_l1, log_cosh [K, n_samples]}.  Row k is, bit for bit, `fm_loss_terms` at ts[k] with eps[k].
        streams as for `bpd`: None = two half-jobs on two streams from SPLIT_MIN_NODES nodes up."""
        self._check_fm_model()
        kind_id, sigma = self._fm_kind(kind, sigma)
        ts = [float(np.float32(v)) for v in ts]
        K, S = len(ts), len(job.sample_struct)
        if K < 1 or not all(0.0 <= v <= 1.0 for v in ts):
            raise ValueError("fm_loss_sweep: ts must be a non-empty list of times in [0, 1]")
        x1 = self._fm_operand(x1, "x1", None)
        assert x1.shape == (job.n_nodes, 3)
        x0 = self._fm_operand(x0, "x0", x1)
        if kind != "target" and x0 is None:
            raise ValueError(f"fm_loss_sweep: the {kind} matcher needs x0")
        if eps is None:
            if kind == "target" or sigma != 0:
                raise ValueError("fm_loss_sweep: eps may be None only for icfm / vp at sigma = 0")
        else:
            _require_cuda(eps, "eps")
            if tuple(eps.shape) != (K, job.n_nodes, 3):
                raise ValueError(f"eps must be [K, n_nodes, 3] = {(K, job.n_nodes, 3)}, got {tuple(eps.shape)}")
        streams = self._n_streams(job, streams)
        self._fresh_features(job.structures)
        mods = self.step_mods(ts, as_float=True)
        t_host = (C.c_float * K)(*ts)

        def run(jb, a0, a1, ae):
            a1 = a1.contiguous().float()
            a0 = None if a0 is None else a0.contiguous().float()
            ae = None if ae is None else ae.contiguous().float()
            n = len(jb.sample_struct)
            res, out = self._fm_outputs((K, n), self.device)
            xt, ut = torch.empty_like(a1), torch.empty_like(a1)
            self._run("codlad_fm_loss_loop", jb.desc(), _lib.ptr(a0), _lib.ptr(a1), _lib.ptr(ae), kind_id, sigma, t_host, K,
                      _lib.ptr(mods), _lib.ptr(self._job_offsets(jb)), n, _lib.ptr(xt), _lib.ptr(ut), C.byref(out))
            return res

        pick = lambda a, i: None if a is None else a[i]                    # noqa: E731
        if streams <= 1:
            res = run(job, x0, x1, eps)
            if check:
                self.check_status(job)
            return res
        parts = job.parts(streams)
        outs = self._on_streams([lambda p=p, i=i: run(p, pick(x0, i), x1[i], None if eps is None else eps[:, i])
                                 for p, i in parts], streams)
        res = {k: torch.empty(K, S, dtype=torch.float32, device=self.device) for k in self.FM_LOSS_KEYS}
        for p, o in enumerate(outs):
            for k, v in o.items():
                res[k][..., p::streams] = v
        if check:
            self._check_all([p for p, _i in parts])
        return res

    @staticmethod
    def _pin_arrays(pin, n_nodes):
        """(x0, mask) -> (x0 fp32 [n_nodes,3] contiguous, mask uint8 [n_nodes]) on the GPU, checked."""
        x0, mask = pin
        _require_cuda(x0, "pin x0")
        _require_cuda(mask, "pin mask")
        if tuple(x0.shape) != (n_nodes, 3) or tuple(mask.shape) != (n_nodes,):
            raise ValueError(f"pin: x0 must be [{n_nodes}, 3] and mask [{n_nodes}], got {tuple(x0.shape)} and {tuple(mask.shape)}")
        if not x0.is_floating_point():
            raise TypeError(f"pin: x0 must be a floating-point tensor, got {x0.dtype}")
        if mask.dtype not in (torch.bool, torch.uint8, torch.int32):
            raise TypeError(f"pin: mask must be bool, uint8 or int32, got {mask.dtype}")
        x0 = x0.contiguous().float()
        if mask.dtype != torch.uint8:
            mask = mask != 0
        return x0, mask.to(torch.uint8).contiguous()

    def ddpm_update(self, x, model_out, noise, tables, i, return_x_start=False):
        _require_cuda(x, "x")
        n = x.numel() // 3
        x = x.contiguous().float()
        out = torch.empty_like(x)
        x_start = torch.empty_like(x) if return_x_start else None
        coef = np.ascontiguousarray(tables.step_coefficients()[i])
        rc = self.lib.codlad_ddpm_update(_lib.ptr(x), _lib.ptr(model_out.contiguous().float()),
                                         _lib.ptr(noise.contiguous().float()),
                                         coef.ctypes.data_as(C.c_void_p), n, _lib.ptr(out), _lib.ptr(x_start),
                                         _lib.stream_ptr(self.device))
        _lib.check(rc, "codlad_ddpm_update")
        return (out, x_start) if return_x_start else out

    @staticmethod
    def ddpm_pred_xstart(x, model_out, coef):
        """The raw pred_xstart of one step (before denoised_fn and the clamp): x [n,3], model_out [n,6] (or [n,3] with a
        fixed-variance row), coef = one [8] row of the step table (codlad_ddpm_pred_xstart).  Needs no Denoiser: any
        model's output is stepped with it (diffusion_and_flow's per-step path)."""
        _require_cuda(x, "x")
        x = x.contiguous().float()
        out = torch.empty_like(x)
        coef = np.ascontiguousarray(coef, dtype=np.float32)
        _check_step_operands(x, model_out, coef)
        rc = _lib.lib().codlad_ddpm_pred_xstart(_lib.ptr(x), _lib.ptr(model_out.contiguous().float()),
                                                coef.ctypes.data_as(C.c_void_p), x.numel() // 3, _lib.ptr(out),
                                                _lib.stream_ptr(x.device))
        _lib.check(rc, "codlad_ddpm_pred_xstart")
        return out

    @staticmethod
    def ddpm_posterior_step(x, pred_xstart, model_out, noise, coef, grad=None, fixed_variance=0.0):
        """The rest of the step given a (processed) pred_xstart: clamp (mode bit 4), posterior mean, + variance * grad
        (cond_fn), noise -> (sample, clamped pred_xstart) (codlad_ddpm_posterior_step)."""
        _require_cuda(x, "x")
        x = x.contiguous().float()
        out = torch.empty_like(x)
        x_start = torch.empty_like(x)
        coef = np.ascontiguousarray(coef, dtype=np.float32)
        g = None if grad is None else grad.contiguous().float()
        _check_step_operands(x, model_out, coef, pred_xstart=pred_xstart, noise=noise, grad=g)
        rc = _lib.lib().codlad_ddpm_posterior_step(_lib.ptr(x), _lib.ptr(pred_xstart.contiguous().float()),
                                                   _lib.ptr(model_out.contiguous().float()),
                                                   _lib.ptr(noise.contiguous().float()), _lib.ptr(g),
                                                   coef.ctypes.data_as(C.c_void_p), C.c_float(fixed_variance),
                                                   x.numel() // 3, _lib.ptr(out), _lib.ptr(x_start),
                                                   _lib.stream_ptr(x.device))
        _lib.check(rc, "codlad_ddpm_posterior_step")
        return out, x_start

    @staticmethod
    def ddim_step(x, pred_xstart, noise, coef, grad=None, reverse=False):
        """One DDIM update given a (processed) pred_xstart: clamp (mode bit 4), condition_score with grad (cond_fn), eps
        from pred_xstart, then the forward update with noise or the reverse one (noise None) -> (sample, the pred_xstart
        the step used) (codlad_ddim_step).  coef = one [8] row of Tables.ddim_coefficients."""
        _require_cuda(x, "x")
        x = x.contiguous().float()
        out = torch.empty_like(x)
        x_start = torch.empty_like(x)
        coef = np.ascontiguousarray(coef, dtype=np.float32)
        if reverse != (noise is None):
            raise ValueError("the forward DDIM step takes noise, the reverse one none")
        nz = None if noise is None else noise.contiguous().float()
        g = None if grad is None else grad.contiguous().float()
        _check_step_operands(x, None, coef, pred_xstart=pred_xstart, noise=nz, grad=g)
        rc = _lib.lib().codlad_ddim_step(_lib.ptr(x), _lib.ptr(pred_xstart.contiguous().float()), _lib.ptr(nz),
                                         _lib.ptr(g), coef.ctypes.data_as(C.c_void_p), int(bool(reverse)),
                                         x.numel() // 3, _lib.ptr(out), _lib.ptr(x_start), _lib.stream_ptr(x.device))
        _lib.check(rc, "codlad_ddim_step")
        return out, x_start

    @staticmethod
    def dpm_step(x, pred_xstart, prev_xstart, coef, grad=None):
        """One DPM-Solver++(2M) update given this step's (processed) pred_xstart and the previous step's: clamp (mode
        bit 4), condition_score with grad (cond_fn), then x <- (A x + B pred_xstart) + C prev_xstart -> (sample, the
        pred_xstart the step used) (codlad_dpm_step).  coef = one [8] row of Tables.dpm_solver_coefficients; prev_xstart
        is None exactly when its C (column 4) is 0: the first and the last step, and every step of order 1."""
        _require_cuda(x, "x")
        x = x.contiguous().float()
        out = torch.empty_like(x)
        x_start = torch.empty_like(x)
        coef = np.ascontiguousarray(coef, dtype=np.float32)
        g = None if grad is None else grad.contiguous().float()
        prev = None if prev_xstart is None else prev_xstart.contiguous().float()
        _check_step_operands(x, None, coef, pred_xstart=pred_xstart, prev_xstart=prev, grad=g)
        if (coef[4] != 0) != (prev is not None):
            raise ValueError("prev_xstart is given exactly when the row's C (column 4) is not 0")
        rc = _lib.lib().codlad_dpm_step(_lib.ptr(x), _lib.ptr(pred_xstart.contiguous().float()), _lib.ptr(prev), _lib.ptr(g),
                                        coef.ctypes.data_as(C.c_void_p), x.numel() // 3, _lib.ptr(out), _lib.ptr(x_start),
                                        _lib.stream_ptr(x.device))
        _lib.check(rc, "codlad_dpm_step")
        return out, x_start


def _check_step_operands(x, model_out, coef, **same_as_x):
    """Shapes of the split step's operands: the kernels index model_out as [n][6] ([n][3] under the fixed-variance mode
    bit) and every other tensor as [n][3]."""
    n = x.numel() // 3
    if x.numel() != 3 * n or n == 0:
        raise ValueError(f"x must hold [n, 3] latents, got {tuple(x.shape)}")
    if coef.shape != (8,):
        raise ValueError(f"coef must be one [8] row of the step table, got {coef.shape}")
    width = 3 if int(coef[7]) & 2 else 6
    for name, t in dict(model_out=model_out, **same_as_x).items():
        if t is None:
            continue
        _require_cuda(t, name)
        want = n * (width if name == "model_out" else 3)
        if t.numel() != want:
            raise ValueError(f"{name} holds {t.numel()} values, the step needs {want} ({n} nodes)")


class Decoder:
    """De-normalise + VQ lookup + IC decoder + ic_to_xyz."""

    def __init__(self, state_dict, device, mean3=None, std3=None, angle=False, n_codes=4096):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("codlad_amd runs on an MI355X only; no CPU path exists")
        self.lib = _lib.lib()
        # state_dict None: a rank that loads no checkpoint (`angle` / `n_codes` give the layout; a broadcast whose
        # header says otherwise re-derives it)
        if state_dict is None:
            self.weights = DecoderWeights.empty(self.device, angle, n_codes)
        else:
            self.weights = DecoderWeights(state_dict, self.device, mean3, std3)
        f = dict(dtype=torch.float32, device=self.device)
        self._unit = (torch.zeros(3, **f), torch.ones(3, **f))

    # the de-normalisation statistics live in the weight blob (they travel with a broadcast)
    @property
    def mean(self):
        return self.weights.mean

    @property
    def std(self):
        return self.weights.std

    def vq(self, x, normalised=True):
        """x [..., 3] -> (idx int64 [n], z_q [..., 3], latent [..., 3]); de-normalises first when
        `normalised` (reference test.py:548), else looks x up as is."""
        _require_cuda(x, "latent")
        xs = x.contiguous().float()
        n = xs.numel() // 3
        idx = torch.empty(n, dtype=torch.int64, device=self.device)
        zq = torch.empty_like(xs)
        lat = torch.empty_like(xs)
        mean, std = (self.mean, self.std) if normalised else self._unit
        cb = self.weights.codebook
        rc = self.lib.codlad_vq_lookup(_lib.ptr(xs), n, _lib.ptr(mean), _lib.ptr(std), _lib.ptr(cb),
                                       cb.shape[0], _lib.ptr(idx), _lib.ptr(zq), _lib.ptr(lat),
                                       _lib.stream_ptr(self.device))
        _lib.check(rc, "codlad_vq_lookup")
        return idx, zq, lat

    @staticmethod
    def csr_from_pairs(pairs, n_nodes):
        """Undirected CG pairs [E,2] -> CSR over the receiving node of the directed graph, in the
        order the reference's scatter_add visits them (models/gcn_nn.py:54-64, vae_model.py:485)."""
        gtr_ij = bool((pairs[:, 0] > pairs[:, 1]).any())
        gtr_ji = bool((pairs[:, 1] > pairs[:, 0]).any())
        directed = pairs if (gtr_ij and gtr_ji) else torch.cat([pairs, pairs.flip(1)], dim=0)
        recv = directed[:, 0]
        order = torch.sort(recv, stable=True).indices
        src = directed[order, 1].to(torch.int32).contiguous()
        counts = torch.bincount(recv, minlength=n_nodes)
        ptr = torch.zeros(n_nodes + 1, dtype=torch.int32, device=pairs.device)
        ptr[1:] = torch.cumsum(counts, 0).to(torch.int32)
        return ptr, src

    def build_csr(self, cg_xyz, sample_lens, cutoff=21.0, sample_range=None, max_edges=None):
        """Directed CG graph of every sample as CSR, on the device (what the reference's host
        preprocessing + make_directed + scatter order amount to).  cg_xyz [M,3] flat over samples,
        sample_lens: residues per sample."""
        xyz = cg_xyz.to(self.device).contiguous().float()
        M = xyz.shape[0]
        rng = self.sample_ranges(sample_lens) if sample_range is None else sample_range
        assert rng.shape == (M, 2)
        deg = torch.empty(M, dtype=torch.int32, device=self.device)
        st = _lib.stream_ptr(self.device)
        _lib.check(self.lib.codlad_cg_graph(_lib.ptr(xyz), _lib.ptr(rng), M, C.c_float(cutoff), _lib.ptr(deg),
                                            None, None, st), "codlad_cg_graph(count)")
        ptr = torch.zeros(M + 1, dtype=torch.int32, device=self.device)
        ptr[1:] = torch.cumsum(deg, 0).to(torch.int32)
        # max_edges (an upper bound on the directed edge count, e.g. sum L*(L-1)) avoids the host
        # round trip that sizes csr_src exactly; the tail past ptr[-1] is then simply unused
        n_src = max_edges if max_edges is not None else int(ptr[-1])
        src = torch.empty(max(n_src, 1), dtype=torch.int32, device=self.device)
        _lib.check(self.lib.codlad_cg_graph(_lib.ptr(xyz), _lib.ptr(rng), M, C.c_float(cutoff), None,
                                            _lib.ptr(ptr), _lib.ptr(src), st), "codlad_cg_graph(fill)")
        return ptr, src[:n_src]

    def sample_ranges(self, sample_lens):
        """[M,2] int32 device table {first node, L} of the sample each flat node belongs to."""
        M = int(sum(sample_lens))
        rng = np.empty((M, 2), dtype=np.int32)
        o = 0
        for L in sample_lens:
            rng[o:o + L, 0] = o
            rng[o:o + L, 1] = L
            o += L
        return torch.from_numpy(rng).to(self.device)

    # The decoder's scratch, float [M][200], as the kernels lay it out (csrc/ic_decoder_kernels.hip, "Scratch"): four
    # planes of 40 M floats, S^T [40][M] | V [M][40] | phi_a [M][40] | phi_b [M][40]; message block b reads its phi from
    # plane b & 1 and writes the next block's to the other.  Nothing else in Python knows this.
    SCRATCH_WIDTH = 200

    @staticmethod
    def read_taps(scratch):
        """What a finished ic_decode leaves in the `scratch` it was given -> dict of [M,40] tensors (copies): "S" the
        final state (the heads' input), "V" the message sum of block 3, "phi3" the phi rows block 3 summed over and
        "phi2" those of block 2."""
        M = scratch.shape[0]
        assert scratch.shape == (M, Decoder.SCRATCH_WIDTH) and scratch.is_contiguous()
        planes = scratch.reshape(-1).reshape(5, 40 * M)
        return {"S": planes[0].reshape(40, M).t().contiguous(), "V": planes[1].reshape(M, 40).clone(),
                "phi2": planes[2].reshape(M, 40).clone(), "phi3": planes[3].reshape(M, 40).clone()}

    def ic_decode(self, z_q, cg_z, cg_xyz, pairs=None, csr=None, scratch=None):
        """z_q [M,3], cg_z [M], cg_xyz [M,3] and either the undirected CG pairs [E,2] (flat node
        indices, as in batch['CG_nbr_list']) or a prebuilt csr = (ptr, src) -> ic [M,13,3].
        scratch: the caller's own float32 [M,200] work buffer in place of a fresh one; `read_taps` reads the
        intermediate state out of it afterwards."""
        _require_cuda(z_q, "z_q")
        M = z_q.shape[0]
        cg_z = cg_z.to(self.device, torch.int32).contiguous()
        lo, hi = int(cg_z.min()), int(cg_z.max())
        if lo < 0 or hi >= 25:      # res_embed / backbone_dist / sidechain_* tables have 25 rows (vae_model.py:330-345)
            raise ValueError(f"cg_z (residue types {lo}..{hi}) outside the decoder's 25-row embedding tables")
        ptr, src = csr if csr is not None else self.csr_from_pairs(pairs.to(self.device), M)
        assert ptr.numel() == M + 1 and ptr.dtype == torch.int32 and src.dtype == torch.int32
        if src.numel() == 0:        # a graph without edges (either builder returns an empty src, whose pointer is null):
            src = torch.zeros(1, dtype=torch.int32, device=self.device)      # the library wants a buffer; every V is 0
        if scratch is None:
            scratch = torch.empty(M, self.SCRATCH_WIDTH, dtype=torch.float32, device=self.device)
        else:
            _require_cuda(scratch, "scratch")
            if scratch.shape != (M, self.SCRATCH_WIDTH) or scratch.dtype != torch.float32 or not scratch.is_contiguous():
                raise ValueError(f"scratch must be a contiguous float32 [{M}, {self.SCRATCH_WIDTH}] tensor, got "
                                 f"{scratch.dtype} {tuple(scratch.shape)}")
        ic = torch.empty(M, 13, 3, dtype=torch.float32, device=self.device)
        rc = self.lib.codlad_ic_decode(C.byref(self.weights.struct), _lib.ptr(z_q.contiguous().float()),
                                       _lib.ptr(cg_z),
                                       _lib.ptr(cg_xyz.to(self.device).contiguous().float()),
                                       _lib.ptr(ptr), _lib.ptr(src), M, _lib.ptr(scratch), _lib.ptr(ic),
                                       _lib.stream_ptr(self.device))
        _lib.check(rc, "codlad_ic_decode")
        return ic

    def ic_to_xyz(self, ca_full, ic, info):
        """ca_full [B,L+2,3], ic [B,L,13,3], info = (permute, atom_idx, atom_orders) -> [B,n_atoms,3]."""
        _require_cuda(ic, "ic")
        B, L = ic.shape[0], ic.shape[1]
        orders, slot_to_out, n_atoms = info_tables(info, L, self.device)
        out = torch.empty(B, n_atoms, 3, dtype=torch.float32, device=self.device)
        rc = self.lib.codlad_ic_to_xyz(_lib.ptr(ca_full.to(self.device).contiguous().float()),
                                       _lib.ptr(ic.contiguous().float()), _lib.ptr(orders),
                                       _lib.ptr(slot_to_out), B, L, n_atoms, _lib.ptr(out),
                                       _lib.stream_ptr(self.device))
        _lib.check(rc, "codlad_ic_to_xyz")
        return out


    def ic_to_xyz_groups(self, groups, reuse=False):
        """groups: [(ca_full [B,L+2,3], ic [B,L,13,3], info)] of several proteins -> [xyz [B,n_atoms,3]] in ONE launch
        (codlad_ic_to_xyz_groups).  reuse: keep the descriptor table AND the output tensors of the previous call when the
        inputs sit at the same addresses (a job that is run again and again: the results of the earlier call are
        overwritten); default: a fresh table and fresh outputs per call (one small host-to-device copy)."""
        key = tuple((ca.data_ptr(), ic.data_ptr(), id(info[0]), tuple(ic.shape)) for ca, ic, info in groups)
        cache = getattr(self, "_xyz_groups", None) if reuse else None
        if cache is None or cache[0] != key:
            desc = (_lib.XyzGroup * len(groups))()
            outs, keep, row = [], [], 0
            for g, (ca, ic, info) in enumerate(groups):
                _require_cuda(ic, "ic")
                B, L = ic.shape[0], ic.shape[1]
                orders, s2o, n_atoms = info_tables(info, L, self.device)
                ca_d, ic_d = ca.to(self.device).contiguous().float(), ic.contiguous().float()
                assert ic_d.data_ptr() == ic.data_ptr() and ca_d.shape == (B, L + 2, 3)
                out = torch.empty(B, n_atoms, 3, dtype=torch.float32, device=self.device)
                d = desc[g]
                d.ca_full, d.ic, d.orders, d.slot_to_out, d.xyz_out = (ca_d.data_ptr(), ic_d.data_ptr(), orders.data_ptr(),
                                                                       s2o.data_ptr(), out.data_ptr())
                d.B, d.L, d.n_atoms, d.first_row = B, L, n_atoms, row
                row += B * L
                outs.append(out)
                keep += [ca_d, ic_d, orders, s2o]
            table = torch.frombuffer(bytearray(bytes(desc)), dtype=torch.uint8).to(self.device)
            cache = (key, table, outs, keep, row)
            if reuse:
                self._xyz_groups = cache
        _key, table, outs, _keep, rows = cache
        rc = self.lib.codlad_ic_to_xyz_groups(_lib.ptr(table), len(groups), rows, _lib.stream_ptr(self.device))
        _lib.check(rc, "codlad_ic_to_xyz_groups")
        return outs


_INFO_CACHE = {}


def info_tables(info, L, device):
    """(permute, atom_idx, atom_orders) of the reference (utils/protein_module.py:434-494) ->
    int32 device tables for codlad_ic_to_xyz.  Output atom p takes slot atom_idx[permute[p]]
    (utils/utils_ic.py:267)."""
    permute, atom_idx, orders = info
    key = (id(permute), id(atom_idx), id(orders), L, str(device))
    if key not in _INFO_CACHE:
        assert orders.shape == (10, L, 3), "atom_orders does not match the batch's residue count"
        n_atoms = int(permute.numel())
        slot = atom_idx.cpu()[permute.cpu()]
        assert int(slot.max()) < 14 * L and torch.unique(slot).numel() == n_atoms
        s2o = torch.full((14 * L,), -1, dtype=torch.int32)
        s2o[slot] = torch.arange(n_atoms, dtype=torch.int32)
        o32 = orders.to(torch.int32).contiguous()
        assert int(o32.min()) >= 0
        for i in range(10):  # slot i+4 may only reference earlier slots
            assert int(o32[i].max()) < 4 + i, "atom_orders references an atom that is not placed yet"
        if len(_INFO_CACHE) > 256:
            _INFO_CACHE.clear()
        _INFO_CACHE[key] = (o32.to(device), s2o.to(device), n_atoms, info)
    o, s, n, _keepalive = _INFO_CACHE[key]
    return o, s, n
