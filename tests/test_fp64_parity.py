"""GPU: everything after the edge features, node by node and channel by channel against a float64 reference.

The edge features are where the reference is ill-conditioned (tests/conditioning.py; compared edge by edge in
test_hip_parity.py::test_features_prepass_edge_by_edge).  Everything after them is smooth: given the SAME edge state and
adaLN vectors, the fp32 and the float64 oracle agree at every node.  So here the device's own h_E0 rows, neighbour lists
and adaLN row are read back and handed (cast up) to the float64 oracle, `oden.forward(h_E0=, mods=)`, and the device's
output is compared with that - no edge or node is left out.  Per node and per output channel, each channel scaled by its
own largest value over the case:

    err_hip[node, ch] <= c_mode x max(e_ref[ch], FLOOR)

e_ref[ch]: the fp32 oracle's largest per-node error against float64 in that channel, with the same substitutions, computed
in the test.  c_mode = 4 for f32 and f16x4 (the project's precedent for "as good as the reference's fp32",
test_ic_decode_and_xyz) and 16 for f16x3, whose operands carry 22 of 24 significand bits: two bits, a factor 4 on top.
FLOOR = 1e-6 of the channel's maximum.  The last decoder layer's h_V (job.hV) is held to the float64 `dec2_hV` tap by
the same rule, which takes final_kernel out of the picture when something is off.

Measured ratios max(err_hip / max(e_ref, FLOOR)) per mode and case: DESIGN.md section 2.
"""
import pytest
import torch

from codlad_amd import _lib, engine, synth
from codlad_amd.diffusion_and_flow.schedule import Tables, named_betas, space_timesteps
from codlad_amd.engine import Denoiser
from oracle import denoiser as oden
from tests import cases
from tests import conditioning as cond
from tests import ddim_cases as dc
from tests.test_hip_parity import NODE_QUAD_DEFAULT

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MODES = ("f16x3", "f16x4", "f32")
C_MODE = {"f32": 4.0, "f16x4": 4.0, "f16x3": 16.0}
FLOOR = 1e-6
EDGE_LENGTHS = (5, 31, 32, 33, 63, 64, 65, 200, 505)       # test_denoiser_forward_edge_lengths without the 2 048 chain
DDIM_FIRST_STEPS = ("fwd_fixed_small_L46", "fwd_ddim10_L46")


def _frames(prot):
    return [f for f in torch.from_numpy(prot["xyz_full"])[:, 1:-1]], torch.from_numpy(prot["z_full"])[1:-1]


def spec_of(name):
    """name -> dict(kind = which weights ("eps", "selfcond", "three"), xyz / z = the structures, members = the job's
    samples, x [n_nodes,3], t, x_self_cond or None)."""
    if name in cases.DENOISER_CASES:
        L, B, seed = cases.DENOISER_CASES[name]
        prot, _batch, x, t, _mask = cases.denoiser_inputs(L, B, seed)
        xyz, z = _frames(prot)
        return dict(kind="eps", xyz=xyz, z=[z] * B, members=list(range(B)), x=x.reshape(-1, 3), t=int(t[0]), x_sc=None)
    if name.startswith("len_"):
        L = int(name[4:])
        xyz, z = _frames(synth.make_protein(L, 70 + L, n_frames=1))
        return dict(kind="eps", xyz=xyz, z=[z], members=[0], x=synth.gaussian((1, L, 3), 5).reshape(-1, 3), t=777, x_sc=None)
    if name == "selfcond_L46_B2":
        L, B, seed, _T = cases.SELF_COND_CASES["L46_B2_T10"]
        prot, _batch, x, t, _mask = cases.denoiser_inputs(L, B, seed)
        xyz, z = _frames(prot)
        return dict(kind="selfcond", xyz=xyz, z=[z] * B, members=list(range(B)), x=x.reshape(-1, 3), t=int(t[0]),
                    x_sc=synth.gaussian((B, L, 3), 6000 + seed).reshape(-1, 3))
    if name == "flow_L46_B2":
        L, B, seed, times, _n = cases.FLOW_CASES["L46_B2"]
        prot, _batch, x, _t, _mask = cases.denoiser_inputs(L, B, seed)
        xyz, z = _frames(prot)
        return dict(kind="three", xyz=xyz, z=[z] * B, members=list(range(B)), x=x.reshape(-1, 3), t=times[1], x_sc=None)
    if name in DDIM_FIRST_STEPS:
        _rev, L, B, seed, respacing, _kw, _eta, _clip, kind, _hooks = dc.DDIM_CASES[name]
        prot, _batch, _x, _t, _mask = cases.denoiser_inputs(L, B, seed)
        xyz, z = _frames(prot)
        x_T, _eps = cases.loop_noise(dc.T, B, L, seed)
        t = Tables(named_betas("linear", 1000), space_timesteps(1000, respacing)).timestep_map[dc.T - 1]
        assert t == {"fwd_fixed_small_L46": 999, "fwd_ddim10_L46": 900}[name]
        return dict(kind=kind, xyz=xyz, z=[z] * B, members=list(range(B)), x=x_T.reshape(-1, 3), t=int(t), x_sc=None)
    if name == "ragged_46_87_87":        # the job of test_ragged_job_matches_separate_jobs: a member repeated
        (xa, za), (xb, zb) = (_frames(synth.make_protein(L, s, n_frames=1)) for L, s in ((46, 12), (87, 13)))
        return dict(kind="eps", xyz=xa + xb, z=[za, zb], members=[0, 1, 1], x=synth.gaussian((46 + 87 + 87, 3), 99), t=700,
                    x_sc=None)
    raise KeyError(name)


def state_dict_of(kind):
    return synth.denoiser_state_dict(cases.WEIGHT_SEED, flow=kind == "three", self_condition=kind == "selfcond")


_engines = {}


def engine_of(kind, mode):
    if (kind, mode) not in _engines:
        _engines[kind, mode] = Denoiser(state_dict_of(kind), DEV, precision=mode)
    return _engines[kind, mode]


def device_run(den, spec):
    """One forward on the device -> CPU tensors: out [n_nodes,C], hV [n_nodes,128] (the last decoder layer's), and
    what the oracle is given in place of its own: per structure the h_E0 rows [L,K,128] and E_idx [L,K], and the step's
    adaLN row [6016]."""
    st = den.prepare_structures(spec["xyz"], spec["z"])
    job = den.make_job(st, spec["members"])
    x_sc = None if spec["x_sc"] is None else spec["x_sc"].to(DEV)
    out = den.forward(job, spec["x"].to(DEV), spec["t"], x_self_cond=x_sc)
    torch.cuda.synchronize()
    rows = engine.edge_rows(st.h_E0, split=den.split_edge_state).cpu()
    idx = st.E_idx.cpu().long()
    hE0, E_idx = [], []
    for f, L in enumerate(st.lens):
        a, K = int(st.offsets[f]), min(64, L)
        hE0.append(rows[a:a + L, :K].clone())
        E_idx.append(idx[a:a + L, :K].clone())
        assert int(E_idx[-1].min()) >= 0 and int(E_idx[-1].max()) < L
    return dict(out=out.cpu(), hV=job.hV.cpu().clone(), hE0=hE0, E_idx=E_idx, mods=den.step_mods([spec["t"]])[0].cpu().clone())


def oracle_run(sd, spec, data, dtype):
    """The oracle in `dtype` from the device's edge state and adaLN row -> (out [n_nodes,C], dec2_hV [n_nodes,128])."""
    sdd = cond.to_dtype(sd, dtype)
    outs, hVs, off = [], [], 0
    for f in spec["members"]:
        L = spec["xyz"][f].shape[0]
        x = spec["x"][off:off + L][None].to(dtype)
        x_sc = None if spec["x_sc"] is None else spec["x_sc"][off:off + L][None].to(dtype)
        taps = {}
        out = oden.forward(sdd, x, None, spec["xyz"][f][None].to(dtype), spec["z"][f][None].long(),
                           torch.ones(1, L, dtype=torch.bool), taps=taps, x_self_cond=x_sc,
                           h_E0=(data["hE0"][f][None].to(dtype), data["E_idx"][f][None]), mods=data["mods"].to(dtype))
        outs.append(out[0])
        hVs.append(taps["dec2_hV"][0])
        off += L
    assert off == spec["x"].shape[0]
    return torch.cat(outs), torch.cat(hVs)


def ratios(spec, data, kind=None):
    """-> {"out": (worst ratio, node, channel, err, e_ref), "hV": ...}: err_hip / max(e_ref, FLOOR) at its largest."""
    sd = state_dict_of(spec["kind"])
    o64, h64 = oracle_run(sd, spec, data, torch.float64)
    o32, h32 = oracle_run(sd, spec, data, torch.float32)
    assert o64.dtype == torch.float64 and o32.dtype == torch.float32
    res = {}
    for what, got, r32, r64 in (("out", data["out"], o32, o64), ("hV", data["hV"], h32, h64)):
        e_ref = cond.node_channel_error(r32, r64).amax(0)              # [C]
        err = cond.node_channel_error(got, r64)                         # [n_nodes, C]
        ratio = err / e_ref.clamp_min(FLOOR)
        k = int(ratio.argmax())
        node, ch = divmod(k, ratio.shape[1])
        res[what] = (float(ratio.max()), node, ch, float(err[node, ch]), float(e_ref[ch]))
    return res


def check(name, mode, spec, data, label=""):
    assert bool(torch.isfinite(data["out"]).all())
    res = ratios(spec, data)
    msg = "; ".join(f"{what}: err/e_ref {r:.2f} at node {n} channel {c} (err {e:.2e}, e_ref {er:.2e})"
                    for what, (r, n, c, e, er) in res.items())
    print(f"fp64 parity {name} {mode}{label}: {msg}")
    for what, (r, _n, _c, _e, _er) in res.items():
        assert r <= C_MODE[mode], f"{name} {mode}{label}: {msg}"
    return res


# ---------------------------------------------------------------------------------------------------------------------
DEFAULT_CASES = (list(cases.DENOISER_CASES) + [f"len_{L}" for L in EDGE_LENGTHS]
                 + ["selfcond_L46_B2", "flow_L46_B2"] + list(DDIM_FIRST_STEPS) + ["ragged_46_87_87"])


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", DEFAULT_CASES)
def test_forward_after_features_against_float64(name, mode):
    """The kernels a job of this size takes as shipped: in the split-fp16 modes the small-job ones (msg_wide_kernel /
    upd_wide_kernel, node_kernel_q for the node updates, node_kernel_w for the projections), in f32 edge_kernel /
    node_kernel; final_kernel in all."""
    spec = spec_of(name)
    check(name, mode, spec, device_run(engine_of(spec["kind"], mode), spec))


@pytest.mark.parametrize("mode", ["f16x3", "f16x4"])
@pytest.mark.parametrize("name", list(cases.DENOISER_CASES) + list(DDIM_FIRST_STEPS))
def test_forward_after_features_against_float64_large_job_kernels(name, mode):
    """The same with the small-job switches off, so that the kernels of the headline job are held to float64 directly and
    not only through bit-identity with their small-job twins (the dispatch: enqueue_forward / launch_edge_now /
    launch_node in denoiser_forward.hip):
      CODLAD_OPT_EDGE_TILE_MAX_NODES = 0   no job is `tilewise`, no tile list is passed on: msg_kernel_h and (edge-update
                                           variant 0, the default) upd_kernel_h, one workgroup pass per node;
      CODLAD_OPT_NODE_QUAD_MAX_TILES = 0 and CODLAD_OPT_NODEQ_MAX_TILES = 0   neither node_kernel_q nor node_kernel_w:
                                           node_kernel_h, the streaming node update (four waves per workgroup at this
                                           size; the eight-wave instantiation, the XCD-chunked placement and the
                                           shipped thresholds themselves: tests/test_dispatch_thresholds.py).
    The f32 mode has one set of kernels whatever the switches say, so it is not run twice."""
    spec = spec_of(name)
    _lib.set_option(_lib.OPT_EDGE_TILE_MAX_NODES, 0)
    _lib.set_option(_lib.OPT_NODEQ_MAX_TILES, 0)
    _lib.set_option(_lib.OPT_NODE_QUAD_MAX_TILES, 0)
    try:
        data = device_run(engine_of(spec["kind"], mode), spec)
    finally:
        _lib.set_option(_lib.OPT_EDGE_TILE_MAX_NODES, 1 << 30)
        _lib.set_option(_lib.OPT_NODEQ_MAX_TILES, 256)
        _lib.set_option(_lib.OPT_NODE_QUAD_MAX_TILES, NODE_QUAD_DEFAULT)
    check(name, mode, spec, data, " large-job kernels")
