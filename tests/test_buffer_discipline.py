"""GPU: every device buffer is written before it is read, and nothing is written outside a buffer.

The parity tests hold the arithmetic.  They cannot see a kernel that reads a slot nothing has written (the memory of a
test box is zeros or the finite leftovers of the previous test) or one that writes a few rows past its buffer (the
caching allocator's slack takes it).  tests/memcheck.py makes both visible, and every case here follows one rule:

  run it once as it is, then three more times under memcheck.patched_allocations with the fills "zero", "nan" and
  "big" - the engine objects (Denoiser / Decoder / Encoder) built INSIDE the patch, the caller's own inputs and outputs
  in memcheck.guarded buffers - and require
    1. the same bits in all four runs, for every DEFINED output element (each case says which those are);
    2. every red zone intact (memcheck.zones_intact names the buffer and the byte);
    3. every status word 0: NaN poison must not reach the non-finite sentinel;
    4. no NaN where the plain run has none.

Defined elements.  E_idx / h_E0 / E1: the slots k < K = min(64, L) of a node, read through engine.edge_rows (without
the split-fp16 sum: the raw words, permuted); features_kernel writes nothing else when L < 64.  The error norm's table:
word 0 (the later words are per-block partial sums, as many as the launch had blocks).  The results of an EMPTY sample
(sample_off[s] == sample_off[s + 1]): not written, by the header's contract - the case puts a sentinel there and finds it again.
Scratch buffers (ode scratch, x_t / xt / ut of the fused loss loops, the decoder's, the metrics') are zone-checked only.

Poison never becomes a bad index: integer buffers hold 0 or 1 only, and every indexed table of every case has two
entries or more.  Overruns of up to 64 KiB stay inside the guarded allocation.  So no case can fault by construction.

Measured figures and what the cases cannot see: DESIGN.md section 2, "Write before read, writes in bounds".
"""
import ctypes as C

import numpy as np
import pytest
import torch

from codlad_amd import _lib, engine, synth
from codlad_amd.diffusion_and_flow import ode
from codlad_amd.engine import Denoiser
from tests import cases
from tests import memcheck as mc
from tests.test_hip_parity import EDGE_UPD_DEFAULT, EDGE_WIDE_DEFAULT, NODE_QUAD_DEFAULT, tables

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MODES = ("f16x3", "f16x4", "f32")
T = 4
BIG = 1 << 20

OPTION_DEFAULTS = {"OPT_NODEQ_MAX_TILES": 256, "OPT_NODE_QUAD_MAX_TILES": NODE_QUAD_DEFAULT, "OPT_EDGE_TILE_MAX_NODES": 1 << 30,
                   "OPT_EDGE_WIDE_MAX_TILES": EDGE_WIDE_DEFAULT, "OPT_EDGE_UPD_VARIANT": EDGE_UPD_DEFAULT, "OPT_EDGE_PAIR": 1,
                   "OPT_EDGE_CUS": 0}
# name -> the options that differ from the defaults.  Edge kernels: per node (EDGE_TILE_MAX_NODES 0; pairing of short last
# halves on / off; EDGE_UPD_VARIANT 1 and 2 = upd1_kernel_h), per 32-edge tile with one wave (EDGE_WIDE_MAX_TILES 0) or four.
# EDGE_CUS 8: a persistent grid of 8 workgroups, so that a wave walks several nodes of these small jobs and meets pairs.
# Node kernels: streaming (NODEQ 0), eight waves per tile (NODEQ big, QUAD 0), four waves per tile (both big).
KERNEL_SETS = {
    "default": {},
    "pernode_pair_stream": {"OPT_EDGE_TILE_MAX_NODES": 0, "OPT_EDGE_CUS": 8, "OPT_NODEQ_MAX_TILES": 0, "OPT_NODE_QUAD_MAX_TILES": 0},
    "pernode_nopair_wide8": {"OPT_EDGE_TILE_MAX_NODES": 0, "OPT_EDGE_PAIR": 0, "OPT_NODEQ_MAX_TILES": BIG, "OPT_NODE_QUAD_MAX_TILES": 0},
    "pernode_upd1_quad": {"OPT_EDGE_TILE_MAX_NODES": 0, "OPT_EDGE_CUS": 8, "OPT_EDGE_UPD_VARIANT": 1, "OPT_NODEQ_MAX_TILES": BIG,
                          "OPT_NODE_QUAD_MAX_TILES": BIG},
    "pernode_upd2_nopair": {"OPT_EDGE_TILE_MAX_NODES": 0, "OPT_EDGE_UPD_VARIANT": 2, "OPT_EDGE_PAIR": 0},
    "tile1_wide8": {"OPT_EDGE_TILE_MAX_NODES": BIG, "OPT_EDGE_WIDE_MAX_TILES": 0, "OPT_NODEQ_MAX_TILES": BIG, "OPT_NODE_QUAD_MAX_TILES": 0},
    "tile1_stream": {"OPT_EDGE_TILE_MAX_NODES": BIG, "OPT_EDGE_WIDE_MAX_TILES": 0, "OPT_NODEQ_MAX_TILES": 0, "OPT_NODE_QUAD_MAX_TILES": 0},
    "tile4_quad": {"OPT_EDGE_TILE_MAX_NODES": BIG, "OPT_EDGE_WIDE_MAX_TILES": BIG, "OPT_NODEQ_MAX_TILES": BIG, "OPT_NODE_QUAD_MAX_TILES": BIG},
}


class kernel_set:
    """The library's tuning switches set for a block and put back to the shipped values after it."""

    def __init__(self, name):
        self.options = KERNEL_SETS[name]

    def __enter__(self):
        for k, v in self.options.items():
            _lib.set_option(getattr(_lib, k), v)

    def __exit__(self, *exc):
        for k, v in OPTION_DEFAULTS.items():
            _lib.set_option(getattr(_lib, k), v)


# ------------------------------------------------------------------------------------------------- the rule --
def hold(label, case):
    """case(g) -> ({name: tensor of DEFINED elements}, [status words]); g(t, name) puts a caller's tensor on the device:
    plainly in the first run, into a guarded buffer in the three patched ones."""
    def plain(t, name=None):
        return t.to(DEV)

    ref, status = case(plain)
    torch.cuda.synchronize()
    ref = {k: v.detach().cpu().clone() for k, v in ref.items()}
    assert [int(s) for s in status] == [0] * len(status), f"{label}: status {status} in the plain run"
    for fill in mc.FILLS:
        mc.release()
        try:
            with mc.patched_allocations(fill, devices=["cuda"]):
                got, status = case(lambda t, name=None: mc.guard_copy(t, fill, name, device=DEV))
                torch.cuda.synchronize()
                status = [int(s) for s in status]
                got = {k: v.detach().cpu().clone() for k, v in got.items()}
            assert mc.registered() > 0, f"{label}: nothing was allocated under the patch"
            mc.zones_intact()
        finally:
            mc.release()
        assert status == [0] * len(status), f"{label} [{fill}]: status words {status}"
        assert sorted(got) == sorted(ref), label
        for k in ref:
            a, b = ref[k], got[k]
            if a.is_floating_point():
                fresh = int((torch.isnan(b) & ~torch.isnan(a)).sum())
                assert fresh == 0, f"{label} [{fill}]: {k} has {fresh} NaN(s) the plain run has not"
            if not mc.same_bits(a, b):
                bad = (a.contiguous().view(-1).view(mc.INT_VIEW[a.element_size()]) !=
                       b.contiguous().view(-1).view(mc.INT_VIEW[b.element_size()])).nonzero().reshape(-1)
                raise AssertionError(f"{label} [{fill}]: {k} {tuple(a.shape)} differs from the plain run in {bad.numel()} "
                                     f"element(s), first at flat index {int(bad[0])}: {a.view(-1)[bad[0]]!r} plain, "
                                     f"{b.view(-1)[bad[0]]!r} poisoned")


def statuses(job):
    """The status word of a job and of every sub-job it has made (parts of a split job, timestep groups)."""
    jobs = [job] + [p for parts in job._parts.values() for p, _i in parts] + [p for p, _i in getattr(job, "_t_groups", {}).values()]
    return [int(j.status.item()) for j in jobs]


# ----------------------------------------------------------------------------------------------- geometries --
_sds = {}


def state_dict_of(kind):
    if kind not in _sds:
        _sds[kind] = synth.denoiser_state_dict(cases.WEIGHT_SEED, flow=kind == "three", self_condition=kind == "selfcond")
    return _sds[kind]


def _frame(L, seed):
    p = synth.make_protein(L, seed, n_frames=1)
    return torch.from_numpy(p["xyz_full"])[0, 1:-1], torch.from_numpy(p["z_full"])[1:-1]


_geo = {}


def geometry(name):
    """name -> (xyz list, z list, members, x [n_nodes, 3]).
    edge_lengths: K <= 32 (5, 31), K = 32, a partial second half (33, 47), K = 64 (64, 65, 87), structure 2 used by two
                  members; 396 nodes: the last 32-node tile is partial.
    n15:          the 15-node job of tests/test_ode_fp64_parity.py (three members of one length-5 structure).
    l5_33_65:     the loops' second job: 103 nodes."""
    if name not in _geo:
        if name == "n15":
            xyz, z = _frame(5, 75)
            _geo[name] = ([xyz], [z], [0, 0, 0], synth.gaussian((15, 3), 1500))
        else:
            lens, members, seed = {"edge_lengths": ((5, 31, 32, 33, 47, 64, 65, 87), list(range(8)) + [2], 300),
                                   "l5_33_65": ((5, 33, 65), [0, 1, 2], 320)}[name]
            fr = [_frame(L, seed + i) for i, L in enumerate(lens)]
            n = sum(lens[m] for m in members)
            _geo[name] = ([f[0] for f in fr], [f[1] for f in fr], members, synth.gaussian((n, 3), 1700 + n))
    return _geo[name]


def feature_rows(st):
    """The defined part of the step-invariant buffers: per structure the slots k < K of E_idx, h_E0 and E1."""
    out = {}
    h0 = engine.edge_rows(st.h_E0)
    e1 = None if st.E1 is None else engine.edge_rows(st.E1)
    for f, L in enumerate(st.lens):
        a, K = int(st.offsets[f]), min(engine.KNN, L)
        out[f"E_idx[{f}]"] = st.E_idx[a:a + L, :K].clone()
        out[f"h_E0[{f}]"] = h0[a:a + L, :K].clone()
        if e1 is not None:
            out[f"E1[{f}]"] = e1[:, a:a + L, :K].clone()
    return out


# ------------------------------------------------------------------------- 1. denoiser forward and features --
def forward_case(kind, mode, combos):
    """One engine, and for every (geometry, hoist_layer0) of `combos` fresh structures, a job and one forward."""
    t = 0.37 if kind == "three" else 600

    def case(g):
        den = Denoiser(state_dict_of(kind), DEV, precision=mode)
        res, stat = {}, []
        for geo, hoist in combos:
            xyz, z, members, x = geometry(geo)
            x_sc = g(synth.gaussian(tuple(x.shape), 1801), "x_self_cond") if kind == "selfcond" else None
            st = den.prepare_structures(xyz, z, hoist_layer0=hoist)
            job = den.make_job(st, members)
            out = den.forward(job, g(x, "x"), t, x_self_cond=x_sc, check=False)
            res.update({f"{geo}/{hoist}/{k}": v for k, v in dict(feature_rows(st), out=out, hV=job.hV).items()})
            stat += statuses(job)
        return res, stat
    return case


FORWARD_COMBOS = [(geo, hoist) for geo in ("edge_lengths", "n15") for hoist in (True, False)]


@pytest.mark.parametrize("kset", list(KERNEL_SETS))
@pytest.mark.parametrize("mode", MODES)
def test_forward_and_features(mode, kset):
    """Defined: the model output, job.hV (the last decoder layer's node state) and the k < K feature slots."""
    with kernel_set(kset):
        hold(f"forward eps {mode} {kset}", forward_case("eps", mode, FORWARD_COMBOS))


@pytest.mark.parametrize("kind", ["selfcond", "three"])
@pytest.mark.parametrize("mode", MODES)
def test_forward_of_the_self_conditioned_and_the_flow_model(mode, kind):
    for kset in ("default", "tile4_quad"):
        with kernel_set(kset):
            hold(f"forward {kind} {mode} {kset}", forward_case(kind, mode, FORWARD_COMBOS[::2]))


# ------------------------------------------------------------------------------------------------ 2. sub-jobs --
POISON_WORD = {"zero": 0, "nan": 0x7FC07FC0, "big": 0x7BFF7BFF}


@pytest.mark.parametrize("mode", ["f16x3", "f32"])
def test_sub_jobs_keep_to_their_range_of_the_parents_edge_state(mode):
    """job.parts(2): the two sub-jobs lie side by side in the parent's hE.  With the WHOLE parent hE poisoned, running one
    part leaves every word of the other's range as it was, and each part's output and node state are those of the same
    samples run as a job of their own (plain run, and poisoned under each fill)."""
    xyz, z, members, x = geometry("edge_lengths")

    def case(g):
        den = Denoiser(state_dict_of("eps"), DEV, precision=mode)
        st = den.prepare_structures(xyz, z)
        job = den.make_job(st, members)
        parts = job.parts(2)
        xd = g(x, "x")
        res, stat = {}, []
        n0 = parts[0][0].n_nodes
        ranges = [(0, n0), (n0, n0 + parts[1][0].n_nodes)]
        assert ranges[1][1] == job.n_nodes
        words = job.hE.view(torch.int32)
        for p in (0, 1):
            sub, idx = parts[p]
            words.fill_(0x7FC07FC0)                         # NaN, whatever the run's fill: the other part's range must keep it
            out = den.forward(sub, xd[idx].contiguous(), 600, check=False)
            a, b = ranges[1 - p]
            res[f"other_range_after_part{p}"] = (words[a:b] != 0x7FC07FC0).sum().reshape(1)
            own = den.make_job(st, [members[m] for m in range(p, len(members), 2)])
            alone = den.forward(own, xd[idx].contiguous(), 600, check=False)
            res[f"out{p}"], res[f"hV{p}"] = out, sub.hV.clone()
            res[f"out{p}_minus_alone"] = (out.view(torch.int32) != alone.view(torch.int32)).sum().reshape(1)
            res[f"hV{p}_minus_alone"] = (sub.hV.view(torch.int32) != own.hV.view(torch.int32)).sum().reshape(1)
            stat += statuses(own)
        return res, stat + statuses(job)

    def checked(g):
        res, stat = case(g)
        for k, v in res.items():
            if k.startswith("other_range") or k.endswith("_minus_alone"):
                assert int(v) == 0, f"{k}: {int(v)} word(s) differ"
        return res, stat
    hold(f"sub-jobs {mode}", checked)


# ---------------------------------------------------------------------------------------- 3. loops and losses --
def _loop_inputs(geo):
    xyz, z, members, x = geometry(geo)
    n = x.shape[0]
    return xyz, z, members, x, synth.gaussian((T, n, 3), 1900 + n), synth.gaussian((n, 3), 1950 + n) * 0.5


SAMPLERS = {
    # name -> (model kind, Denoiser.sample's kind, takes noise, the coefficient table of tables(T) or None = the default, pinned)
    "ddpm_learned": ("eps", "ddpm", True, None, False),
    "ddpm_fixed": ("three", "ddpm", True, lambda tb: tb.step_coefficients(var_type="fixed_small"), False),
    "ddpm_selfcond": ("selfcond", "ddpm", True, None, False),
    "ddpm_pinned": ("eps", "ddpm", True, None, True),
    "ddim": ("eps", "ddim", True, None, False),
    "ddim_selfcond": ("selfcond", "ddim", True, None, False),
    "ddim_reverse": ("eps", "ddim_reverse", False, None, False),
    "dpmpp": ("eps", "dpmpp", False, None, False),
}


@pytest.mark.parametrize("streams", [1, 2])
@pytest.mark.parametrize("name", list(SAMPLERS))
def test_sampling_loops(name, streams):
    """Defined: the whole returned state.  x_start (the self-conditioning input and the multistep history) is made by
    torch.empty_like inside the engine and is unwritten at the first step, which must not read it."""
    kind, skind, noisy, coef_of, pinned = SAMPLERS[name]
    tb = tables(T)
    for geo in ("n15", "l5_33_65"):
        xyz, z, members, x, eps, x0 = _loop_inputs(geo)
        mask = (torch.arange(x.shape[0]) % 3 == 0).to(torch.uint8)

        def case(g):
            den = Denoiser(state_dict_of(kind), DEV, precision="f16x3")
            job = den.make_job(den.prepare_structures(xyz, z), members)
            pin = (g(x0, "pin_x0"), g(mask, "pin_mask")) if pinned else None
            out = den.sample(job, g(x, "x_T"), g(eps, "noise") if noisy else None, tb, check=False, streams=streams, pin=pin,
                             coef=None if coef_of is None else coef_of(tb), kind=skind)
            return dict(x0=out), statuses(job)
        hold(f"sample {name} {geo} streams={streams}", case)


@pytest.mark.parametrize("method,streams", [("euler", 1), ("euler", 2), ("rk4", 1), ("rk4", 2), ("dopri5", 1)])
def test_ode_loops(method, streams):
    """Defined: the whole trajectory [3, n_nodes, 3].  (dopri5 always runs on one stream.)"""
    for geo in ("n15", "l5_33_65"):
        xyz, z, members, x, _eps, _x0 = _loop_inputs(geo)

        def case(g):
            den = Denoiser(state_dict_of("three"), DEV, precision="f16x3")
            job = den.make_job(den.prepare_structures(xyz, z), members)
            traj, stats = den.sample_ode(job, g(x, "y0"), [0.0, 0.4, 1.0], method=method, rtol=1e-4, atol=1e-4, check=False,
                                         streams=streams)
            counts = torch.tensor([stats["n_eval"], stats["n_accept"], stats["n_reject"]])
            return dict(traj=traj, counts=counts), statuses(job)
        hold(f"sample_ode {method} {geo} streams={streams}", case)


@pytest.mark.parametrize("entry", ["loss_terms", "loss_terms_per_sample_t", "bpd_1", "bpd_2", "fm_loss_terms", "fm_loss_terms_per_sample_t",
                                   "fm_loss_sweep_1", "fm_loss_sweep_2"])
def test_losses(entry):
    """Defined: every returned table (each sample has nodes, so each of its terms is written)."""
    tb = tables(T)
    flow = entry.startswith("fm")
    for geo in ("n15", "l5_33_65"):
        xyz, z, members, x, eps, x0 = _loop_inputs(geo)

        def case(g):
            den = Denoiser(state_dict_of("three" if flow else "eps"), DEV, precision="f16x3")
            job = den.make_job(den.prepare_structures(xyz, z), members)
            xs = g(x0, "x_start")
            if entry.startswith("loss_terms"):
                t = [1, 3, 1] if entry.endswith("per_sample_t") else 2
                res = den.loss_terms(job, xs, t, g(eps[0], "noise"), tb, check=False, want_model_out=True)
            elif entry.startswith("bpd"):
                res = den.bpd(job, xs, g(eps, "noise"), tb, streams=int(entry[-1]), check=False)
            elif entry.startswith("fm_loss_terms"):
                t = [0.2, 0.9, 0.2] if entry.endswith("per_sample_t") else 0.55
                res = den.fm_loss_terms(job, xs, t, kind="icfm", sigma=0.1, x0=g(x, "x0"), eps=g(eps[0], "eps"), check=False,
                                        want_model_out=True)
            else:
                res = den.fm_loss_sweep(job, xs, [0.1, 0.5, 0.9], kind="vp", sigma=0.1, x0=g(x, "x0"), eps=g(eps[:3], "eps"),
                                        streams=int(entry[-1]), check=False)
            return dict(res), statuses(job)
        hold(f"{entry} {geo}", case)


def test_loops_through_the_c_abi_with_the_tests_own_buffers():
    """Denoiser.sample / sample_ode make the loops' in / out state by .clone() inside ATen, which the patch does not see:
    here x, noise, x_start, the trajectory and the scratch are the test's own guarded buffers (the 15-node job, f16x3).
    Defined: x and x_start after the loop (every step writes every node's pred_xstart), the whole trajectory."""
    xyz, z, members, x, eps, _x0 = _loop_inputs("n15")
    n = x.shape[0]
    tb = tables(T)

    def diffusion(entry):
        def case(g):
            den = Denoiser(state_dict_of("eps"), DEV, precision="f16x3")
            job = den.make_job(den.prepare_structures(xyz, z), members)
            coef = {"codlad_sample_loop": tb.step_coefficients, "codlad_ddim_loop": tb.ddim_coefficients,
                    "codlad_dpm_loop": tb.dpm_solver_coefficients}[entry]()
            mode = int(coef[0, 7])
            xd, mods, coef_d = g(x, "x"), den.step_mods(tb.timestep_map), g(torch.from_numpy(coef), "coef")
            x_start = torch.empty(n, 3, dtype=torch.float32, device=DEV)           # guarded and poisoned under the patch
            noise = g(eps, "noise")
            p = _lib.ptr
            if entry == "codlad_sample_loop":
                den._run(entry, job.desc(), p(xd), p(x_start), p(noise), p(mods), p(coef_d), T)
            elif entry == "codlad_ddim_loop":
                den._run(entry, job.desc(), p(xd), p(x_start), p(noise), p(mods), p(coef_d), T, mode, 0, None, None)
            else:
                den._run(entry, job.desc(), p(xd), p(x_start), p(mods), p(coef_d), T, mode, None, None)
            return dict(x=xd, x_start=x_start), statuses(job)
        return case

    for entry in ("codlad_sample_loop", "codlad_ddim_loop", "codlad_dpm_loop"):
        hold(entry, diffusion(entry))

    for method in ("euler", "midpoint", "rk4"):
        def case(g):
            den = Denoiser(state_dict_of("three"), DEV, precision="f16x3")
            job = den.make_job(den.prepare_structures(xyz, z), members)
            ts = [0.0, 0.4, 1.0]
            dts = [b - a for a, b in zip(ts, ts[1:])]
            mods = den.step_mods(ode.stage_times(method, ts))
            y0 = g(x, "y0")
            traj = torch.empty(len(ts), n, 3, dtype=torch.float32, device=DEV)
            scratch = torch.empty(5, n, 3, dtype=torch.float32, device=DEV)
            den._run("codlad_ode_loop", job.desc(), _lib.ptr(y0), _lib.ptr(traj), _lib.ptr(mods), _lib.ODE_METHODS[method],
                     (C.c_float * len(dts))(*dts), len(dts), _lib.ptr(scratch))
            return dict(traj=traj, y0=y0), statuses(job)
        hold(f"codlad_ode_loop {method}", case)


# -------------------------------------------------------------------------- 4. stand-alone element-wise entries --
ELEMENTWISE_NODES = (15, 86)          # 45 elements, and 258: two elements in a second 256-thread block


def _vec(n, seed, scale=1.0):
    return synth.gaussian((n, 3), seed) * scale


@pytest.mark.parametrize("n", ELEMENTWISE_NODES)
def test_step_entries(n):
    """ddpm_update, ddpm_pred_xstart, ddpm_posterior_step, ddim_step, dpm_step through their Python entry points (the
    outputs are the engine's torch.empty_like).  Defined: every output, whole."""
    tb = tables(T)
    x, out6, out3, noise, grad, px, prev = (_vec(n, 2000 + n), synth.gaussian((n, 6), 2001 + n), _vec(n, 2002 + n), _vec(n, 2003 + n),
                                            _vec(n, 2004 + n, 0.1), _vec(n, 2005 + n, 0.5), _vec(n, 2006 + n, 0.5))
    step, ddim, dpm = tb.step_coefficients(clip_denoised=True), tb.ddim_coefficients(eta=0.5), tb.dpm_solver_coefficients()
    fixed = tb.step_coefficients(var_type="fixed_small")
    assert dpm[2, 4] != 0 and dpm[T - 1, 4] == 0

    def case(g):
        den = Denoiser(state_dict_of("eps"), DEV, precision="f16x3")
        a = [g(t, nm) for t, nm in ((x, "x"), (out6, "model_out6"), (out3, "model_out3"), (noise, "noise"), (grad, "grad"),
                                    (px, "pred_xstart"), (prev, "prev_xstart"))]
        xd, o6, o3, nz, gr, pxd, pv = a
        res = {}
        res["upd"], res["upd_xs"] = den.ddpm_update(xd, o6, nz, tb, 2, return_x_start=True)
        res["upd0"] = den.ddpm_update(xd, o6, nz, tb, 0)
        res["pred"] = Denoiser.ddpm_pred_xstart(xd, o6, step[2])
        res["pred_fixed"] = Denoiser.ddpm_pred_xstart(xd, o3, fixed[2])
        res["post"], res["post_xs"] = Denoiser.ddpm_posterior_step(xd, pxd, o6, nz, step[2], grad=gr)
        res["post_f"], res["post_f_xs"] = Denoiser.ddpm_posterior_step(xd, pxd, o3, nz, fixed[1], fixed_variance=0.01)
        res["ddim"], res["ddim_xs"] = Denoiser.ddim_step(xd, pxd, nz, ddim[2], grad=gr)
        res["ddim_r"], res["ddim_r_xs"] = Denoiser.ddim_step(xd, pxd, None, tb.ddim_coefficients(reverse=True)[1], reverse=True)
        res["dpm"], res["dpm_xs"] = Denoiser.dpm_step(xd, pxd, pv, dpm[2], grad=gr)
        res["dpm_first"], res["dpm_first_xs"] = Denoiser.dpm_step(xd, pxd, None, dpm[T - 1])
        return res, []
    hold(f"step entries n={n}", case)


SENTINEL = -7.0


def _offsets(n):
    """Three samples over n nodes, the middle one EMPTY (the C ABI skips it: its results are not written)."""
    a = n // 3
    return [0, a, a, n]


@pytest.mark.parametrize("n", ELEMENTWISE_NODES)
def test_per_sample_entries_through_the_c_abi_with_an_empty_sample(n):
    """q_sample, q_posterior, vb_terms, prior_bpd, fm_path, fm_terms with sample offsets [0, a, a, n]: the Python entry
    points refuse an empty sample, the C ABI skips it.  Defined: the per-node outputs whole (every node belongs to a
    sample with nodes), the per-sample ones at samples 0 and 2; the empty sample's slot is not written, so it is given a
    sentinel in every run and must still hold it afterwards."""
    tb = tables(T)
    coef = torch.from_numpy(np.ascontiguousarray(tb.loss_coefficients(), dtype=np.float32))
    xs, nz, xt, out6, ut = _vec(n, 2100 + n, 0.5), _vec(n, 2101 + n), _vec(n, 2102 + n), synth.gaussian((n, 6), 2103 + n), _vec(n, 2104 + n)
    off = torch.tensor(_offsets(n), dtype=torch.int32)
    tvec, tfl = torch.tensor([1, 3, 0], dtype=torch.int32), torch.tensor([0.2, 0.5, 0.9], dtype=torch.float32)
    lib, p = _lib.lib(), _lib.ptr

    def case(g):
        st = _lib.stream_ptr(torch.device(DEV))
        xs_d, nz_d, xt_d, o6, ut_d, off_d, cf, tv, tf = (g(t, nm) for t, nm in (
            (xs, "x_start"), (nz, "noise"), (xt, "x_t"), (out6, "model_out"), (ut, "ut"), (off, "sample_off"), (coef, "coef"),
            (tvec, "t_of_sample"), (tfl, "t_of_sample_f")))
        f = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=DEV)      # noqa: E731
        res = {}
        for name, fn, b in (("q_sample", lib.codlad_q_sample, nz_d), ("q_posterior", lib.codlad_q_posterior, xt_d)):
            for tag, tdev in (("shared", None), ("per_sample", tv)):
                o, v, lv = f(n, 3), f(n, 3), f(n, 3)
                _lib.check(fn(p(xs_d), p(b), p(cf), T, p(off_d), 3, p(tdev), 2, p(o), p(v), p(lv), st), name)
                res.update({f"{name}_{tag}": o, f"{name}_{tag}_var": v, f"{name}_{tag}_logvar": lv})
        per = {k: f(3) for k in Denoiser.LOSS_KEYS}
        for v in per.values():
            v[1] = SENTINEL
        per["pred_xstart"] = f(n, 3)
        terms = _lib.LossTerms()
        for k, v in per.items():
            setattr(terms, k, v.data_ptr())
        _lib.check(lib.codlad_vb_terms(p(o6), p(xs_d), p(xt_d), p(nz_d), p(cf), T, p(off_d), 3, p(tv), 0, C.byref(terms), st),
                   "codlad_vb_terms")
        res.update({f"vb_{k}": v for k, v in per.items()})
        prior = f(3)
        prior[1] = SENTINEL
        _lib.check(lib.codlad_prior_bpd(p(xs_d), p(cf), T, p(off_d), 3, p(prior), st), "codlad_prior_bpd")
        res["prior_bpd"] = prior
        for kind, kid in _lib.FM_KINDS.items():
            for tag, tdev in (("shared", None), ("per_sample", tf)):
                o, u = f(n, 3), f(n, 3)
                _lib.check(lib.codlad_fm_path(p(xt_d), p(xs_d), p(nz_d), p(off_d), 3, p(tdev), 0.55, kid, 0.1, p(o), p(u), st),
                           "codlad_fm_path")
                res.update({f"fm_{kind}_{tag}_xt": o, f"fm_{kind}_{tag}_ut": u})
        fm = {k: f(3) for k in Denoiser.FM_LOSS_KEYS}
        for v in fm.values():
            v[1] = SENTINEL
        out = _lib.FmLossOut()
        for k, v in fm.items():
            setattr(out, k, v.data_ptr())
        _lib.check(lib.codlad_fm_terms(p(xt_d), p(ut_d), p(off_d), 3, C.byref(out), st), "codlad_fm_terms")
        res.update({f"fm_{k}": v for k, v in fm.items()})
        for k, v in res.items():
            if v.shape == (3,):
                assert float(v[1]) == SENTINEL, f"{k}: the empty sample's slot was written ({float(v[1])!r})"
        return res, []
    hold(f"per-sample entries n={n}", case)


@pytest.mark.parametrize("n", ELEMENTWISE_NODES)
def test_per_sample_entries_through_python(n):
    """The same entries through Denoiser's static wrappers, whose outputs are the engine's own torch.empty: q_sample,
    q_posterior, vb_terms, fm_path, fm_terms.  Defined: everything returned."""
    tb = tables(T)
    coef = tb.loss_coefficients()
    lens = [n // 3, n - n // 3]
    xs, nz, xt, out6, ut = _vec(n, 2100 + n, 0.5), _vec(n, 2101 + n), _vec(n, 2102 + n), synth.gaussian((n, 6), 2103 + n), _vec(n, 2104 + n)

    def case(g):
        xs_d, nz_d, xt_d, o6, ut_d = (g(t, nm) for t, nm in ((xs, "x_start"), (nz, "noise"), (xt, "x_t"), (out6, "model_out"), (ut, "ut")))
        res = {}
        for kind, b in (("q_sample", nz_d), ("q_posterior", xt_d)):
            for tag, t in (("shared", 2), ("per_sample", [1, 3])):
                for nm, v in zip(("", "_var", "_logvar"), Denoiser.q_affine(kind, xs_d, b, lens, t, coef)):
                    res[f"{kind}_{tag}{nm}"] = v
        res.update({f"vb_{k}": v for k, v in Denoiser.vb_terms(o6, xs_d, xt_d, nz_d, lens, [3, 0], coef).items()})
        res.update({f"vb_nonoise_{k}": v for k, v in Denoiser.vb_terms(o6, xs_d, xt_d, None, lens, 1, coef).items()})
        for kind in _lib.FM_KINDS:
            res[f"fm_{kind}_xt"], res[f"fm_{kind}_ut"] = Denoiser.fm_path(kind, 0.1, xt_d, xs_d, nz_d, lens, [0.2, 0.9])
        res.update({f"fm_{k}": v for k, v in Denoiser.fm_terms(xt_d, ut_d, lens).items()})
        return res, []
    hold(f"per-sample wrappers n={n}", case)


@pytest.mark.parametrize("n", ELEMENTWISE_NODES)
def test_ode_combine_and_error_norm(n):
    """ode.combine with one, four and seven slopes (its output: the package's torch.empty_like), and codlad_ode_error_norm
    into the test's own table.  Defined: the combination whole; word 0 of the norm table (words 1 .. blocks hold the
    launch's per-block partial sums, the rest of the 257 nothing)."""
    y, ks = _vec(n, 2200 + n), [_vec(n, 2201 + n + j) for j in range(7)]
    err, y1 = _vec(n, 2210 + n, 1e-5), _vec(n, 2211 + n)
    cf = [0.3, -0.2, 0.15, 0.7, -0.4, 0.05, 0.11]

    def case(g):
        yd, kd, ed, y1d = g(y, "y"), [g(k, f"k{j}") for j, k in enumerate(ks)], g(err, "err"), g(y1, "y1")
        res = {f"combine{m}": ode.combine(yd, kd[:m], cf[:m], 0.125) for m in (1, 4, 7)}
        norm = torch.empty(_lib.ODE_NORM_WORDS, dtype=torch.float64, device=DEV)
        rc = _lib.lib().codlad_ode_error_norm(_lib.ptr(ed), _lib.ptr(yd), _lib.ptr(y1d), ed.numel(), C.c_float(1e-5), C.c_float(1e-5),
                                              _lib.ptr(norm), _lib.stream_ptr(torch.device(DEV)))
        _lib.check(rc, "codlad_ode_error_norm")
        res["norm"] = norm[:1]
        return res, []
    hold(f"ode combine / norm n={n}", case)


@pytest.mark.parametrize("mode", MODES)
def test_step_mods(mode):
    """The adaLN rows of integer and of fractional times.  Defined: every row, whole."""
    def case(g):
        den = Denoiser(state_dict_of("three"), DEV, precision=mode)
        return dict(ints=den.step_mods([0, 250, 999]), one=den.step_mods([7]), floats=den.step_mods([0.0, 0.37, 1.0]),
                    whole_as_float=den.step_mods([3, 4], as_float=True)), []
    hold(f"step_mods {mode}", case)


# ------------------------------------------------------------------------------- 5. decoder, encoder, metrics --
DECODER_SMALLEST = {"N6": "N6_L46_B3", "K3": "K3_L60_B2", "K4": "K4_L129_B1"}       # cases.DECODER_CASES per VAE type


@pytest.mark.parametrize("vae_type", list(DECODER_SMALLEST))
def test_decoder_entries(vae_type):
    """Decoder.vq, ic_decode without a caller's scratch under both DEC_EDGE_VARIANTs, build_csr (codlad_cg_graph), ic_decode
    over that graph, ic_to_xyz and ic_to_xyz_groups.  Defined: idx / z_q / latent, ic, the CSR's ptr whole and src up to
    ptr[-1], the coordinates; the decoder's scratch is the engine's own torch.empty and is zone-checked."""
    from codlad_amd.engine import Decoder
    from tests import decoder_cases as dc
    L, B, seed, _v = cases.DECODER_CASES[DECODER_SMALLEST[vae_type]]
    prot, batch, latent, dataname = cases.decoder_inputs(L, B, seed, vae_type)
    mean, std = synth.norm_stats(dataname, vae_type)
    case_ = dc.existing_case(DECODER_SMALLEST[vae_type])
    ca_full = batch["OG_CG_nxyz"].reshape(-1, L + 2, 4)[:, :, 1:].contiguous()
    x_norm = ((latent - mean) / std).reshape(-1, 3).float()

    def case(g):
        dec = Decoder(dc.state_dict_of(vae_type), DEV, mean, std)
        res = {}
        res["idx"], res["zq"], res["lat"] = dec.vq(g(x_norm, "x"))
        res["idx_raw"], res["zq_raw"], res["lat_raw"] = dec.vq(g(latent.reshape(-1, 3).float(), "latent"), normalised=False)
        zq, xyz = g(case_["z_q"], "z_q"), g(case_["cg_xyz"], "cg_xyz")
        for variant in (0, 1):
            _lib.set_option(_lib.OPT_DEC_EDGE_VARIANT, variant)
            try:
                res[f"ic{variant}"] = dec.ic_decode(zq, case_["cg_z"], xyz, case_["pairs"])
            finally:
                _lib.set_option(_lib.OPT_DEC_EDGE_VARIANT, 0)
        ptr, src = dec.build_csr(xyz, [L] * B)
        res["csr_ptr"], res["csr_src"] = ptr, src[:int(ptr[-1])]
        ptr2, src2 = dec.build_csr(xyz, [L] * B, max_edges=B * L * (L - 1))      # the tail past ptr[-1] stays unwritten
        res["csr_ptr_bound"], res["csr_src_bound"] = ptr2, src2[:int(ptr2[-1])]
        res["ic_csr"] = dec.ic_decode(zq, case_["cg_z"], xyz, csr=(ptr2, src2))
        ic = res["ic0"].view(B, L, 13, 3)
        res["xyz"] = dec.ic_to_xyz(g(ca_full, "ca_full"), ic, prot["info"])
        groups = dec.ic_to_xyz_groups([(g(ca_full, "ca_full"), ic, prot["info"]),
                                       (g(ca_full[:1], "ca_full_1"), ic[:1].contiguous(), prot["info"])])
        res["xyz_g0"], res["xyz_g1"] = groups
        return res, []
    hold(f"decoder {vae_type}", case)


def test_xyz_to_ic():
    """codlad_xyz_to_ic through dataset_builder.xyz_to_ic on 3 frames of 40 atoms and 23 quads, some with an index < 0
    (the slot does not exist: zeros are written).  Defined: the whole [3, 23, 3] output."""
    from codlad_amd.utils.dataset_builder import xyz_to_ic
    rng = np.random.default_rng(77)
    xyz = torch.from_numpy(rng.normal(0, 3.0, (3, 40, 3)).astype(np.float32))
    quads = np.stack([rng.permutation(40)[:4] for _ in range(23)]).astype(np.int32)
    quads[[2, 11, 22], [3, 0, 1]] = -1

    def case(g):
        return dict(ic=xyz_to_ic(g(xyz, "xyz"), g(torch.from_numpy(quads), "quads"))), []
    hold("xyz_to_ic", case)


@pytest.mark.parametrize("variant", [0, 1, 2])
def test_encoder_entries(variant):
    """Prior.forward (two frames of 5 beads) and Encoder.forward (the 12-residue case of tests/test_e3nn_encoder.py) under
    every TP_CONV_VARIANT, the packed weight images made inside the patch.  Defined: mu, sigma and the latent, whole."""
    from codlad_amd.encoder import Encoder, Prior
    L, frames, wseed = cases.E3NN_ENCODER_CASES["L12"]
    prot = synth.make_protein(L, 50 + L, n_frames=frames)
    batch, atoms = synth.make_batch(prot), synth.make_atoms(prot, seed=L)
    pb = synth.make_batch(synth.make_protein(5, 45, n_frames=2))
    psd, esd = synth.prior_state_dict(31), synth.encoder_state_dict(wseed)

    def case(g):
        _lib.set_option(_lib.OPT_TP_CONV_VARIANT, variant)
        try:
            mu, sigma = Prior(psd, DEV).forward(pb["CG_nxyz"][:, 0].long(), g(pb["CG_nxyz"][:, 1:].contiguous(), "cg_xyz"), pb["CG_nbr_list"])
            lat = Encoder(esd, DEV).forward(atoms["nxyz"][:, 0], g(atoms["nxyz"][:, 1:].contiguous(), "xyz"), batch["CG_nxyz"][:, 0].long(),
                                            g(batch["CG_nxyz"][:, 1:].contiguous(), "cg_xyz"), atoms["CG_mapping"], atoms["nbr_list"],
                                            batch["CG_nbr_list"])
            enc = Encoder(esd, DEV)
            enc.pack_weights = False
            lat_unpacked = enc.forward(atoms["nxyz"][:, 0], atoms["nxyz"][:, 1:], batch["CG_nxyz"][:, 0].long(), batch["CG_nxyz"][:, 1:],
                                       atoms["CG_mapping"], atoms["nbr_list"], batch["CG_nbr_list"])
        finally:
            _lib.set_option(_lib.OPT_TP_CONV_VARIANT, 0)
        return dict(mu=mu, sigma=sigma, latent=lat, latent_unpacked=lat_unpacked), []
    hold(f"encoder variant {variant}", case)


@pytest.mark.parametrize("name", ["no_inter", "only_pipi"])
def test_eval_metrics(name):
    """metrics.all_results (one codlad_eval_metrics launch; `out` is a torch.zeros and `scratch` a torch.empty of the
    package's) on the two smallest cases, with empty interaction lists.  Defined: the eight results."""
    from codlad_amd import metrics as gm
    d = cases.metric_inputs(name)

    def case(g):
        dd = {k: g(v, k) for k, v in d.items()}
        r = gm.all_results(dd["ic_recon"], dd["ic"], dd["mask"], dd["xyz_recon"], dd["xyz"], dd["edge_list"], dd["nbr_list"],
                           dd["bb_NO_list"], dd["interaction_list"], dd["pi_pi_list"])
        return {k: v.reshape(1) for k, v in r.items()}, []
    hold(f"eval_metrics {name}", case)


def test_bond_graph_counts():
    """Defined: the [3, 6] count table."""
    from codlad_amd import metrics as gm
    d = cases.validity_inputs("loose")

    def case(g):
        return dict(counts=gm.bond_graph_counts(g(d["xyz"], "xyz"), g(d["xyz_recon"], "xyz_recon"), d["num_atoms"], d["atomic_nums"])), []
    hold("bond_graph_counts", case)


def test_ensemble_entries():
    """superposed_rmsd_batch (with the transform, with a selection, onto one target), superpose, pairwise_rmsd and
    diversity_terms on the builders of tests/test_ensemble.py.  Defined: everything returned."""
    from codlad_amd import metrics as gm
    from tests import ensemble_ref as er
    from tests.test_ensemble import _div_inputs
    a, b = (torch.from_numpy(np.array(v)) for v in er.batch(7, 257, 47))
    sel = [5, 3, 256, 0, 128, 64, 63, 255, 17, 200]
    rng = np.random.default_rng(5365)
    x = torch.from_numpy((rng.standard_normal((1, 3, 65, 3)) * 5.0 + rng.standard_normal((5, 3, 65, 3)) * 0.8 + 300.0).astype(np.float32))
    gen, ref = (torch.from_numpy(v) for v in _div_inputs())

    def case(g):
        da, db = g(a, "a"), g(b, "b")
        res = {}
        res["msd"], res["R"], res["t"] = gm.superposed_rmsd_batch(da, db, squared=True, return_transform=True)
        res["rmsd_sel"] = gm.superposed_rmsd_batch(da, db, sel=sel)
        res["rmsd_one_target"] = gm.superposed_rmsd_batch(da, g(b[0], "b0"))
        res["moved"] = gm.superpose(da, db, sel=sel)
        res["pairwise"] = gm.pairwise_rmsd(g(x, "x"))
        res["pairwise_sel"] = gm.pairwise_rmsd(g(x, "x"), sel=list(range(0, 65, 7)))
        res["to_ref"], res["to_mean"] = gm.diversity_terms(g(gen, "gen"), g(ref, "ref"))
        return res, []
    hold("ensemble", case)


@pytest.mark.parametrize("n", [4, 257])
def test_geometry_check(n):
    """geometry_check_lists on the generic topologies of tests/test_geometry_check.py (4 atoms; 257: a second row block), and
    at n = 257 also geometry_check on the protein case.  Defined: counts [S, 5] and min_dist [S] (the kernel's counters
    are the package's torch.empty: the host zeroes them before the launch)."""
    from codlad_amd import metrics as gm
    from tests import test_geometry_check as tg
    radius, bonds, xyz, _refs = tg.case(n)
    prot = tg.protein_case() if n == 257 else None

    def case(g):
        out = gm.geometry_check_lists(g(torch.from_numpy(xyz), "xyz"), torch.from_numpy(radius), bonds)
        res = dict(counts=out["counts"], min_dist=out["min_dist"])
        if prot is not None:
            out = gm.geometry_check(g(torch.from_numpy(prot[1]), "xyz_protein"), prot[0])
            res.update(p_counts=out["counts"], p_min_dist=out["min_dist"])
        return res, []
    hold(f"geometry_check n={n}", case)


@pytest.mark.parametrize("key", [3, 65, "two_chains"])
def test_stereo_check(key):
    """stereo_check on three structures of tests/test_stereo_check.py's cases.  Defined: values [S, R, 9] (NaN where the
    residue has no such quantity - in the plain run too, hence the comparison of bits), flags [S, R], counts [S, 6]."""
    from codlad_amd import metrics as gm
    from tests import test_stereo_check as ts
    c = ts.case(key)

    def case(g):
        out = gm.stereo_check(g(torch.from_numpy(np.ascontiguousarray(c["x"][0])), "xyz"), c["top"])
        return dict(values=out["values"], flags=out["flags"], counts=out["counts"]), []
    hold(f"stereo_check {key}", case)
