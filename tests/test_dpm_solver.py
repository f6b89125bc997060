"""DPM-Solver++(2M) on the HIP path (GPU): the stand-alone update against float64, order 1 against the DDIM goldens, the
fused loop (codlad_dpm_loop, final_kernel's DPM step) against the step-by-step path to the bit and against a float64 CPU loop
of the oracle, the analytic Gaussian model of tests/dpm_solver_ref.py on the device, pinning, streams, the status word and
`test.py --sampler dpmpp --timestep_spacing logsnr` end to end."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from codlad_amd import _lib, synth
from codlad_amd.diffusion_and_flow import PinLatents, create_diffusion
from codlad_amd.diffusion_and_flow.schedule import named_betas
from codlad_amd.engine import Denoiser
from codlad_amd.models.latent_model import MPNN_models
from oracle import denoiser as oden
from tests import cases
from tests import conditioning as cond
from tests import ddim_cases as dc
from tests import dpm_solver_ref as ref
from tests import guidance_cases as gc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
MODES = ("f16x3", "f16x4", "f32")


def rel_err(a, b):
    a = torch.as_tensor(a).detach().cpu().double()
    b = torch.as_tensor(b).detach().cpu().double()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def model_of(kind, precision="f16x3"):
    three, sc = kind == "three", kind == "selfcond"
    model = MPNN_models["mpnn_diffusion"](input_size=3, unconditional=True, diffusion="fm" if three else "diffusion",
                                          self_condition=sc)
    model.load_state_dict(synth.denoiser_state_dict(cases.WEIGHT_SEED, flow=three, self_condition=sc), strict=True)
    model.precision = precision
    return model.to(DEV).eval()


def on_dev(batch, mask):
    return dict(y=None, mask=mask.to(DEV), batch={k: (v.to(DEV) if hasattr(v, "to") else v) for k, v in batch.items()})


def per_step(model):
    """The model as an arbitrary callable: the loops then step through it instead of fusing."""
    return lambda x, t, **k: model(x, t, **k)


# ---------------------------------------------------------------------------------------- 6 --
@pytest.mark.parametrize("n", [1, 85, 86, 257])
def test_dpm_step_against_float64(n):
    """codlad_dpm_step on random operands against float64 with the fp32 row widened: three products and two sums, each
    correctly rounded, with slack for fused forms: |err| <= 3 * 2^-23 * (|A x| + |B x0| + |C x0_prev|) per element.  85
    nodes fill one 256-thread block but for a thread, 86 start the second, 257 the fourth.  A first-order row runs without
    prev_xstart, a second-order row refuses to."""
    g = torch.Generator().manual_seed(40 + n)
    x, x0, prev = (torch.randn(n, 3, generator=g).to(DEV) for _ in range(3))
    rows = ref.tables_for("linear", "logsnr10").dpm_solver_coefficients(2)
    for i, history in ((5, True), (1, True), (rows.shape[0] - 1, False), (0, False)):
        row = rows[i]
        assert (row[4] != 0) == history
        out, used = Denoiser.dpm_step(x, x0, prev if history else None, row)
        A, B, C = (float(v) for v in row[2:5])
        xd, x0d, pd = x.cpu().double(), x0.cpu().double(), prev.cpu().double()
        want = A * xd + B * x0d + (C * pd if history else 0.0)
        bound = 3 * 2.0 ** -23 * ((A * xd).abs() + (B * x0d).abs() + ((C * pd).abs() if history else 0.0))
        err = (out.cpu().double() - want).abs()
        print(f"n={n} row {i}: max err / bound {float((err / bound.clamp_min(1e-300)).max()):.3f}")
        assert bool((err <= bound).all()), (n, i, float((err / bound).max()))
        assert torch.equal(used, x0)
        if i == 0:
            assert torch.equal(out, x0)                                  # (0, 1, 0): the last step returns pred_xstart
    lib = _lib.lib()
    st = _lib.stream_ptr(torch.device(DEV))
    second = np.ascontiguousarray(rows[5])
    first = np.ascontiguousarray(rows[-1])
    out = torch.empty_like(x)
    assert lib.codlad_dpm_step(_lib.ptr(x), _lib.ptr(x0), None, None, second.ctypes.data_as(_lib.P), n, _lib.ptr(out), None, st) == -1
    assert b"prev_xstart" in lib.codlad_last_error()
    assert lib.codlad_dpm_step(_lib.ptr(x), _lib.ptr(x0), None, None, first.ctypes.data_as(_lib.P), n, _lib.ptr(out), None, st) == 0
    # x_out may alias x and x_start_out pred_xstart; the clamp bit acts on pred_xstart before the update
    clip = second.copy()
    clip[7] = 4
    want, want_used = Denoiser.dpm_step(x, x0, prev, clip)
    xa, x0a = x.clone(), x0.clone()
    assert lib.codlad_dpm_step(_lib.ptr(xa), _lib.ptr(x0a), _lib.ptr(prev), None, clip.ctypes.data_as(_lib.P), n, _lib.ptr(xa),
                               _lib.ptr(x0a), st) == 0
    assert torch.equal(xa, want) and torch.equal(x0a, want_used) and torch.equal(want_used, x0.clamp(-1, 1))


# ---------------------------------------------------------------------------------------- 7 --
ORDER1_CASES = ("fwd_L46", "fwd_xstart_L87", "fwd_fixed_small_L46", "fwd_ddim10_L46", "fwd_pin_L46", "fwd_tanh_L46",
                "fwd_cond_L46")


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ORDER1_CASES)
def test_order1_is_ddim(name, mode):
    """dpm_solver_sample_loop(order=1) is DDIM at eta 0: on the eta-0 forward cases of tests/ddim_cases.py, with their
    hooks, it meets the g18_ddim goldens at that file's tolerances - the sample (the fused loop where the case fuses), every
    step's sample and pred_xstart (step by step through an arbitrary callable)."""
    reverse, L, B, seed, respacing, kw, eta, clip, kind, _hooks = dc.DDIM_CASES[name]
    assert not reverse and eta == 0.0
    gold = np.load(cases.npz_path(f"g18_ddim_{name}"))
    tol = dc.DDIM_TOL.get(name, 2e-5)
    model = model_of(kind, mode)
    d = create_diffusion(respacing, noise_schedule="linear", **kw)
    _prot, batch, _x, _t, mask = cases.denoiser_inputs(L, B, seed)
    kwargs = on_dev(batch, mask)
    z = cases.loop_noise(dc.T, B, L, seed)[0].to(DEV)
    denoised_fn, cond_fn = dc.hooks_for(name, DEV)
    out = d.dpm_solver_sample_loop(model.forward, z.shape, z, clip_denoised=clip, denoised_fn=denoised_fn, cond_fn=cond_fn,
                                   model_kwargs=kwargs, order=1)
    err = rel_err(out, gold["sample"])
    print(f"{name} {mode}: sample rel err {err:.3e}")
    assert err < tol, f"{name} {mode}: sample rel err {err:.3e}"
    denoised_fn, cond_fn = dc.hooks_for(name, DEV)
    steps = list(d.dpm_solver_sample_loop_progressive(per_step(model), z.shape, z, clip_denoised=clip, denoised_fn=denoised_fn,
                                                      cond_fn=cond_fn, model_kwargs=kwargs, order=1))
    assert len(steps) == dc.T
    errs = [rel_err(o["sample"], gold["traj"][k]) for k, o in enumerate(steps)]
    assert max(errs) < tol, f"{name} {mode}: per-step trajectory rel err {['%.2e' % e for e in errs]}"
    for k, (o, i) in enumerate(zip(steps, range(dc.T - 1, -1, -1))):
        e = rel_err(o["pred_xstart"], gold["pred_xstart"][k])
        assert e < tol * max(1.0, float(d.sqrt_recipm1_alphas_cumprod[i])), f"{name} {mode}: pred_xstart of step {k}: {e:.3e}"
    if cond_fn is not None:
        assert cond_fn.timesteps[:dc.T] == [d.timestep_map[i] for i in range(dc.T - 1, -1, -1)]


# ---------------------------------------------------------------------------------------- 8 --
#   variant -> (model kind, create_diffusion kwargs, pinned)
VARIANTS = {"plain": ("eps", dict(), False), "pinned": ("eps", dict(), True),
            "selfcond": ("selfcond", dict(self_condition=True), False),
            "selfcond_pinned": ("selfcond", dict(self_condition=True), True),
            "xstart": ("eps", dict(predict_xstart=True), False),
            "fixed_var": ("three", dict(learn_sigma=False, sigma_small=True), False)}


@pytest.mark.parametrize("mode", ["f16x3", "f32"])
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_fused_equals_stepwise(variant, mode):
    """Order 2, T = 4 on "logsnr4": the fused loop equals the model forward, codlad_ddpm_pred_xstart, an optional
    PinLatents and codlad_dpm_step in a row, bit for bit, with clip_denoised on and off, at 5 and 33 residues x 2."""
    kind, kw, pinned = VARIANTS[variant]
    model = model_of(kind, mode)
    d = create_diffusion("logsnr4", **kw)
    assert d.num_timesteps == 4 and (d.dpm_solver_coefs(False)[1:3, 4] != 0).all()
    for L in (5, 33):
        B, seed = 2, 300 + L
        _prot, batch, x, _t, mask = cases.denoiser_inputs(L, B, seed)
        kwargs, z = on_dev(batch, mask), x.to(DEV)
        pin = wrapped = None
        if pinned:
            x0, pm = gc.pin_inputs(L, B, seed)
            pin = PinLatents(x0.to(DEV), pm.to(DEV))
            wrapped = lambda v: pin(v)                                      # noqa: E731  (not a PinLatents: per step)
        for clip in (False, True):
            fused = d.dpm_solver_sample_loop(model.forward, z.shape, z, clip_denoised=clip, denoised_fn=pin, model_kwargs=kwargs)
            split = d.dpm_solver_sample_loop(model.forward, z.shape, z, clip_denoised=clip, denoised_fn=wrapped,
                                             model_kwargs=kwargs) if pinned else \
                d.dpm_solver_sample_loop(per_step(model), z.shape, z, clip_denoised=clip, model_kwargs=kwargs)
            assert bool(torch.isfinite(fused).all())
            assert torch.equal(fused, split), (variant, mode, L, clip, rel_err(fused, split))
            first = d.dpm_solver_sample_loop(model.forward, z.shape, z, clip_denoised=clip, denoised_fn=pin,
                                             model_kwargs=kwargs, order=1)
            assert not torch.equal(fused, first)                            # the history term is there


@pytest.mark.parametrize("mode", ["f16x3", "f32"])
@pytest.mark.parametrize("self_condition", [False, True])
def test_fused_equals_stepwise_on_a_ragged_job(self_condition, mode):
    """One engine job of 5 + 8 + 13 residues: Denoiser.sample(kind="dpmpp") equals forward, ddpm_pred_xstart, the pin and
    dpm_step in a row, bit for bit, pinned or not."""
    sd = synth.denoiser_state_dict(cases.WEIGHT_SEED, self_condition=self_condition)
    den = Denoiser(sd, DEV, precision=mode)
    prots = [synth.make_protein(L, 20 + L, n_frames=1) for L in (5, 8, 13)]
    st = den.prepare_structures([torch.from_numpy(p["xyz_full"])[0, 1:-1] for p in prots],
                                [torch.from_numpy(p["z_full"])[1:-1] for p in prots])
    job = den.make_job(st, [0, 1, 2])
    n = job.n_nodes
    assert n == 26
    tables = create_diffusion("logsnr4", self_condition=self_condition)
    coef = tables.dpm_solver_coefs(False)
    g = torch.Generator(device=DEV).manual_seed(29)
    x_T = torch.randn(n, 3, device=DEV, generator=g)
    pin = (torch.randn(n, 3, device=DEV, generator=g), torch.rand(n, device=DEV, generator=g) < 0.3)
    for p in (None, pin):
        fused = den.sample(job, x_T, None, tables, coef=coef, pin=p, kind="dpmpp")
        x, prev = x_T, None
        for i in range(3, -1, -1):
            out = den.forward(job, x, tables.timestep_map[i], x_self_cond=prev if self_condition else None)
            x0 = Denoiser.ddpm_pred_xstart(x, out, coef[i])
            if p is not None:
                x0 = torch.where(p[1][:, None], p[0], x0)
            x, prev = Denoiser.dpm_step(x, x0, prev if coef[i, 4] != 0 else None, coef[i])
        assert torch.equal(fused, x), (self_condition, mode, p is not None)
    with pytest.raises(ValueError, match="noise must be None"):
        den.sample(job, x_T, torch.zeros(4, n, 3, device=DEV), tables, coef=coef, kind="dpmpp")


# ---------------------------------------------------------------------------------------- 9 --
@functools.lru_cache(maxsize=None)
def oracle_loops(name):
    """(float64 loop, fp32 loop) of oracle/denoiser.py on a case's geometry with "logsnr10", order 2: final x [B, L, 3].
    float64: weights, inputs, tables and update in float64; fp32: the reference's fp32 forward, the fp32 table rows and an
    fp32 update."""
    _rev, L, B, seed, _resp, kw, _eta, clip, kind, _hooks = dc.DDIM_CASES[name]
    assert kind == "eps" and not clip
    sd = synth.denoiser_state_dict(cases.WEIGHT_SEED)
    _prot, batch, _x, _t, _mask = cases.denoiser_inputs(L, B, seed)
    cg_z, cg_xyz, mask = oden.batch_to_dense(batch)
    z = cases.loop_noise(dc.T, B, L, seed)[0]
    d = create_diffusion("logsnr10", **kw)
    T = d.num_timesteps
    outs = []
    for dtype in (torch.float64, torch.float32):
        sdd = cond.to_dtype(sd, dtype)
        xyz = cg_xyz.to(dtype)
        feats = oden.ca_features(sdd, xyz, mask.int())
        if dtype == torch.float64:
            abc = torch.from_numpy(ref.paper_abc(d, 2))
            c0, c1 = torch.from_numpy(d.sqrt_recip_alphas_cumprod), torch.from_numpy(d.sqrt_recipm1_alphas_cumprod)
        else:
            rows = torch.from_numpy(d.dpm_solver_coefs(False))
            abc, c0, c1 = rows[:, 2:5], rows[:, 0], rows[:, 1]
        x, prev = z.to(dtype), None
        for i in range(T - 1, -1, -1):
            t = torch.full((B,), int(d.timestep_map[i]), dtype=torch.int64)
            out = oden.forward(sdd, x, t, xyz, cg_z, mask, features=feats)[..., :3]
            x0 = out if kw.get("predict_xstart") else c0[i] * x - c1[i] * out
            new = abc[i, 0] * x + abc[i, 1] * x0
            if abc[i, 2] != 0:
                new = new + abc[i, 2] * prev
            x, prev = new, x0
            assert x.dtype == dtype
        outs.append(x)
    return tuple(outs)


@pytest.mark.parametrize("name", ["fwd_L46", "fwd_xstart_L87"])
def test_order2_against_the_oracle(name):
    """The fused order-2 loop on "logsnr10" against a float64 CPU loop of the oracle, on the two DDIM geometries without a
    feature discontinuity: within 4 x max(e_ref, 5e-6) of the tensor's maximum, e_ref the fp32 CPU oracle loop's own
    distance from the float64 loop (a case whose e_ref alone exceeded 2e-5 would be dropped, not given a wider bound: none
    does).  Measured figures: DESIGN.md section 7."""
    _rev, L, B, seed, _resp, kw, _eta, clip, kind, _hooks = dc.DDIM_CASES[name]
    x64, x32 = oracle_loops(name)
    e_ref = rel_err(x32, x64)
    assert e_ref <= 2e-5, f"{name}: the reference side alone is off by {e_ref:.3e}"
    model = model_of(kind)
    d = create_diffusion("logsnr10", **kw)
    _prot, batch, _x, _t, mask = cases.denoiser_inputs(L, B, seed)
    z = cases.loop_noise(dc.T, B, L, seed)[0].to(DEV)
    out = d.dpm_solver_sample_loop(model.forward, z.shape, z, clip_denoised=clip, model_kwargs=on_dev(batch, mask))
    err = rel_err(out, x64)
    print(f"{name}: device vs float64 {err:.3e}, fp32 oracle vs float64 (e_ref) {e_ref:.3e}, bound {4 * max(e_ref, 5e-6):.3e}")
    assert err <= 4 * max(e_ref, 5e-6), (name, err, e_ref)


# --------------------------------------------------------------------------------------- 10 --
class GaussianEps:
    """The exact noise prediction of data N(0, s^2 I) as a plain CUDA callable: eps | zero variance channels."""

    def __init__(self, s, schedule="linear"):
        acp = np.cumprod(1.0 - named_betas(schedule, ref.BASE_STEPS))
        self.e = torch.from_numpy(ref.gaussian_eps_factor(acp, s).astype(np.float32)).to(DEV)

    def __call__(self, x, t, **_kwargs):
        return torch.cat([self.e[t].view(-1, 1, 1) * x, torch.zeros_like(x)], dim=-1)


def test_analytic_model_on_the_device():
    """The Gaussian denoiser through the stepwise path (the callable, codlad_ddpm_pred_xstart, codlad_dpm_step) at L = 20,
    B = 2 on "logsnr20": the final x is within 4 x max(e32, 1e-6) of the float64 restatement, e32 the fp32 numpy
    restatement's own distance from it (measured: DESIGN.md section 7); and the second order is at least 4 times closer
    to the exact solution than the first, on the device as in float64."""
    s, L, B = 1.0, 20, 2
    d = create_diffusion("logsnr20")
    x_T = synth.gaussian((B, L, 3), 77)
    flat = x_T.numpy().astype(np.float64).reshape(-1)
    exact = ref.exact_solution(flat, d.alphas_cumprod[-1], s)
    to_exact = {}
    for order in (1, 2):
        x64 = ref.solve(d, order, s, flat)
        x32 = ref.solve(d, order, s, flat, dtype=np.float32)
        e32 = float(np.abs(x32 - x64).max() / np.abs(x64).max())
        out = d.dpm_solver_sample_loop(GaussianEps(s), x_T.shape, x_T.to(DEV), clip_denoised=False, order=order)
        got = out.cpu().numpy().astype(np.float64).reshape(-1)
        err = float(np.abs(got - x64).max() / np.abs(x64).max())
        to_exact[order] = float(np.abs(got - exact).max() / np.abs(exact).max())
        print(f"order {order}: device vs float64 {err:.3e}, fp32 numpy vs float64 (e32) {e32:.3e}, "
              f"bound {4 * max(e32, 1e-6):.3e}, device vs exact {to_exact[order]:.3e}")
        assert err <= 4 * max(e32, 1e-6), (order, err, e32)
    assert to_exact[1] / to_exact[2] >= 4.0, to_exact


# --------------------------------------------------------------------------------------- 11 --
@pytest.mark.parametrize("clip", [False, True])
def test_pinned_nodes_end_exactly_on_their_latents(clip):
    """Row 0 is (0, 1, 0): a pinned node ends on its latent exactly - on the clamped latent under clip_denoised; the rest
    differs from the unpinned run; two runs give equal bits."""
    L, B, seed = 46, 2, 107
    model = model_of("eps")
    d = create_diffusion("logsnr10")
    assert tuple(d.dpm_solver_coefs(clip)[0, 2:5]) == (0.0, 1.0, 0.0)
    _prot, batch, x, _t, mask = cases.denoiser_inputs(L, B, seed)
    kwargs, z = on_dev(batch, mask), x.to(DEV)
    x0, pm = gc.pin_inputs(L, B, seed)
    pin = PinLatents(x0.to(DEV), pm.to(DEV))
    assert bool((pin.x0[pin.mask].abs() > 1).any())                        # the clamp has something to do
    out = d.dpm_solver_sample_loop(model.forward, z.shape, z, clip_denoised=clip, denoised_fn=pin, model_kwargs=kwargs)
    again = d.dpm_solver_sample_loop(model.forward, z.shape, z, clip_denoised=clip, denoised_fn=pin, model_kwargs=kwargs)
    free = d.dpm_solver_sample_loop(model.forward, z.shape, z, clip_denoised=clip, model_kwargs=kwargs)
    m = pin.mask
    want = pin.x0.clamp(-1, 1) if clip else pin.x0
    assert torch.equal(out[m], want[m])
    assert torch.equal(out, again)
    assert not torch.equal(out[~m], free[~m]) and bool(torch.isfinite(out).all())


@pytest.mark.parametrize("self_condition", [False, True])
def test_streams_equal_one_stream(self_condition):
    """Denoiser.sample(kind="dpmpp") on a small ragged job with repeated members gives the same bits on 1 and 2 streams,
    pinned or not: each half-job carries its own x_start history."""
    sd = synth.denoiser_state_dict(cases.WEIGHT_SEED, self_condition=self_condition)
    den = Denoiser(sd, DEV)
    pa, pb = synth.make_protein(46, 12, n_frames=1), synth.make_protein(33, 13, n_frames=1)
    st = den.prepare_structures([torch.from_numpy(p["xyz_full"])[0, 1:-1] for p in (pa, pb)],
                                [torch.from_numpy(p["z_full"])[1:-1] for p in (pa, pb)])
    job = den.make_job(st, [0, 1, 1, 0, 1])
    n = job.n_nodes
    tables = create_diffusion("logsnr6", self_condition=self_condition)
    g = torch.Generator(device=DEV).manual_seed(31)
    x_T = torch.randn(n, 3, device=DEV, generator=g)
    pin = (torch.randn(n, 3, device=DEV, generator=g), torch.rand(n, device=DEV, generator=g) < 0.25)
    for p in (None, pin):
        one, two = (den.sample(job, x_T, None, tables, streams=s, pin=p, kind="dpmpp") for s in (1, 2))
        assert torch.equal(one, two), (self_condition, p is not None)
        assert bool(torch.isfinite(one).all())


def test_status_word_raises_from_the_dpm_loop():
    """Edge features far outside the fp16 range (the weights of test_precision_envelope): the loop reports it through the
    status word as the other loops do, and the job is usable again afterwards."""
    L, B, seed = cases.ENVELOPE_GEOMETRY
    prot, _batch, _x, _t, _mask = cases.denoiser_inputs(L, B, seed)
    sd = synth.denoiser_state_dict(cases.WEIGHT_SEED)
    sd["features.norm_edges.weight"] = sd["features.norm_edges.weight"] * 1e6
    den = Denoiser(sd, DEV, precision="f16x3")
    frames = torch.from_numpy(prot["xyz_full"])[:, 1:-1]
    st = den.prepare_structures([f for f in frames], [torch.from_numpy(prot["z_full"])[1:-1]] * B)
    job = den.make_job(st, list(range(B)))
    z = cases.loop_noise(3, B, L, seed)[0].reshape(-1, 3).to(DEV)
    with pytest.raises(RuntimeError, match="not finite"):
        den.sample(job, z, None, create_diffusion("logsnr3"), kind="dpmpp")
    assert int(job.status.item()) == 0


# --------------------------------------------------------------------------------------- 12 --
def _cli(extra, cwd):
    cmd = [sys.executable, os.path.join(ROOT, "test.py"), "--synthetic", "--synthetic_weights", "--synthetic_frames", "2",
           "--save_codes"] + extra
    os.makedirs(cwd, exist_ok=True)
    res = subprocess.run(cmd, env=dict(os.environ, PYTHONPATH=ROOT), cwd=str(cwd), capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-1500:] + res.stderr[-3000:]
    out_dir = os.path.join(str(cwd), "logs", "generated_samples_0_best", "experiment_cifar_default_PED")
    return res.stdout, lambda L, what: np.load(os.path.join(out_dir, f"synthetic_L{L}_{what}.npy"))


def test_cli_sampler_dpmpp(tmp_path):
    """test.py --sampler dpmpp --timestep_spacing logsnr --num_sampling_steps 20 --fix_residues 3-10 on the synthetic PED set:
    prints the steps kept, writes finite coordinates, and residues 3-10 of every structure carry the VQ codes of the
    encoder's latents (the --experiment recon run's)."""
    out, got = _cli(["--sampler", "dpmpp", "--timestep_spacing", "logsnr", "--num_sampling_steps", "20", "--fix_residues", "3-10"],
                    tmp_path / "dpmpp")
    assert "20 of 20 requested steps kept" in out and "done: 8 structures on 1 GPU(s)" in out
    _out, enc = _cli(["--experiment", "recon"], tmp_path / "recon")
    for L in (46, 87, 92, 129):
        xyz, codes = got(L, "xyz_recon"), got(L, "codes")
        assert np.isfinite(xyz).all() and codes.shape == (2, L)
        assert np.array_equal(codes[:, 2:10], enc(L, "codes")[:, 2:10])
        assert not np.array_equal(codes, enc(L, "codes"))                   # the other residues were sampled
