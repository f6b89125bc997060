"""DDIM sampling and inversion (the IDDPM release's ddim_sample / ddim_reverse_sample over the reference's respaced tables)
on the HIP path - fused into the loop (codlad_ddim_loop, final_kernel's DDIM steps), or step by step through the model and
codlad_ddpm_pred_xstart / codlad_ddim_step - against the reference's own p_mean_variance / condition_score with the
DDIM update restated (g18 goldens, tests/ddim_cases.py), and `test.py --sampler ddim` end to end.  The CPU part checks the
coefficient table against the reference's fp32 values, argument validation and the new C entry points."""
import ctypes
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

from codlad_amd import _lib, synth
from codlad_amd.diffusion_and_flow import ModelMeanType, PinLatents, SpacedDiffusion, create_diffusion
from codlad_amd.diffusion_and_flow.schedule import Tables, named_betas, space_timesteps
from codlad_amd.models.latent_model import MPNN_models
from tests import cases
from tests import ddim_cases as dc
from tests import guidance_cases as gc
from tests.cli_script import load_cli

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
gpu = pytest.mark.gpu


def rel_err(a, b):
    a = torch.as_tensor(a).detach().cpu().double()
    b = torch.as_tensor(b).detach().cpu().double()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def cli_module():
    return load_cli("codlad_cli")


def case_diffusion(name):
    _rev, _L, _B, _seed, respacing, kw, _eta, _clip, _model, _hooks = dc.DDIM_CASES[name]
    return create_diffusion(respacing, noise_schedule="linear", **kw)


# ---------------------------------------------------------------------------------------- CPU --
@pytest.mark.parametrize("name", list(dc.DDIM_CASES))
def test_ddim_coefficients_are_the_reference_values(name):
    """Every schedule factor of the DDIM table is the reference's fp32 value to the bit (forward at eta 0 / 0.5 / 1,
    reverse, the "ddim10" respacing); column 7 is the step table's mode word."""
    reverse, _L, _B, _seed, respacing, kw, eta, clip, _model, _hooks = dc.DDIM_CASES[name]
    gold = np.load(cases.npz_path(f"g18_ddim_{name}"))
    d = case_diffusion(name)
    assert d.timestep_map == gold["timestep_map"].tolist()
    c = d.ddim_coefs(clip, eta, reverse)
    assert c.dtype == np.float32 and c.shape == (dc.T, 8)
    assert np.array_equal(c[:, :6], gold["coef"])
    assert np.array_equal(c[:, 7], d.coefficients(clip)[:, 7]) and not c[:, 6].any()
    if reverse:
        assert not c[:, 4].any()


def test_ddim_table_limits():
    """The forward table's last row gives pred_xstart itself (sqrt(acp_prev) = 1, no eps, no noise) at any eta; at eta = 1
    sigma^2 is the posterior variance; the reverse table's last row gives eps itself (acp_next = 0)."""
    tb = Tables(named_betas("linear", 1000), space_timesteps(1000, "ddim10"))
    for eta in (0.0, 0.5, 1.0):
        c = tb.ddim_coefficients(eta)
        assert c[0, 2] == 1.0 and c[0, 3] == 0.0 and c[0, 4] == 0.0
        assert (c[1:, 4] > 0).all() == (eta > 0)
    one = tb.ddim_coefficients(1.0)
    # (fp32 as in the reference: 1 - acp_prev cancels at the first steps, 1.7e-4 relative at i = 1 of "ddim10")
    assert np.allclose(one[1:, 4].astype(np.float64) ** 2, tb.posterior_variance[1:], rtol=1e-3, atol=0)
    r = tb.ddim_coefficients(reverse=True)
    assert r[-1, 2] == 0.0 and r[-1, 3] == 1.0
    with pytest.raises(ValueError, match="eta must be >= 0"):
        tb.ddim_coefficients(-0.1)
    with pytest.raises(ValueError, match="eta must be 0"):
        tb.ddim_coefficients(0.5, reverse=True)
    with pytest.raises(ValueError, match="unknown variance type"):
        tb.ddim_coefficients(var_type="fixed_medium")


def test_ddim_argument_validation():
    model = MPNN_models["mpnn_diffusion"](input_size=3, unconditional=True, diffusion="diffusion", self_condition=False)
    prot, batch, x, t, mask = cases.denoiser_inputs(20, 2, 11)
    d = create_diffusion("10")
    kw = dict(y=None, mask=mask, batch=batch)
    with pytest.raises(ValueError, match="eta must be >= 0"):
        d.ddim_sample_loop(model.forward, x.shape, x, model_kwargs=kw, eta=-0.5)
    with pytest.raises(ValueError, match="eta must be >= 0"):
        next(d.ddim_sample_loop_progressive(model.forward, x.shape, x, model_kwargs=kw, eta=-1.0))
    with pytest.raises(ValueError, match="eta must be 0"):
        d.ddim_reverse_sample_loop(model.forward, x, model_kwargs=kw, eta=0.5)
    with pytest.raises(ValueError, match="eta must be 0"):
        d.ddim_reverse_sample(model.forward, x, t, model_kwargs=kw, eta=1.0)
    with pytest.raises(TypeError, match="denoised_fn must be callable"):
        d.ddim_sample_loop(model.forward, x.shape, x, denoised_fn=3, model_kwargs=kw)
    with pytest.raises(TypeError, match="cond_fn must be callable"):
        d.ddim_reverse_sample_loop(model.forward, x, cond_fn="grad", model_kwargs=kw)
    with pytest.raises(TypeError, match="cond_fn must be callable"):
        next(d.ddim_sample_loop_progressive(model.forward, x.shape, x, cond_fn=1.0, model_kwargs=kw))
    with pytest.raises(TypeError, match="eta must be a number"):
        d.ddim_sample_loop(model.forward, x.shape, x, model_kwargs=kw, eta="0")
    with pytest.raises(NotImplementedError, match="PREVIOUS_X"):
        SpacedDiffusion(space_timesteps(1000, "10"), named_betas("linear", 1000), model_mean_type=ModelMeanType.PREVIOUS_X)
    x0, pm = gc.pin_inputs(20, 2, 5)
    for hooks in (dict(), dict(denoised_fn=PinLatents(x0, pm)), dict(denoised_fn=gc.tanh_denoised_fn),
                  dict(cond_fn=gc.PullToTarget(x0))):
        with pytest.raises(RuntimeError, match="MI355X"):
            d.ddim_sample_loop(model.forward, x.shape, x, clip_denoised=False, model_kwargs=kw, **hooks)
        with pytest.raises(RuntimeError, match="MI355X"):
            d.ddim_reverse_sample_loop(model.forward, x, clip_denoised=False, model_kwargs=kw, **hooks)


def test_cli_sampler_combinations():
    cli = cli_module()
    base = dict(sampler="ddpm", eta=0.0, experiment="latent", model="diffusion")
    cli.check_sampler(types.SimpleNamespace(**base))
    cli.check_sampler(types.SimpleNamespace(**dict(base, sampler="ddim")))
    cli.check_sampler(types.SimpleNamespace(**dict(base, sampler="ddim", eta=1.0)))
    for change, msg in ((dict(eta=0.5), "--eta applies to --sampler ddim only"),
                        (dict(sampler="ddim", eta=-1.0), "--eta must be >= 0"),
                        (dict(sampler="ddim", model="fm"), "--model diffusion"),
                        (dict(sampler="ddim", model="otcfm"), "--model diffusion"),
                        (dict(sampler="ddim", experiment="recon"), "--experiment latent"),
                        (dict(sampler="ddim", experiment="genzprot"), "--experiment latent"),
                        (dict(sampler="plms"), "ddpm or ddim")):
        with pytest.raises(SystemExit, match=msg):
            cli.check_sampler(types.SimpleNamespace(**dict(base, **change)))
    # the DDPM defaults pass with any model / experiment, as before
    for other in (dict(model="fm"), dict(experiment="recon"), dict(experiment="genzprot")):
        cli.check_sampler(types.SimpleNamespace(**dict(base, **other)))


def test_ddim_entry_points_validate_their_arguments():
    lib = _lib.lib()
    coef = (np.zeros(8, dtype=np.float32)).ctypes.data_as(_lib.P)
    one = torch.zeros(12)
    p = _lib.ptr(one)
    w = _lib.DenoiserWeights()
    w.out_dim, w.self_condition = 6, 0
    wp = ctypes.byref(w)

    def loop(w=wp, node_info=p, T=10, mode=0, reverse=0, noise=p, x_start=None, pin_x0=None, pin_mask=None, x=p):
        job = _lib.JobDesc(node_info, 4, p, p, None, 1, None)
        return lib.codlad_ddim_loop(w, ctypes.byref(job), x, x_start, noise, p, p, T, mode, reverse, pin_x0, pin_mask, None)

    assert loop(w=None) == -1 and b"codlad_ddim_loop: null pointer" in lib.codlad_last_error()
    assert loop(x=None) == -1 and b"null pointer" in lib.codlad_last_error()
    assert loop(noise=None) == -1 and b"noise" in lib.codlad_last_error()
    assert loop(pin_x0=p) == -1 and b"pin_x0 and pin_mask" in lib.codlad_last_error()
    for T in (0, -3):
        assert loop(T=T) == -1 and b"T must be positive" in lib.codlad_last_error()
    assert loop(mode=2) == -1 and b"mode and model disagree" in lib.codlad_last_error()
    assert loop(mode=8) == -1 and b"unknown mode bits" in lib.codlad_last_error()
    w.out_dim = 3
    assert loop(mode=0) == -1 and b"mode and model disagree" in lib.codlad_last_error()
    assert loop(mode=2 | 4, reverse=1, noise=None) == -1 and b"incomplete workspace" in lib.codlad_last_error()
    w.out_dim, w.self_condition = 6, 1
    assert loop() == -1 and b"x_start buffer" in lib.codlad_last_error()

    assert lib.codlad_ddim_step(None, p, p, None, coef, 0, 4, p, None, None) == -1
    assert b"codlad_ddim_step: null pointer" in lib.codlad_last_error()
    assert lib.codlad_ddim_step(p, p, None, None, coef, 0, 4, p, None, None) == -1
    assert b"noise" in lib.codlad_last_error()
    assert lib.codlad_ddim_step(p, p, p, None, coef, 1, 0, p, None, None) == -1
    assert b"n_nodes must be positive" in lib.codlad_last_error()


# ---------------------------------------------------------------------------------------- GPU --
def ddim_model(kind):
    three, sc = kind == "three", kind == "selfcond"
    model = MPNN_models["mpnn_diffusion"](input_size=3, unconditional=True, diffusion="fm" if three else "diffusion",
                                          self_condition=sc)
    model.load_state_dict(synth.denoiser_state_dict(cases.WEIGHT_SEED, flow=three, self_condition=sc), strict=True)
    return model.to(DEV).eval()


def case_setup(name):
    reverse, L, B, seed, _resp, _kw, eta, clip, kind, _hooks = dc.DDIM_CASES[name]
    model = ddim_model(kind)
    prot, batch, _x, _t, mask = cases.denoiser_inputs(L, B, seed)
    batch = {k: (v.to(DEV) if hasattr(v, "to") else v) for k, v in batch.items()}
    z, eps = cases.loop_noise(dc.T, B, L, seed)
    return model, case_diffusion(name), dict(y=None, mask=mask.to(DEV), batch=batch), z.to(DEV), eps.to(DEV), clip, eta


def run_case(name, model_fn, hooks):
    """(final sample, per-step outputs or None) of a case through the drop-in calls with model_fn."""
    reverse = dc.DDIM_CASES[name][0]
    model, d, kwargs, z, eps, clip, eta = case_setup(name)
    denoised_fn, cond_fn = hooks
    if reverse:
        return (d.ddim_reverse_sample_loop(model_fn(model), z, clip_denoised=clip, denoised_fn=denoised_fn,
                                           cond_fn=cond_fn, model_kwargs=kwargs, device=DEV),
                list(d.ddim_reverse_sample_loop_progressive(model_fn(model), z, clip_denoised=clip, denoised_fn=denoised_fn,
                                                            cond_fn=cond_fn, model_kwargs=kwargs, device=DEV)))
    return (d.ddim_sample_loop(model_fn(model), z.shape, z, clip_denoised=clip, denoised_fn=denoised_fn, cond_fn=cond_fn,
                               model_kwargs=kwargs, device=DEV, eta=eta, step_noise=eps),
            list(d.ddim_sample_loop_progressive(model_fn(model), z.shape, z, clip_denoised=clip, denoised_fn=denoised_fn,
                                                cond_fn=cond_fn, model_kwargs=kwargs, device=DEV, eta=eta, step_noise=eps)))


@gpu
@pytest.mark.parametrize("name", list(dc.DDIM_CASES))
def test_ddim_like_the_reference(name):
    """ddim_sample_loop / ddim_reverse_sample_loop against the reference: with the codlad_amd model (no hook or a PinLatents
    = the fused loop, any other hook = per step) and, per step, with an arbitrary model callable; every step's sample and
    pred_xstart within 2e-5 of the reference's, the two paths equal to the bit, cond_fn handed the original-process
    timesteps."""
    gold = np.load(cases.npz_path(f"g18_ddim_{name}"))
    tol = dc.DDIM_TOL.get(name, 2e-5)
    hooks = dc.hooks_for(name, DEV)
    out, _ = run_case(name, lambda m: m.forward, hooks)
    err = rel_err(out, gold["sample"])
    assert err < tol, f"{name}: sample rel err {err:.3e}"
    hooks = dc.hooks_for(name, DEV)
    final, steps = run_case(name, lambda m: (lambda x, t, **k: m(x, t, **k)), hooks)
    errs = [rel_err(o["sample"], gold["traj"][k]) for k, o in enumerate(steps)]
    assert max(errs) < tol, f"{name}: per-step trajectory rel err {['%.2e' % e for e in errs]}"
    # pred_xstart = sqrt_recip_acp * x - sqrt_recipm1_acp * eps carries the model output's rounding times sqrt_recipm1_acp
    # (up to 157 at the first step of T = 10); a clamped pred_xstart (max 1) shows it: the bar scales with that factor
    d = case_diffusion(name)
    order = list(range(dc.T)) if dc.DDIM_CASES[name][0] else list(range(dc.T - 1, -1, -1))
    for k, (o, i) in enumerate(zip(steps, order)):
        e = rel_err(o["pred_xstart"], gold["pred_xstart"][k])
        assert e < tol * max(1.0, float(d.sqrt_recipm1_alphas_cumprod[i])), f"{name}: pred_xstart of step {k}: rel err {e:.3e}"
    assert torch.equal(steps[-1]["sample"], final) and torch.equal(final, out)
    _d, cond_fn = hooks
    if cond_fn is not None:
        want = [d.timestep_map[i] for i in order]
        assert cond_fn.timesteps[:dc.T] == gold["cond_timesteps"].tolist() == want


@gpu
@pytest.mark.parametrize("name", ["fwd_pin_L46", "rev_pin_L46", "fwd_cond_pin_eta05_L87"])
def test_fused_pin_equals_the_split_step(name):
    """The pin fused into final_kernel's DDIM steps and PinLatents between codlad_ddpm_pred_xstart and codlad_ddim_step
    round alike, forward and reverse, with and without self-conditioning (a self-conditioned model on the same case)."""
    reverse, L, B, seed, _resp, _kw, eta, clip, _kind, _hooks = dc.DDIM_CASES[name]
    for kind in ("eps", "selfcond"):
        model = ddim_model(kind)
        d = create_diffusion("10", self_condition=kind == "selfcond")
        prot, batch, _x, _t, mask = cases.denoiser_inputs(L, B, seed)
        kwargs = dict(y=None, mask=mask.to(DEV), batch={k: (v.to(DEV) if hasattr(v, "to") else v) for k, v in batch.items()})
        z, eps = (v.to(DEV) for v in cases.loop_noise(dc.T, B, L, seed))
        pin, _ = dc.hooks_for(name, DEV)
        wrapped = lambda x: pin(x)                                          # noqa: E731  (not a PinLatents: per step)
        if reverse:
            fused = d.ddim_reverse_sample_loop(model.forward, z, clip_denoised=clip, denoised_fn=pin, model_kwargs=kwargs)
            split = d.ddim_reverse_sample_loop(model.forward, z, clip_denoised=clip, denoised_fn=wrapped, model_kwargs=kwargs)
        else:
            fused = d.ddim_sample_loop(model.forward, z.shape, z, clip_denoised=clip, denoised_fn=pin, model_kwargs=kwargs,
                                       eta=eta, step_noise=eps)
            split = d.ddim_sample_loop(model.forward, z.shape, z, clip_denoised=clip, denoised_fn=wrapped,
                                       model_kwargs=kwargs, eta=eta, step_noise=eps)
        assert torch.equal(fused, split), (name, kind)


@gpu
@pytest.mark.parametrize("eta", [0.0, 0.5])
def test_pinned_nodes_end_exactly_on_their_latents(eta):
    """The forward table's last row is sqrt(acp_prev) = 1, sqrt(1 - acp_prev - sigma^2) = 0, sigma = 0: without
    clip_denoised a pinned node ends on its latent exactly; the rest differs from the unpinned run on the same noise."""
    model, d, kwargs, z, eps, clip, _eta = case_setup("fwd_pin_L46")
    c = d.ddim_coefs(False, eta)[0]
    assert c[2] == 1.0 and c[3] == 0.0 and c[4] == 0.0
    pin, _ = dc.hooks_for("fwd_pin_L46", DEV)
    out = d.ddim_sample_loop(model.forward, z.shape, z, clip_denoised=False, denoised_fn=pin, model_kwargs=kwargs, eta=eta,
                             step_noise=eps)
    free = d.ddim_sample_loop(model.forward, z.shape, z, clip_denoised=False, model_kwargs=kwargs, eta=eta, step_noise=eps)
    m = pin.mask
    assert torch.equal(out[m], pin.x0[m])
    assert not torch.equal(out[~m], free[~m])
    assert bool(torch.isfinite(out).all())


@gpu
def test_ddim_eta1_is_the_fixed_small_ddpm_sampler():
    """DDIM with eta = 1 is the ancestral sampler with the posterior variance (FIXED_SMALL) in exact arithmetic; on the
    3-output head with the same noise the two fused loops agree to the golden bar."""
    model = ddim_model("three")
    L, B, seed = 46, 2, 105
    prot, batch, _x, _t, mask = cases.denoiser_inputs(L, B, seed)
    kwargs = dict(y=None, mask=mask.to(DEV), batch={k: (v.to(DEV) if hasattr(v, "to") else v) for k, v in batch.items()})
    z, eps = (v.to(DEV) for v in cases.loop_noise(dc.T, B, L, seed))
    d = create_diffusion("10", learn_sigma=False, sigma_small=True)
    ddim = d.ddim_sample_loop(model.forward, z.shape, z, clip_denoised=False, model_kwargs=kwargs, eta=1.0, step_noise=eps)
    ddpm = d.p_sample_loop(model.forward, z.shape, z, clip_denoised=False, model_kwargs=kwargs, step_noise=eps)
    err = rel_err(ddim, ddpm)
    print(f"DDIM eta=1 vs DDPM FIXED_SMALL, rel err {err:.3e}")
    assert err < 2e-5, err


@gpu
@pytest.mark.parametrize("self_condition", [False, True])
def test_streams_equal_one_stream(self_condition):
    """Denoiser.sample(kind="ddim" / "ddim_reverse") on a ragged job with repeated members (structures of 46 and 87
    residues, 12 samples) gives the same result on 1, 2 and 3 streams, to the bit, pinned or not."""
    model = ddim_model("selfcond" if self_condition else "eps")
    eng = model.engine()
    pa, pb = synth.make_protein(46, 12, n_frames=1), synth.make_protein(87, 13, n_frames=1)
    st = eng.prepare_structures([torch.from_numpy(p["xyz_full"])[0, 1:-1] for p in (pa, pb)],
                                [torch.from_numpy(p["z_full"])[1:-1] for p in (pa, pb)])
    members = [0, 1, 1, 0, 1, 0, 0, 1, 1, 1, 0, 0]
    job = eng.make_job(st, members)
    n = job.n_nodes
    T = 10
    tables = create_diffusion(str(T), self_condition=self_condition)
    gen = torch.Generator(device=DEV).manual_seed(23)
    x_T = torch.randn(n, 3, device=DEV, generator=gen)
    noise = torch.randn(T, n, 3, device=DEV, generator=gen)
    pin = (torch.randn(n, 3, device=DEV, generator=gen), torch.rand(n, device=DEV, generator=gen) < 0.25)
    for kind, coef, nz in (("ddim", tables.ddim_coefs(False, 0.5), noise), ("ddim_reverse", None, None)):
        for p in (None, pin):
            outs = [eng.sample(job, x_T, nz, tables, coef=coef, streams=s, pin=p, kind=kind) for s in (1, 2, 3)]
            assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2]), (kind, p is not None)
            assert bool(torch.isfinite(outs[0]).all())


@gpu
def test_large_job_fused_equals_stepwise():
    """24 frames x 87 residues (2 088 nodes): the fused DDIM loop and the per-step path agree to the bit, forward at
    eta = 0.5 and reverse."""
    model = ddim_model("eps")
    L, B, seed = 87, 24, 131
    prot, batch, _x, _t, mask = cases.denoiser_inputs(L, B, seed)
    kwargs = dict(y=None, mask=mask.to(DEV), batch={k: (v.to(DEV) if hasattr(v, "to") else v) for k, v in batch.items()})
    z, eps = (v.to(DEV) for v in cases.loop_noise(dc.T, B, L, seed))
    assert B * L >= 2000
    d = create_diffusion("10")
    step = lambda x, t, **k: model(x, t, **k)                               # noqa: E731
    fused = d.ddim_sample_loop(model.forward, z.shape, z, clip_denoised=False, model_kwargs=kwargs, eta=0.5, step_noise=eps)
    split = d.ddim_sample_loop(step, z.shape, z, clip_denoised=False, model_kwargs=kwargs, eta=0.5, step_noise=eps)
    assert torch.equal(fused, split)
    inv = d.ddim_reverse_sample_loop(model.forward, fused, clip_denoised=False, model_kwargs=kwargs)
    inv_split = d.ddim_reverse_sample_loop(step, fused, clip_denoised=False, model_kwargs=kwargs)
    assert torch.equal(inv, inv_split) and bool(torch.isfinite(inv).all())


def _cli(extra, cwd, timeout=600):
    cmd = [sys.executable, os.path.join(ROOT, "test.py"), "--synthetic", "--synthetic_weights", "--synthetic_frames", "2",
           "--num_ensemble", "2", "--data_type", "PED", "--vae_type", "N6", "--exp", "clitest",
           "--num_sampling_steps", "10"] + extra
    os.makedirs(cwd, exist_ok=True)
    env = dict(os.environ, PYTHONPATH=ROOT)
    res = subprocess.run(cmd, env=env, cwd=str(cwd), capture_output=True, text=True, timeout=timeout)
    assert res.returncode == 0, res.stdout[-1500:] + res.stderr[-3000:]
    assert "done: 16 structures on 1 GPU(s)" in res.stdout
    out_dir = os.path.join(str(cwd), "logs", "generated_samples_0_best", "clitest_PED")
    return lambda L: np.load(os.path.join(out_dir, f"synthetic_L{L}_xyz_recon.npy"))


@gpu
def test_cli_sampler_ddim(tmp_path):
    """test.py --sampler ddim on the synthetic PED set: writes its outputs, two runs give identical files, they differ from
    the DDPM run; with --fix_residues 1-46 the 46-residue structure decodes to exactly the --experiment recon output."""
    a = _cli(["--sampler", "ddim"], tmp_path / "a")
    b = _cli(["--sampler", "ddim"], tmp_path / "b")
    ddpm = _cli([], tmp_path / "ddpm")
    for L in (46, 87, 92, 129):
        assert np.isfinite(a(L)).all() and np.array_equal(a(L), b(L))
        assert a(L).shape == ddpm(L).shape and not np.array_equal(a(L), ddpm(L))
    recon = _cli(["--experiment", "recon"], tmp_path / "recon")
    pinned = _cli(["--sampler", "ddim", "--eta", "0.5", "--fix_residues", "1-46"], tmp_path / "pinned")
    assert np.array_equal(pinned(46), recon(46))
    bad = subprocess.run([sys.executable, os.path.join(ROOT, "test.py"), "--synthetic", "--synthetic_weights",
                          "--sampler", "ddim", "--model", "fm"], env=dict(os.environ, PYTHONPATH=ROOT), cwd=str(tmp_path),
                         capture_output=True, text=True, timeout=600)
    assert bad.returncode != 0 and "--model diffusion" in bad.stdout + bad.stderr
