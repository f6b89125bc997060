"""Guided sampling: the reference's denoised_fn / cond_fn hooks (gaussian_diffusion.py:335-349, 374-384, 436-446;
respace.py:99-100, 117-129) on the HIP path - residue pinning fused into the loop (codlad_sample_loop_pinned), any
callable between the halves of the split step (codlad_ddpm_pred_xstart / codlad_ddpm_posterior_step) - against the
reference's own loops (g17 goldens, tests/guidance_cases.py), and `test.py --fix_residues` end to end.  The CPU part
checks argument validation: PinLatents, the residue spec and the new C entry points."""
import ctypes
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

from codlad_amd import _lib, synth
from codlad_amd.diffusion_and_flow import PinLatents, create_diffusion
from codlad_amd.diffusion_and_flow.schedule import Tables, named_betas, space_timesteps
from codlad_amd.models.latent_model import MPNN_models
from tests import cases
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


# ---------------------------------------------------------------------------------------- CPU --
def test_pin_latents_is_the_where_of_the_reference():
    x0, mask = gc.pin_inputs(20, 2, 5)
    x = synth.gaussian((2, 20, 3), 6)
    pin = PinLatents(x0, mask)
    assert torch.equal(pin(x), torch.where(mask[..., None], x0, x))
    assert torch.equal(pin(x)[mask], x0[mask]) and torch.equal(pin(x)[~mask], x[~mask])


def test_pin_latents_refuses_bad_shapes_and_dtypes():
    x0, mask = gc.pin_inputs(20, 2, 5)
    with pytest.raises(TypeError, match="x0 must be a floating-point"):
        PinLatents(x0.long(), mask)
    with pytest.raises(TypeError, match="x0 must be a floating-point"):
        PinLatents(x0.numpy(), mask)
    with pytest.raises(TypeError, match="mask must be a bool"):
        PinLatents(x0, mask.to(torch.uint8))
    with pytest.raises(ValueError, match="shape of x0 without its channel axis"):
        PinLatents(x0, mask[:, :10])
    with pytest.raises(ValueError, match="shape of x0 without its channel axis"):
        PinLatents(x0, mask[..., None].expand(2, 20, 3))
    with pytest.raises(ValueError, match="does not match x0"):
        PinLatents(x0, mask)(torch.zeros(2, 21, 3))


def test_hooks_must_be_callables_and_cpu_tensors_are_still_refused():
    from codlad_amd.models.latent_model import MPNN_models as M
    model = M["mpnn_diffusion"](input_size=3, unconditional=True, diffusion="diffusion", self_condition=False)
    prot, batch, x, t, mask = cases.denoiser_inputs(20, 2, 11)
    d = create_diffusion("10")
    kw = dict(y=None, mask=mask, batch=batch)
    with pytest.raises(TypeError, match="denoised_fn must be callable"):
        d.p_sample_loop(model.forward, x.shape, x, denoised_fn=3, model_kwargs=kw)
    with pytest.raises(TypeError, match="cond_fn must be callable"):
        next(d.p_sample_loop_progressive(model.forward, x.shape, x, cond_fn="grad", model_kwargs=kw))
    x0, pm = gc.pin_inputs(20, 2, 5)
    for hooks in (dict(denoised_fn=PinLatents(x0, pm)), dict(denoised_fn=gc.tanh_denoised_fn),
                  dict(cond_fn=gc.PullToTarget(x0))):
        with pytest.raises(RuntimeError, match="MI355X"):
            d.p_sample_loop(model.forward, x.shape, x, clip_denoised=False, model_kwargs=kw, **hooks)


def test_fixed_variances_are_the_reference_tables():
    tb = Tables(named_betas("linear", 1000), space_timesteps(1000, "10"))
    small, large = tb.step_variances("fixed_small"), tb.step_variances("fixed_large")
    assert small.dtype == np.float32 and small[0] == 0.0 and np.array_equal(small, tb.posterior_variance.astype(np.float32))
    assert large[0] == np.float32(tb.posterior_variance[1]) and np.array_equal(large[1:], tb.betas[1:].astype(np.float32))
    assert not tb.step_variances("learned_range").any()
    d = create_diffusion("10", learn_sigma=False)
    assert np.array_equal(d.fixed_variances(), large)
    with pytest.raises(ValueError):
        tb.step_variances("fixed_medium")


def test_fix_residues_spec_parsing_and_range():
    cli = cli_module()
    assert cli.parse_fix_residues("3-5,41") == [3, 4, 5, 41]
    assert cli.parse_fix_residues(" 7 , 2-3,3 ") == [2, 3, 7]
    assert cli.parse_fix_residues("1-46") == list(range(1, 47))
    for bad in ("", "  ", ",", "a", "3-", "-3", "0", "0-4", "5-3", "2,,4", "1.5", "3-4-5"):
        with pytest.raises(ValueError, match="--fix_residues"):
            cli.parse_fix_residues(bad)
    m = cli.fix_residue_mask([1, 3, 46], 46, 2)
    assert m.shape == (2, 46) and m.dtype == torch.bool and m.sum() == 6
    assert m[:, 0].all() and m[:, 2].all() and m[:, 45].all() and not m[:, 1].any()
    with pytest.raises(ValueError, match="out of range"):
        cli.fix_residue_mask([3, 47], 46, 2)


def test_fix_residues_is_refused_where_it_does_not_apply():
    cli = cli_module()
    base = dict(fix_residues="3-20,41", experiment="latent", model="diffusion", vae_type="N6", synthetic=True,
                pdb_files=None, data_process=False)
    assert cli.check_fix_residues(types.SimpleNamespace(**base)) == list(range(3, 21)) + [41]
    assert cli.check_fix_residues(types.SimpleNamespace(**dict(base, fix_residues=None))) is None
    for change, msg in ((dict(experiment="recon"), "--experiment latent"), (dict(model="fm"), "--model diffusion"),
                        (dict(vae_type="C2"), "VQ-VAE"), (dict(synthetic=False), "input with atoms"),
                        (dict(fix_residues="9-2"), "out of range"), (dict(fix_residues=""), "empty")):
        with pytest.raises(SystemExit, match=msg):
            cli.check_fix_residues(types.SimpleNamespace(**dict(base, **change)))
    for source in (dict(pdb_files=["a.pdb"]), dict(data_process=True)):
        assert cli.check_fix_residues(types.SimpleNamespace(**dict(base, synthetic=False, **source)))


def test_new_entry_points_validate_their_arguments():
    lib = _lib.lib()
    coef = (np.zeros(8, dtype=np.float32)).ctypes.data_as(_lib.P)
    one = torch.zeros(12)
    p = _lib.ptr(one)
    assert lib.codlad_ddpm_pred_xstart(None, p, coef, 4, p, None) == -1
    assert b"codlad_ddpm_pred_xstart: null pointer" in lib.codlad_last_error()
    assert lib.codlad_ddpm_pred_xstart(p, p, coef, 0, p, None) == -1
    assert b"n_nodes must be positive" in lib.codlad_last_error()
    assert lib.codlad_ddpm_posterior_step(p, None, p, p, None, coef, 0.0, 4, p, None, None) == -1
    assert b"codlad_ddpm_posterior_step: null pointer" in lib.codlad_last_error()
    assert lib.codlad_ddpm_posterior_step(p, p, p, p, None, coef, 0.0, -1, p, None, None) == -1
    assert b"n_nodes must be positive" in lib.codlad_last_error()
    job = _lib.JobDesc(p, 4, p, p, None, 1, None)
    assert lib.codlad_sample_loop_pinned(None, ctypes.byref(job), p, None, p, p, p, 10, p, p, None) == -1
    assert b"codlad_sample_loop_pinned: null pointer" in lib.codlad_last_error()


# ---------------------------------------------------------------------------------------- GPU --
def guided_model(kind):
    three, sc = kind == "three", kind == "selfcond"
    model = MPNN_models["mpnn_diffusion"](input_size=3, unconditional=True, diffusion="fm" if three else "diffusion",
                                          self_condition=sc)
    model.load_state_dict(synth.denoiser_state_dict(cases.WEIGHT_SEED, flow=three, self_condition=sc), strict=True)
    return model.to(DEV).eval()


def case_setup(name):
    L, B, seed, kw, clip, kind, _hooks = gc.GUIDANCE_CASES[name]
    model = guided_model(kind)
    prot, batch, _x, _t, mask = cases.denoiser_inputs(L, B, seed)
    batch = {k: (v.to(DEV) if hasattr(v, "to") else v) for k, v in batch.items()}
    z, eps = cases.loop_noise(gc.T, B, L, seed)
    diffusion = create_diffusion(str(gc.T), noise_schedule="linear", **kw)
    return model, diffusion, dict(y=None, mask=mask.to(DEV), batch=batch), z.to(DEV), eps.to(DEV), clip


@gpu
@pytest.mark.parametrize("name", list(gc.GUIDANCE_CASES))
def test_guidance_like_the_reference(name):
    """p_sample_loop(..., denoised_fn=, cond_fn=) against the reference's own loop: with the codlad_amd model (a PinLatents
    without cond_fn = the fused loop, anything else = the split per-step path) and with an arbitrary model callable
    (always per step); the two agree bit for bit, cond_fn is handed the original-process timesteps."""
    model, diffusion, kwargs, z, eps, clip = case_setup(name)
    gold = np.load(cases.npz_path(f"g17_guidance_{name}"))
    tol = gc.GUIDANCE_TOL.get(name, 2e-5)
    denoised_fn, cond_fn = gc.hooks_for(name, DEV)
    out = diffusion.p_sample_loop(model.forward, z.shape, z, clip_denoised=clip, denoised_fn=denoised_fn, cond_fn=cond_fn,
                                  model_kwargs=kwargs, device=DEV, step_noise=eps)
    err = rel_err(out, gold["sample"])
    assert err < tol, f"{name}: sample rel err {err:.3e}"
    denoised_fn, cond_fn = gc.hooks_for(name, DEV)
    traj = [o["sample"] for o in diffusion.p_sample_loop_progressive(lambda x, t, **k: model(x, t, **k), z.shape, z,
                                                                     clip_denoised=clip, denoised_fn=denoised_fn,
                                                                     cond_fn=cond_fn, model_kwargs=kwargs, device=DEV,
                                                                     step_noise=eps)]
    errs = [rel_err(traj[k], gold["traj"][k]) for k in range(gc.T)]
    assert max(errs) < tol, f"{name}: per-step trajectory rel err {['%.2e' % e for e in errs]}"
    assert torch.equal(traj[-1], out)
    if cond_fn is not None:
        assert cond_fn.timesteps == gold["cond_timesteps"].tolist() == [diffusion.timestep_map[i] for i in range(gc.T - 1, -1, -1)]


@gpu
@pytest.mark.parametrize("name", ["pin_eps_L46", "pin_clip_selfcond_L46", "pin_xstart_L87", "pin_fixed_small_L46"])
def test_fused_pin_equals_the_split_step(name):
    """The pin fused into final_kernel and PinLatents between codlad_ddpm_pred_xstart and codlad_ddpm_posterior_step round
    alike: the whole loop, trajectory end and the pred_xstart handed on, to the bit."""
    model, diffusion, kwargs, z, eps, clip = case_setup(name)
    pin, _ = gc.hooks_for(name, DEV)
    fused = diffusion.p_sample_loop(model.forward, z.shape, z, clip_denoised=clip, denoised_fn=pin, model_kwargs=kwargs,
                                    device=DEV, step_noise=eps)
    wrapped = lambda x: pin(x)                                              # noqa: E731  (not a PinLatents: per step)
    split = diffusion.p_sample_loop(model.forward, z.shape, z, clip_denoised=clip, denoised_fn=wrapped, model_kwargs=kwargs,
                                    device=DEV, step_noise=eps)
    assert torch.equal(fused, split)


@gpu
@pytest.mark.parametrize("name", ["pin_eps_L46", "pin_xstart_L87", "pin_fixed_small_L46"])
def test_pinned_nodes_end_exactly_on_their_latents(name):
    """Without clip_denoised the last step's table row is post_coef1 = 1, post_coef2 = 0, no noise: a pinned node ends on
    its latent exactly; the rest is sampled conditioned on the pins (it differs from the unpinned run on the same noise)."""
    model, diffusion, kwargs, z, eps, clip = case_setup(name)
    assert not clip
    c = diffusion.coefficients(clip)[0]
    assert c[2] == 1.0 and c[3] == 0.0 and c[6] == 0.0
    pin, _ = gc.hooks_for(name, DEV)
    out = diffusion.p_sample_loop(model.forward, z.shape, z, clip_denoised=False, denoised_fn=pin, model_kwargs=kwargs,
                                  device=DEV, step_noise=eps)
    free = diffusion.p_sample_loop(model.forward, z.shape, z, clip_denoised=False, model_kwargs=kwargs, device=DEV,
                                   step_noise=eps)
    m = pin.mask
    assert torch.equal(out[m], pin.x0[m])
    assert not torch.equal(out[~m], free[~m])
    assert bool(torch.isfinite(out).all())


@gpu
def test_two_streams_equal_one_stream_pinned_and_unpinned():
    """A job of 8 352 nodes (96 samples x 87 residues, above Denoiser.SPLIT_MIN_NODES) runs as two half-jobs on two HIP
    streams by default; the result is the one-stream loop's bit for bit, with and without a pin (the pin arrays are
    gathered per part exactly as x_T and the noise)."""
    model = guided_model("eps")
    eng = model.engine()
    L, frames, rep = 87, 8, 12
    prot, batch, _x, _t, _mask = cases.denoiser_inputs(L, frames, 91)
    batch = {k: (v.to(DEV) if hasattr(v, "to") else v) for k, v in batch.items()}
    job, lens = model.job_for(batch, rep)
    n = job.n_nodes
    assert n == 96 * 87 and n >= eng.SPLIT_MIN_NODES and len(job.parts(2)) == 2
    T = 10
    tables = create_diffusion(str(T))
    gen = torch.Generator(device=DEV).manual_seed(17)
    x_T = torch.randn(n, 3, device=DEV, generator=gen)
    noise = torch.randn(T, n, 3, device=DEV, generator=gen)
    x0 = torch.randn(n, 3, device=DEV, generator=gen)
    mask = torch.rand(n, device=DEV, generator=gen) < 0.25
    for pin in (None, (x0, mask)):
        one = eng.sample(job, x_T, noise, tables, streams=1, pin=pin)
        two = eng.sample(job, x_T, noise, tables, streams=2, pin=pin)
        default = eng.sample(job, x_T, noise, tables, pin=pin)
        assert torch.equal(one, two) and torch.equal(one, default)
        if pin is not None:
            assert torch.equal(one[mask], x0[mask])


@gpu
def test_sample_many_keeps_every_jobs_pin_arrays_until_the_streams_are_joined():
    """Two pinned jobs with boolean masks through Denoiser.sample_many: each result is that of `sample` on the job alone, bit
    for bit.  The masks are converted to uint8 - new tensors, on the caller's stream - before the jobs go to their side
    streams, and stay referenced until those have been joined; released after each job's enqueue, the first job's mask
    would be handed to the second job's conversion while the first loop still reads it."""
    eng = guided_model("eps").engine()
    prots = [synth.make_protein(L, 100 + L, n_frames=1) for L in (33, 65)]
    st = eng.prepare_structures([torch.from_numpy(p["xyz_full"])[0, 1:-1] for p in prots],
                                [torch.from_numpy(p["z_full"])[1:-1] for p in prots])
    jobs = [eng.make_job(st, [0, 1, 0]), eng.make_job(st, [1, 0])]
    T = 10
    tables = create_diffusion(str(T))
    gen = torch.Generator(device=DEV).manual_seed(23)
    x_Ts = [torch.randn(j.n_nodes, 3, device=DEV, generator=gen) for j in jobs]
    noises = [torch.randn(T, j.n_nodes, 3, device=DEV, generator=gen) for j in jobs]
    pins = [(torch.randn(j.n_nodes, 3, device=DEV, generator=gen), torch.rand(j.n_nodes, device=DEV, generator=gen) < 0.3)
            for j in jobs]
    for kind in ("ddpm", "ddim"):
        alone = [eng.sample(j, x, nz, tables, streams=1, pin=p, kind=kind) for j, x, nz, p in zip(jobs, x_Ts, noises, pins)]
        together = eng.sample_many(jobs, x_Ts, noises, tables, pins=pins, kind=kind)
        for a, b, (x0, mask) in zip(alone, together, pins):
            assert torch.equal(a, b)
            assert kind != "ddpm" or torch.equal(b[mask], x0[mask])


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
def test_cli_fix_residues(tmp_path):
    """test.py --fix_residues 1-46 on the synthetic PED set (structures of 46, 87, 92 and 129 residues): the 46-residue
    structure is pinned whole, so it decodes to exactly what --experiment recon decodes (the decoder sees only the VQ
    codes of the encoder's latents, and a pinned residue ends on its latent); in the longer ones the spec is partial -
    finite coordinates, different from an unpinned run on the same noise."""
    recon = _cli(["--experiment", "recon"], tmp_path / "recon")
    pinned = _cli(["--fix_residues", "1-46"], tmp_path / "pinned")
    free = _cli([], tmp_path / "free")
    assert np.array_equal(pinned(46), recon(46))
    assert not np.array_equal(free(46), recon(46))
    for L in (87, 92, 129):
        assert np.isfinite(pinned(L)).all() and pinned(L).shape == free(L).shape
        assert not np.array_equal(pinned(L), free(L))
    bad = subprocess.run([sys.executable, os.path.join(ROOT, "test.py"), "--synthetic", "--synthetic_weights",
                          "--synthetic_frames", "2", "--num_sampling_steps", "10", "--fix_residues", "40-47"],
                         env=dict(os.environ, PYTHONPATH=ROOT), cwd=str(tmp_path), capture_output=True, text=True,
                         timeout=600)
    assert bad.returncode != 0 and "out of range" in bad.stdout + bad.stderr
