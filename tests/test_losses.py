"""Forward-only loss evaluation on the HIP path (q_sample_kernel, loss_kernel, prior_kernel; codlad_q_sample,
codlad_q_posterior, codlad_vb_terms, codlad_loss_forward, codlad_bpd_loop) against the reference's own q_sample /
training_losses / _vb_terms_bpd and the restated calc_bpd_loop (g19 goldens, tests/loss_cases.py), the identities the
engine's grouping by timestep and its two-stream split rest on, the status word, and `test.py --experiment bpd`."""
import os
import random
import subprocess
import sys

import numpy as np
import pytest
import torch

from codlad_amd import synth
from codlad_amd.diffusion_and_flow import LossType, create_diffusion
from codlad_amd.engine import Denoiser
from codlad_amd.models.latent_model import MPNN_models
from tests import cases
from tests import loss_cases as lc
from tests.test_precision_envelope import job_of

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
PRECISIONS = ["f16x3", "f16x4", "f32"]          # the contraction modes of tests/test_hip_parity.py's `den` fixture
# tests/test_hip_parity.py::test_denoiser_forward holds the forward to this, per element, relative to the output's maximum
FORWARD_BOUND = 1e-5
CLASS_INDEX = {"kl": 0, "nll": 1, "mse": 2}
KEYS = ("kl", "nll", "vb", "mse", "xstart_mse", "eps_mse")


def model_of(kind, precision="f16x3"):
    three, sc = kind == "three", kind == "selfcond"
    model = MPNN_models["mpnn_diffusion"](input_size=3, unconditional=True, diffusion="fm" if three else "diffusion",
                                          self_condition=sc)
    model.load_state_dict(synth.denoiser_state_dict(cases.WEIGHT_SEED, flow=three, self_condition=sc), strict=True)
    model.precision = precision
    return model.to(DEV).eval()


def case_diffusion(kw, loss_type=None):
    d = create_diffusion(str(lc.T), noise_schedule="linear", **kw)
    if loss_type is not None:
        d.loss_type = LossType[loss_type]
    return d


def on_dev(batch, mask):
    return dict(y=None, mask=mask.to(DEV), batch={k: (v.to(DEV) if hasattr(v, "to") else v) for k, v in batch.items()})


def class_of(key, t):
    """The term class (tests/loss_cases.py) of a term at step t; vb is the nll at t = 0, else the kl."""
    return lc.TERM_CLASS[key] or ("nll" if t == 0 else "kl")


def used(key, t):
    """Everything but the nll at t > 0, which _vb_terms_bpd discards and which is rounding noise there (loss_cases.py)."""
    return not (key == "nll" and t > 0)


def kernel_bound(g, cls):
    """4 x the reference's own fp32-against-float64 deviation of the class (tests/loss_cases.py)."""
    return lc.REF_DEV_FACTOR * float(g["ref_dev"][CLASS_INDEX[cls]])


def check_terms(label, got, g, ts, extra=None, rows=None):
    """got[key] [N] against the golden's float64 terms (extra None: the kernel-level bound) or its fp32 terms (extra[key]
    [N]: the propagated allowance, absolute, added to the kernel-level bound).  Prints every figure, then asserts."""
    worst, failures = {}, []
    for key in KEYS:
        if key not in got:
            continue
        ref64 = np.asarray(g["f64_" + key] if rows is None else g["f64_" + key][rows], dtype=np.float64)
        ref = ref64 if extra is None else np.asarray(g["f32_" + key] if rows is None else g["f32_" + key][rows], dtype=np.float64)
        val = got[key].detach().cpu().double().numpy()
        for n, t in enumerate(ts):
            if not used(key, t):
                continue
            cls = class_of(key, t)
            allowed = kernel_bound(g, cls) * abs(ref64[n]) + (0.0 if extra is None else float(extra[key][n]))
            dev = abs(val[n] - ref[n])
            rel = dev / max(abs(ref64[n]), 1e-300)
            worst[cls] = max(worst.get(cls, 0.0), rel)
            if not dev <= allowed:
                failures.append((key, n, t, val[n], ref[n], dev, allowed))
    print(f"{label}: measured relative deviation per class {worst}; kernel-level bounds "
          f"{ {c: kernel_bound(g, c) for c in CLASS_INDEX} }")
    assert not failures, failures


# ------------------------------------------------------------------------------------ arithmetic --
@pytest.mark.parametrize("name", list(lc.LOSS_CASES))
def test_forward_process_is_bit_exact(name):
    """q_sample, q_mean_variance and q_posterior_mean_variance: unfused fp32 multiply-adds on the reference's fp32 table
    values, so the reference's bits, with a different timestep per sample."""
    L, B, seed, n_rep, kw, _lt, _kind, ts, _rs = lc.LOSS_CASES[name]
    g = np.load(cases.npz_path("g19_loss_" + name))
    _prot, _batch, _mask, x_start, noise = lc.inputs(L, B, seed, n_rep)
    x_start, noise = lc.stored_inputs(g, x_start, noise)
    d = case_diffusion(kw)
    x0, nz, t = x_start.to(DEV), noise[0].to(DEV), torch.tensor(ts, device=DEV)
    x_t = d.q_sample(x0, t, noise=nz)
    assert np.array_equal(x_t.cpu().numpy(), g["x_t"])
    for got, key in zip(d.q_mean_variance(x0, t), ("q_mean", "q_variance", "q_log_variance")):
        assert np.array_equal(got.cpu().numpy(), g[key]), key
    for got, key in zip(d.q_posterior_mean_variance(x0, x_t, t), ("post_mean", "post_variance", "post_log_variance")):
        assert np.array_equal(got.cpu().numpy(), g[key]), key


@pytest.mark.parametrize("name", list(lc.LOSS_CASES))
def test_vb_terms_on_the_references_model_output(name):
    """codlad_vb_terms on the golden's model output against the golden's float64 terms: at most 4 x ref_dev per class."""
    L, B, seed, n_rep, kw, _lt, _kind, ts, _rs = lc.LOSS_CASES[name]
    g = np.load(cases.npz_path("g19_loss_" + name))
    _prot, _batch, _mask, x_start, noise = lc.inputs(L, B, seed, n_rep)
    x_start, noise = lc.stored_inputs(g, x_start, noise)
    d = case_diffusion(kw)
    out = torch.from_numpy(g["model_out"]).to(DEV)
    got = Denoiser.vb_terms(out.reshape(-1, out.shape[-1]), x_start.reshape(-1, 3).to(DEV),
                            torch.from_numpy(g["x_t"]).reshape(-1, 3).to(DEV), noise[0].reshape(-1, 3).to(DEV),
                            [L] * len(ts), list(ts), d.loss_coefs(False))
    check_terms(name, got, g, ts)
    # pred_xstart is elementwise: the reference's bits
    assert np.array_equal(got["pred_xstart"].cpu().view(len(ts), L, 3).numpy(), g["pred_xstart"])


@pytest.mark.parametrize("name", list(lc.BPD_CASES))
def test_vb_terms_on_the_bound_loops_model_outputs(name):
    L, B, seed, kw, _kind, clip = lc.BPD_CASES[name]
    g = np.load(cases.npz_path("g19_" + name))
    _prot, _batch, _mask, x_start, eps = lc.inputs(L, B, seed, 1, n_steps=lc.T)
    x_start, eps = lc.stored_inputs(g, x_start, eps)
    d = case_diffusion(kw)
    for k, i in enumerate(range(lc.T - 1, -1, -1)):
        out = torch.from_numpy(g["model_out"][k]).to(DEV)
        got = Denoiser.vb_terms(out.reshape(-1, out.shape[-1]), x_start.reshape(-1, 3).to(DEV),
                                torch.from_numpy(g["x_t"][k]).reshape(-1, 3).to(DEV), eps[k].reshape(-1, 3).to(DEV),
                                [L] * B, i, d.loss_coefs(clip))
        check_terms(f"{name} step {i}", got, g, [i] * B, rows=k)


# ------------------------------------------------------------------------------------ end to end --
def propagated(tables, g_out, x_start, x_t, noise, ts, kw, clip):
    """key -> [N]: what a term may move, to first order doubled, when every element of the model output moves by the
    forward's bound: 2 x sum |d term / d out| x FORWARD_BOUND x max |out|, the sum by autograd through the float64
    restatement at the golden's model output."""
    px, var = lc.diffusion_flags(kw)
    delta = FORWARD_BOUND * float(np.abs(g_out).max())
    with torch.enable_grad():
        out = torch.from_numpy(g_out).double().requires_grad_(True)
        terms = lc.terms64(tables, out, x_start, x_t, noise, torch.tensor(ts), predict_xstart=px, var_type=var,
                           clip_denoised=clip)
        res = {}
        for key in KEYS:
            rows = []
            for n in range(len(ts)):
                grad, = torch.autograd.grad(terms[key][n], out, retain_graph=True, allow_unused=True)
                rows.append(0.0 if grad is None else 2.0 * float(grad.abs().sum()) * delta)
            res[key] = rows
    return res


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", list(lc.LOSS_CASES))
def test_training_losses_end_to_end(name, precision):
    """training_losses with the HIP model against the reference's fp32 results: per-sample timesteps (grouped by t inside),
    every mean / variance / loss type, self-conditioning on both sides of the reference's random() draw."""
    L, B, seed, n_rep, kw, loss_type, kind, ts, rseed = lc.LOSS_CASES[name]
    g = np.load(cases.npz_path("g19_loss_" + name))
    _prot, batch, mask, x_start, noise = lc.inputs(L, B, seed, n_rep)
    x_start, noise = lc.stored_inputs(g, x_start, noise)
    d = case_diffusion(kw, loss_type)
    model = model_of(kind, precision)
    if rseed is not None:
        random.seed(rseed)
    t = torch.tensor(ts, device=DEV)
    losses = d.training_losses(model.forward, x_start.to(DEV), t, model_kwargs=on_dev(batch, mask), noise=noise[0].to(DEV))
    if rseed is not None:                       # exactly one draw was consumed, where the reference consumes it
        after = random.random()
        random.seed(rseed)
        assert random.random() == float(g["random_draw"]) and random.random() == after
    assert set(losses) == {k[len("loss_"):] for k in g.files if k.startswith("loss_")}
    allow = propagated(d, g["model_out"], x_start, torch.from_numpy(g["x_t"]), noise[0], ts, kw, False)
    scale = {LossType.RESCALED_KL: float(lc.T), LossType.RESCALED_MSE: lc.T / 1000.0}.get(d.loss_type, 1.0)
    worst, failures = {}, []
    for key, val in losses.items():
        ref = g["loss_" + key].astype(np.float64)
        val = val.cpu().double().numpy()
        assert val.shape == (len(ts),)
        for n, tv in enumerate(ts):
            parts = {"mse": [("mse", 1.0)], "vb": [("vb", scale)], "loss": [("vb", scale)] if d.loss_type.is_vb() else
                     [("mse", 1.0)] + ([("vb", scale)] if "vb" in losses else [])}[key]
            allowed = sum(s * (allow[p][n] + kernel_bound(g, class_of(p, tv)) * abs(float(g["f64_" + p][n]))) for p, s in parts)
            dev = abs(val[n] - ref[n])
            worst[key] = max(worst.get(key, 0.0), dev / abs(ref[n]))
            if not dev <= allowed:
                failures.append((key, n, tv, val[n], ref[n], dev, allowed))
    print(f"{name} {precision}: measured relative deviation {worst}")
    assert not failures, failures


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", list(lc.BPD_CASES))
def test_calc_bpd_loop_end_to_end(name, precision):
    """calc_bpd_loop, fused (one codlad_bpd_loop call), against the reference's functions in the restated loop."""
    L, B, seed, kw, kind, clip = lc.BPD_CASES[name]
    g = np.load(cases.npz_path("g19_" + name))
    _prot, batch, mask, x_start, eps = lc.inputs(L, B, seed, 1, n_steps=lc.T)
    x_start, eps = lc.stored_inputs(g, x_start, eps)
    d = case_diffusion(kw)
    model = model_of(kind, precision)
    r = d.calc_bpd_loop(model.forward, x_start.to(DEV), clip_denoised=clip, model_kwargs=on_dev(batch, mask),
                        step_noise=eps.to(DEV))
    assert set(r) == {"total_bpd", "prior_bpd", "vb", "xstart_mse", "mse"}
    for key in ("vb", "xstart_mse", "mse"):
        assert tuple(r[key].shape) == (B, lc.T)
    total_allowed = np.zeros(B)
    for k, i in enumerate(range(lc.T - 1, -1, -1)):
        allow = propagated(d, g["model_out"][k], x_start, torch.from_numpy(g["x_t"][k]), eps[k], [i] * B, kw, clip)
        got = {"vb": r["vb"][:, k], "xstart_mse": r["xstart_mse"][:, k], "eps_mse": r["mse"][:, k]}
        check_terms(f"{name} {precision} step {i}", got, g, [i] * B, extra=allow, rows=k)
        total_allowed += np.asarray(allow["vb"]) + kernel_bound(g, class_of("vb", i)) * np.abs(g["f64_vb"][k])
    # the prior: the kl class's bound on the float64 restatement's value
    prior = r["prior_bpd"].cpu().double().numpy()
    prior_allowed = kernel_bound(g, "kl") * np.abs(g["f64_prior_bpd"])
    print(f"{name} {precision}: prior {prior} against {g['f64_prior_bpd']} (allowed {prior_allowed})")
    assert (np.abs(prior - g["f64_prior_bpd"]) <= prior_allowed).all()
    total = r["total_bpd"].cpu().double().numpy()
    print(f"{name} {precision}: total {total} against {g['total_bpd']} (allowed {total_allowed + prior_allowed})")
    assert (np.abs(total - g["total_bpd"].astype(np.float64)) <= total_allowed + prior_allowed).all()


# ------------------------------------------------------------------------------------ identities --
def engine_case(precision="f16x3", L=46, B=2, seed=101, n_rep=2, kind="eps"):
    prot, batch, mask, x_start, noise = lc.inputs(L, B, seed, n_rep, n_steps=lc.T)
    sd = synth.denoiser_state_dict(cases.WEIGHT_SEED, flow=kind == "three", self_condition=kind == "selfcond")
    den = Denoiser(sd, DEV, precision=precision, self_condition=kind == "selfcond", out_dim=3 if kind == "three" else 6)
    frames = torch.from_numpy(prot["xyz_full"])[:, 1:-1]
    z = torch.from_numpy(prot["z_full"])[1:-1]
    st = den.prepare_structures([f for f in frames], [z for _ in frames])
    job = den.make_job(st, list(range(B)) * n_rep)
    return den, st, job, x_start.reshape(-1, 3).to(DEV), noise.reshape(lc.T, -1, 3).to(DEV)


def same(a, b):
    assert set(a) == set(b)
    for k in a:
        assert torch.equal(a[k], b[k]), k


@pytest.mark.parametrize("precision", PRECISIONS)
def test_loss_head_gives_final_kernels_logits(precision):
    """loss_kernel's head (LayerNorm, modulation, Linear 128 -> 6) on the h_V of a forward: the bits of final_kernel's
    logits mode on the same job."""
    den, _st, job, x0, noise = engine_case(precision)
    tb = create_diffusion(str(lc.T))
    x_t = den.q_sample(job, x0, 4, noise[0], tb)
    r = den.loss_terms(job, x0, 4, noise[0], tb, want_model_out=True)
    out = den.forward(job, x_t, tb.timestep_map[4])
    assert torch.equal(r["model_out"], out)
    three = engine_case(precision, kind="three")
    tb3 = create_diffusion(str(lc.T), learn_sigma=False)
    r = three[0].loss_terms(three[2], three[3], 4, three[4][0], tb3, coef=tb3.loss_coefs(False), want_model_out=True)
    x_t = three[0].q_sample(three[2], three[3], 4, three[4][0], tb3)
    assert torch.equal(r["model_out"], three[0].forward(three[2], x_t, tb3.timestep_map[4]))


def test_per_sample_timesteps_equal_the_union_of_shared_timestep_calls():
    den, st, job, x0, noise = engine_case()
    tb = create_diffusion(str(lc.T))
    ts = [9, 0, 5, 0]
    L = job.sample_lens[0]
    mixed = den.loss_terms(job, x0, ts, noise[0], tb, want_model_out=True)
    for tv in sorted(set(ts)):
        members = [m for m in range(4) if ts[m] == tv]
        sub = den.make_job(st, [job.sample_struct[m] for m in members])
        idx = torch.cat([torch.arange(m * L, (m + 1) * L) for m in members]).to(DEV)
        alone = den.loss_terms(sub, x0[idx], tv, noise[0][idx], tb, want_model_out=True)
        for k, v in alone.items():
            per_node = k in ("pred_xstart", "model_out")
            assert torch.equal(mixed[k][idx] if per_node else mixed[k][torch.tensor(members, device=DEV)], v), (k, tv)
    # ... and twice the same bits (the second call finds its sub-jobs cached)
    same(mixed, den.loss_terms(job, x0, ts, noise[0], tb, want_model_out=True))


def test_fused_bound_loop_equals_stepping():
    """codlad_bpd_loop = q_sample, codlad_loss_forward per step and the prior, bit for bit; a self-conditioned model is
    conditioned on zeros in both."""
    for kind in ("eps", "selfcond"):
        den, _st, job, x0, noise = engine_case(kind=kind)
        tb = create_diffusion(str(lc.T), self_condition=kind == "selfcond")
        fused = den.bpd(job, x0, noise, tb, streams=1)
        for k, i in enumerate(range(lc.T - 1, -1, -1)):
            r = den.loss_terms(job, x0, i, noise[k], tb)
            assert torch.equal(fused["vb"][i], r["vb"]) and torch.equal(fused["mse"][i], r["eps_mse"])
            assert torch.equal(fused["xstart_mse"][i], r["xstart_mse"])
        assert bool(torch.isfinite(fused["total_bpd"]).all())
        same(fused, den.bpd(job, x0, noise, tb, streams=1))                   # two runs: the same bits


def test_two_streams_equal_one_and_a_row_ignores_its_neighbours():
    den, st, job, x0, noise = engine_case()
    tb = create_diffusion(str(lc.T))
    one = den.bpd(job, x0, noise, tb, streams=1)
    same(one, den.bpd(job, x0, noise, tb, streams=2))
    # sample 1 alone, and in a ragged job beside a structure of another length
    L = job.sample_lens[0]
    alone = den.bpd(den.make_job(st, [job.sample_struct[1]]), x0[L:2 * L], noise[:, L:2 * L], tb, streams=1)
    for k in one:
        assert torch.equal(one[k][..., 1], alone[k][..., 0]), k
    other = synth.make_protein(31, 77, n_frames=1)
    frames = torch.from_numpy(other["xyz_full"])[:, 1:-1]
    prot = cases.denoiser_inputs(46, 2, 101)[0]
    f46 = torch.from_numpy(prot["xyz_full"])[:, 1:-1]
    st2 = den.prepare_structures([frames[0], f46[1]], [torch.from_numpy(other["z_full"])[1:-1],
                                                       torch.from_numpy(prot["z_full"])[1:-1]])
    job2 = den.make_job(st2, [0, 1])
    x2 = torch.cat([synth.gaussian((31, 3), 5).to(DEV), x0[L:2 * L]])
    n2 = torch.cat([synth.gaussian((lc.T, 31, 3), 6).to(DEV), noise[:, L:2 * L]], dim=1)
    ragged = den.bpd(job2, x2, n2, tb, streams=1)
    for k in one:
        assert torch.equal(one[k][..., 1], ragged[k][..., 1]), k


@pytest.mark.parametrize("precision", ["f16x3", "f16x4"])
def test_status_word_raises_from_the_loss_path(precision):
    """The weights of test_precision_envelope.test_fp16_range_overflow_is_an_error_not_a_number (edge features far outside
    the fp16 range): the loss paths report it through the status word as the sampling loop does."""
    L, B, seed = cases.ENVELOPE_GEOMETRY
    prot, _batch, _x, _t, _mask = cases.denoiser_inputs(L, B, seed)
    sd = synth.denoiser_state_dict(cases.WEIGHT_SEED)
    sd["features.norm_edges.weight"] = sd["features.norm_edges.weight"] * 1e6
    den = Denoiser(sd, DEV, precision=precision)
    job = job_of(den, prot, B)
    z, eps = cases.loop_noise(lc.T, B, L, seed)
    x0, eps = z.reshape(-1, 3).to(DEV), eps.reshape(lc.T, -1, 3).to(DEV)
    tb = create_diffusion(str(lc.T))
    with pytest.raises(RuntimeError, match="not finite"):
        den.loss_terms(job, x0, 3, eps[0], tb)
    with pytest.raises(RuntimeError, match="not finite"):
        den.loss_terms(job, x0, [3, 7], eps[0], tb)
    with pytest.raises(RuntimeError, match="not finite"):
        den.bpd(job, x0, eps, tb, streams=1)
    assert int(job.status.item()) == 0


def test_existing_refusals_stay():
    d = create_diffusion(str(lc.T))
    model = model_of("eps")
    name, lengths, seed = cases.PADDED_CASE
    batch, x, _t, mask = cases.padded_inputs(lengths, seed)
    with pytest.raises(NotImplementedError, match="padded mixed-length"):
        d.training_losses(model.forward, x.to(DEV), torch.tensor([1, 2, 3], device=DEV), model_kwargs=on_dev(batch, mask))
    with pytest.raises(NotImplementedError, match="channel width"):
        d.q_sample(torch.zeros(2, 5, 2, device=DEV), torch.tensor([1, 2], device=DEV))
    prot, batch, x, _t, mask = cases.denoiser_inputs(20, 2, 11)
    with pytest.raises(NotImplementedError, match="per-sample timesteps"):
        model(x.to(DEV), torch.tensor([1, 2], device=DEV), None, **{k: v for k, v in on_dev(batch, mask).items() if k != "y"})
    # a foreign callable is stepped with codlad_vb_terms: the same numbers as the fused path on the same model
    kwargs = on_dev(batch, mask)
    t = torch.tensor([2, 2], device=DEV)
    nz = synth.gaussian(tuple(x.shape), 3).to(DEV)
    fused = d.training_losses(model.forward, x.to(DEV), t, model_kwargs=kwargs, noise=nz)
    foreign = d.training_losses(lambda a, b, **k: model(a, b, **k), x.to(DEV), t, model_kwargs=kwargs, noise=nz)
    for k in fused:
        assert torch.equal(fused[k], foreign[k]), k


# ------------------------------------------------------------------------------------------ CLI --
def test_cli_experiment_bpd(tmp_path):
    cmd = [sys.executable, os.path.join(ROOT, "test.py"), "--synthetic", "--synthetic_weights", "--experiment", "bpd",
           "--num_sampling_steps", "10", "--exp", "clitest"]
    env = dict(os.environ, PYTHONPATH=ROOT)
    res = subprocess.run(cmd, env=env, cwd=str(tmp_path), capture_output=True, text=True, timeout=900)
    assert res.returncode == 0, res.stdout[-1500:] + res.stderr[-3000:]
    import re
    totals = re.findall(r"total_bpd (\S+) prior_bpd (\S+):", res.stdout)
    assert len(totals) == 4, res.stdout[-1500:]                    # one line per synthetic PED file
    for total, prior in totals:
        assert np.isfinite(float(total)) and np.isfinite(float(prior)), (total, prior)
    found = {}
    for root, _dirs, files in os.walk(str(tmp_path)):
        for f in files:
            for key in ("vb", "mse", "xstart_mse"):
                if f.endswith(f"_bpd_{key}.npy"):
                    found.setdefault(key, []).append(np.load(os.path.join(root, f)))
    assert set(found) == {"vb", "mse", "xstart_mse"}
    for key, arrays in found.items():
        for a in arrays:
            assert a.ndim == 2 and a.shape[1] == 10 and np.isfinite(a).all(), (key, a.shape)
    two = subprocess.run(cmd, env=dict(env, WORLD_SIZE="2", RANK="0", LOCAL_RANK="0"), cwd=str(tmp_path), capture_output=True,
                         text=True, timeout=600)
    assert two.returncode != 0 and "--experiment bpd runs on one rank" in two.stdout + two.stderr
