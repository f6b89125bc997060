"""Flow-matching loss evaluation on the HIP path (fm_path_kernel, fm_loss_kernel; codlad_fm_path, codlad_fm_terms,
codlad_fm_loss_forward, codlad_fm_loss_loop) against the reference's own matchers, flow model and loss_fn (g20 goldens,
tests/flow_loss_cases.py), the identities the engine's grouping by time and its two-stream split rest on, the status word,
and `test.py --experiment fmloss`."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from codlad_amd import synth
from codlad_amd.diffusion_and_flow import flow
from codlad_amd.engine import Denoiser
from codlad_amd.models.latent_model import MPNN_models
from tests import cases
from tests import flow_loss_cases as fc
from tests import flow_loss_ref as fr
from tests.test_precision_envelope import job_of

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
PRECISIONS = ["f16x3", "f16x4", "f32"]
KEYS = fc.LOSS_TYPES
MATCHER = {"icfm": flow.ConditionalFlowMatcher, "target": flow.TargetConditionalFlowMatcher,
           "vp": flow.VariancePreservingConditionalFlowMatcher}
RAGGED_LENS = (5, 9, 46)            # idle half waves, the first wrap, the general case
RAGGED_TIMES = (0.2, 0.55, 0.9)


def flow_sd():
    return synth.denoiser_state_dict(cases.WEIGHT_SEED, flow=True)


def model_of(precision="f16x3"):
    model = MPNN_models["mpnn_diffusion"](input_size=3, unconditional=True, diffusion="fm", self_condition=False)
    model.load_state_dict(flow_sd(), strict=True)
    model.precision = precision
    return model.to(DEV).eval()


def on_dev(batch, mask):
    return dict(y=None, mask=mask.to(DEV), batch={k: (v.to(DEV) if hasattr(v, "to") else v) for k, v in batch.items()})


def kernel_bound(g, key):
    return fc.REF_DEV_FACTOR * float(g["ref_dev"][fc.REF_DEV_INDEX[key]])


def same(a, b, keys=None):
    for k in keys or a:
        assert torch.equal(a[k], b[k]), k


def ragged(precision="f16x3", sd=None):
    """(engine, structures, the job of RAGGED_LENS, x0, x1 [60, 3], eps [3, 60, 3])."""
    den = Denoiser(sd or flow_sd(), DEV, precision=precision)
    prots = [synth.make_protein(L, 900 + i, n_frames=1) for i, L in enumerate(RAGGED_LENS)]
    st = den.prepare_structures([torch.from_numpy(p["xyz_full"])[0, 1:-1] for p in prots],
                                [torch.from_numpy(p["z_full"])[1:-1] for p in prots])
    job = den.make_job(st, [0, 1, 2])
    n = sum(RAGGED_LENS)
    return (den, st, job, synth.gaussian((n, 3), 4100).to(DEV), synth.gaussian((n, 3), 4200).to(DEV),
            synth.gaussian((3, n, 3), 4300).to(DEV))


def l46(precision="f16x3"):
    """(engine, the job of L46_B2, x0, x1 [92, 3], eps [3, 92, 3])."""
    prot, _batch, _mask, x0, x1 = fc.inputs("L46_B2", 1)
    den = Denoiser(flow_sd(), DEV, precision=precision)
    return (den, job_of(den, prot, 2), x0.reshape(-1, 3).to(DEV), x1.reshape(-1, 3).to(DEV),
            synth.gaussian((3, 92, 3), 4400).to(DEV))


# ------------------------------------------------------------------------------------ 1. the path --
@pytest.mark.parametrize("name", list(fc.FM_CASES))
def test_path_against_the_reference(name):
    """ICFM and TARGET: the reference's bits (unfused fp32 operations in its order, the correctly rounded division); VP:
    every element within 4 x ref_dev (relative to the quantity's maximum) of the reference's float64 evaluation."""
    geometry, kind, sigma, n_rep, case_t = fc.FM_CASES[name]
    _p, _batch, _mask, x0, x1 = fc.inputs(geometry, n_rep)
    g = fc.load(name)
    t = fc.times(case_t, x1.shape[0]).to(DEV)
    x0, x1, eps = x0.to(DEV), x1.to(DEV), torch.from_numpy(g["eps"]).to(DEV)
    fm = MATCHER[kind](sigma)
    xt = fm.sample_xt(x0, x1, t, eps)
    ut = fm.compute_conditional_flow(x0, x1, t, xt)
    for label, got, key in (("xt", xt, "xt"), ("ut", ut, "ut")):
        got = got.cpu().numpy()
        ulps = np.abs(got.view(np.int32).astype(np.int64) - g[key].view(np.int32).astype(np.int64)).max()
        dev = np.abs(got.astype(np.float64) - g["f64_" + key]).max() / np.abs(g["f64_" + key]).max()
        print(f"{name} {label}: largest distance to the reference's fp32 {ulps} ulp; to its float64 {dev:.3e} of the maximum")
        if kind != "vp":
            assert np.array_equal(got, g[key]), label
        else:
            bound = fc.REF_DEV_FACTOR * float(g["ref_dev"][fc.REF_DEV_INDEX["vp_" + label]])
            assert (np.abs(got.astype(np.float64) - g["f64_" + key]) <= bound * np.abs(g["f64_" + key]).max()).all(), label
    # the pieces agree with one another: the mean is the path without noise, sigma_t the reference's expression
    mu = fm.compute_mu_t(x0, x1, t)
    zero = torch.zeros_like(eps)
    if kind == "target":
        assert torch.equal(mu, fm.sample_xt(x0, x1, t, zero))
        c = torch.tensor(1.0 - sigma, dtype=torch.float64).float()
        assert torch.equal(fm.compute_sigma_t(t).cpu(), 1 - c * t.cpu())
    else:
        assert torch.equal(mu, MATCHER[kind](0.0).sample_xt(x0, x1, t, zero)) and fm.compute_sigma_t(t) == sigma
    # sample_location_and_conditional_flow: t as given, the noise it drew returned, xt and ut those of the pieces
    torch.manual_seed(5)
    t2, xt2, ut2, eps2 = fm.sample_location_and_conditional_flow(x0, x1, t=t, return_noise=True)
    torch.manual_seed(5)
    assert torch.equal(eps2, torch.randn_like(x0)) and torch.equal(t2, t)
    assert torch.equal(xt2, fm.sample_xt(x0, x1, t, eps2)) and torch.equal(ut2, fm.compute_conditional_flow(x0, x1, t, xt2))
    torch.manual_seed(6)
    t3, xt3, _ut3 = fm.sample_location_and_conditional_flow(x0, x1)
    torch.manual_seed(6)
    assert torch.equal(t3, torch.sigmoid(torch.randn(x0.shape[0]).to(DEV))) and bool(torch.isfinite(xt3).all())


# ------------------------------------------------------------------------------------ 2. the terms --
def check_terms(label, got, g, extra=None, rows=None):
    """got[key] [N] against the golden's float64 terms (extra None: the kernel-level bound) or its fp32 terms (extra[key]
    [N]: the propagated allowance, absolute, added to the kernel-level bound).  Prints every figure, then asserts."""
    worst, failures = {}, []
    for key in KEYS:
        ref64 = np.asarray(g["f64_" + key] if rows is None else g["f64_" + key][rows], dtype=np.float64)
        ref = ref64 if extra is None else np.asarray(g["f32_" + key] if rows is None else g["f32_" + key][rows], dtype=np.float64)
        val = got[key].detach().cpu().double().numpy()
        assert val.shape == ref.shape, (key, val.shape, ref.shape)
        for n in range(len(val)):
            allowed = kernel_bound(g, key) * abs(ref64[n]) + (0.0 if extra is None else float(extra[key][n]))
            dev = abs(val[n] - ref[n])
            worst[key] = max(worst.get(key, 0.0), dev / abs(ref64[n]))
            if not dev <= allowed:
                failures.append((key, n, val[n], ref[n], dev, allowed))
    print(f"{label}: measured relative deviation {worst}; kernel-level bounds { {k: kernel_bound(g, k) for k in KEYS} }")
    assert not failures, failures


@pytest.mark.parametrize("name", list(fc.FM_CASES))
def test_terms_on_the_references_model_output(name):
    """codlad_fm_terms on the golden's model output and ut against the golden's float64 terms: at most 4 x ref_dev."""
    g = fc.load(name)
    vt, ut = torch.from_numpy(g["model_out"]).to(DEV), torch.from_numpy(g["ut"]).to(DEV)
    N, L, _ = vt.shape
    got = Denoiser.fm_terms(vt.reshape(-1, 3), ut.reshape(-1, 3), [L] * N)
    check_terms(name, got, g)
    assert torch.equal(got["huber"], got["smooth_l1"])
    for k in KEYS:                                                           # loss_fn: the batch scalar, on the host
        want = float(g[f"f64_batch_{k}"])
        assert abs(float(flow.loss_fn(vt, ut, loss_type=k)) - want) <= kernel_bound(g, k) * abs(want), k


def test_terms_of_short_samples_follow_the_fixed_order():
    """Lengths 5, 8, 9 and 46 (idle half waves, one node per half wave, the first wrap, the general case) in one call: the
    arithmetic losses are the bits of the restated fixed-order fp32 sum, log_cosh (the device's logf / coshf) is inside
    its bound; differences on both sides of Huber's threshold."""
    lens = [5, 8, 9, 46]
    g = fc.load("icfm_s0_L46")
    vt, ut = 1.5 * synth.gaussian((sum(lens), 3), 4500), synth.gaussian((sum(lens), 3), 4600)
    assert bool(((vt - ut).abs() < 1).any()) and bool(((vt - ut).abs() > 1).any())
    got = Denoiser.fm_terms(vt.to(DEV), ut.to(DEV), lens)
    off = 0
    for s, L in enumerate(lens):
        a, b = vt[off:off + L][None], ut[off:off + L][None]
        want32, want64 = fr.terms32(a, b), fr.terms64(a, b)
        for k in ("l2", "l1", "huber", "smooth_l1"):
            assert got[k][s].item() == want32[k][0].item(), (k, L)
        rel = abs(got["log_cosh"][s].item() - want64["log_cosh"][0].item()) / want64["log_cosh"][0].item()
        print(f"L = {L}: log_cosh relative deviation {rel:.3e} (bound {kernel_bound(g, 'log_cosh'):.3e})")
        assert rel <= kernel_bound(g, "log_cosh"), L
        off += L


# ------------------------------------------------------------------------------------ 3. end to end --
def propagated(g_out, g_ut):
    """key -> [N]: what a term may move, to first order doubled, when every element of the model output moves by the
    forward's bound: 2 x sum |d term / d out| x FORWARD_BOUND x max |out|, the sum by autograd through the float64
    restatement at the golden's model output (tests/test_losses.py's allowance)."""
    delta = fc.FORWARD_BOUND * float(np.abs(g_out).max())
    with torch.enable_grad():
        out = torch.from_numpy(g_out).double().requires_grad_(True)
        terms = fr.terms64(out, torch.from_numpy(g_ut))
        res = {}
        for key in KEYS:
            rows = []
            for n in range(out.shape[0]):
                grad, = torch.autograd.grad(terms[key][n], out, retain_graph=True)
                rows.append(2.0 * float(grad.abs().sum()) * delta)
            res[key] = rows
    return res


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", list(fc.FM_CASES))
def test_training_losses_end_to_end(name, precision):
    """training_losses with the HIP model (per-sample times, grouped inside) against the reference's fp32 results."""
    geometry, kind, sigma, n_rep, case_t = fc.FM_CASES[name]
    _p, batch, mask, x0, x1 = fc.inputs(geometry, n_rep)
    g = fc.load(name)
    t = fc.times(case_t, x1.shape[0]).to(DEV)
    model = model_of(precision)
    r = MATCHER[kind](sigma).training_losses(model.forward, x0.to(DEV), x1.to(DEV), t=t, eps=torch.from_numpy(g["eps"]).to(DEV),
                                             model_kwargs=on_dev(batch, mask), loss_type="huber")
    assert set(r) == {"loss", "per_sample", "t", "terms"} and set(r["terms"]) == set(KEYS)
    assert torch.equal(r["t"], t) and torch.equal(r["per_sample"], r["terms"]["huber"])
    allow = propagated(g["model_out"], g["ut"])
    check_terms(f"{name} {precision}", r["terms"], g, extra=allow)
    # the batch scalar: a weighted mean of the per-sample means, so the mean of their allowances holds it
    want = float(g["f32_batch_huber"])
    allowed = float(np.mean(allow["huber"])) + kernel_bound(g, "huber") * abs(float(g["f64_batch_huber"]))
    assert r["loss"].dtype == torch.float64 and abs(float(r["loss"]) - want) <= allowed


@pytest.mark.parametrize("precision", PRECISIONS)
def test_loss_sweep_end_to_end(precision):
    """loss_sweep with the HIP model (one codlad_fm_loss_loop call) against the reference's fp32 results per time."""
    name = "sweep_icfm_L46"
    geometry, kind, sigma, ts = fc.SWEEP_CASES[name]
    _p, batch, mask, x0, x1 = fc.inputs(geometry, 1)
    g = fc.load(name)
    r = MATCHER[kind](sigma).loss_sweep(model_of(precision).forward, x0.to(DEV), x1.to(DEV), ts,
                                        step_noise=torch.from_numpy(g["eps"]).to(DEV), model_kwargs=on_dev(batch, mask))
    N, K = x1.shape[0], len(ts)
    assert tuple(r["loss"].shape) == (K,) and tuple(r["per_sample"].shape) == (N, K)
    assert all(tuple(v.shape) == (N, K) for v in r["terms"].values())
    for k in range(K):
        allow = propagated(g["model_out"][k], g["ut"][k])
        check_terms(f"{name} {precision} t = {ts[k]}", {key: v[:, k] for key, v in r["terms"].items()}, g, extra=allow, rows=k)
        allowed = float(np.mean(allow["l2"])) + kernel_bound(g, "l2") * abs(float(g["f64_batch_l2"][k]))
        assert abs(float(r["loss"][k]) - float(g["f32_batch_l2"][k])) <= allowed


# ------------------------------------------------------------------------------------ 4 - 8. identities --
@pytest.mark.parametrize("precision", PRECISIONS)
def test_loss_head_gives_the_forwards_output(precision):
    """fm_loss_kernel's head on the h_V of a forward: the bits of Denoiser.forward at the same time."""
    den, job, x0, x1, eps = l46(precision)
    r = den.fm_loss_terms(job, x1, 0.37, kind="icfm", sigma=0.1, x0=x0, eps=eps[0], want_model_out=True)
    assert torch.equal(r["model_out"], den.forward(job, r["xt"], float(np.float32(0.37))))
    assert bool(torch.isfinite(r["l2"]).all())


def test_per_sample_times_equal_each_sample_alone():
    den, st, job, x0, x1, eps = ragged()
    mixed = den.fm_loss_terms(job, x1, RAGGED_TIMES, kind="target", sigma=0.1, eps=eps[0], want_model_out=True)
    for s, tv in enumerate(RAGGED_TIMES):
        a, b = int(job.sample_off[s]), int(job.sample_off[s + 1])
        alone = den.fm_loss_terms(den.make_job(st, [s]), x1[a:b], tv, kind="target", sigma=0.1, eps=eps[0][a:b],
                                  want_model_out=True)
        for k in KEYS:
            assert torch.equal(mixed[k][s:s + 1], alone[k]), (k, s)
        for k in ("xt", "ut", "model_out"):
            assert torch.equal(mixed[k][a:b], alone[k]), (k, s)
    # ... and twice the same bits (the second call finds its sub-jobs cached)
    same(mixed, den.fm_loss_terms(job, x1, RAGGED_TIMES, kind="target", sigma=0.1, eps=eps[0], want_model_out=True))


@pytest.mark.parametrize("precision", ["f16x3", "f32"])
@pytest.mark.parametrize("where", ["ragged", "L46_B2"])
def test_fused_sweep_equals_stepping(where, precision):
    """Row k of codlad_fm_loss_loop = codlad_fm_path and codlad_fm_loss_forward at ts[k] with eps[k], bit for bit."""
    if where == "ragged":
        den, _st, job, x0, x1, eps = ragged(precision)
        kind, sigma = "target", 0.1
    else:
        den, job, x0, x1, eps = l46(precision)
        kind, sigma = "vp", 0.1
    ts = [0.25, 0.5, 0.75]
    fused = den.fm_loss_sweep(job, x1, ts, kind=kind, sigma=sigma, x0=x0, eps=eps, streams=1)
    for k, tv in enumerate(ts):
        r = den.fm_loss_terms(job, x1, tv, kind=kind, sigma=sigma, x0=x0, eps=eps[k])
        for key in KEYS:
            assert torch.equal(fused[key][k], r[key]), (key, k)
    assert all(bool(torch.isfinite(fused[key]).all()) for key in KEYS)


def test_two_streams_equal_one_and_a_sample_ignores_its_neighbours():
    den, st, job, x0, x1, eps = ragged()
    ts = [0.25, 0.5, 0.75]
    one = den.fm_loss_sweep(job, x1, ts, kind="icfm", sigma=0.1, x0=x0, eps=eps, streams=1)
    same(one, den.fm_loss_sweep(job, x1, ts, kind="icfm", sigma=0.1, x0=x0, eps=eps, streams=2))
    same(one, den.fm_loss_sweep(job, x1, ts, kind="icfm", sigma=0.1, x0=x0, eps=eps, streams=1))     # two runs: the same bits
    # sigma = 0 runs without noise, and gives what zero noise gives
    same(den.fm_loss_sweep(job, x1, ts, kind="icfm", sigma=0.0, x0=x0, streams=1),
         den.fm_loss_sweep(job, x1, ts, kind="icfm", sigma=0.0, x0=x0, eps=torch.zeros_like(eps), streams=2))
    # the sample of 46 nodes alone, and beside other neighbours (itself, twice)
    a, b = int(job.sample_off[2]), int(job.sample_off[3])
    alone = den.fm_loss_sweep(den.make_job(st, [2]), x1[a:b], ts, kind="icfm", sigma=0.1, x0=x0[a:b], eps=eps[:, a:b], streams=1)
    twice = den.fm_loss_sweep(den.make_job(st, [2, 2]), x1[a:b].repeat(2, 1), ts, kind="icfm", sigma=0.1,
                              x0=x0[a:b].repeat(2, 1), eps=eps[:, a:b].repeat(1, 2, 1), streams=2)
    for k in KEYS:
        assert torch.equal(one[k][:, 2], alone[k][:, 0]) and torch.equal(one[k][:, 2], twice[k][:, 1]), k


# ------------------------------------------------------------------------------------ 9. the status word --
@pytest.mark.parametrize("precision", PRECISIONS)
def test_status_word_raises_from_the_flow_loss_path(precision):
    """The weights of test_precision_envelope.test_fp16_range_overflow_is_an_error_not_a_number (edge features far outside
    the fp16 range): the split-fp16 modes report it through the status word, the fp32 mode computes a finite result."""
    sd = flow_sd()
    sd["features.norm_edges.weight"] = sd["features.norm_edges.weight"] * 1e6
    den, _st, job, x0, x1, eps = ragged(precision, sd)
    ts = [0.25, 0.5, 0.75]
    if precision == "f32":
        r = den.fm_loss_terms(job, x1, RAGGED_TIMES, kind="icfm", sigma=0.1, x0=x0, eps=eps[0])
        s = den.fm_loss_sweep(job, x1, ts, kind="icfm", sigma=0.1, x0=x0, eps=eps, streams=2)
        assert all(bool(torch.isfinite(r[k]).all()) and bool(torch.isfinite(s[k]).all()) for k in KEYS)
        return
    with pytest.raises(RuntimeError, match="not finite"):
        den.fm_loss_terms(job, x1, 0.5, kind="icfm", sigma=0.1, x0=x0, eps=eps[0])
    with pytest.raises(RuntimeError, match="not finite"):
        den.fm_loss_terms(job, x1, RAGGED_TIMES, kind="icfm", sigma=0.1, x0=x0, eps=eps[0])
    for streams in (1, 2):
        with pytest.raises(RuntimeError, match="not finite"):
            den.fm_loss_sweep(job, x1, ts, kind="icfm", sigma=0.1, x0=x0, eps=eps, streams=streams)
    assert int(job.status.item()) == 0


def test_refusals():
    den, _st, job, x0, x1, eps = ragged()
    with pytest.raises(ValueError, match="needs x0"):
        den.fm_loss_terms(job, x1, 0.5, kind="vp", eps=eps[0])
    with pytest.raises(ValueError, match="eps may be None only"):
        den.fm_loss_sweep(job, x1, [0.5], kind="target")
    with pytest.raises(ValueError, match=r"\[0, 1\]"):
        den.fm_loss_sweep(job, x1, [0.5, 1.5], kind="icfm", x0=x0)
    six = Denoiser(synth.denoiser_state_dict(cases.WEIGHT_SEED), DEV)
    with pytest.raises(ValueError, match="flow-matching model"):
        six.fm_loss_terms(job, x1, 0.5, kind="icfm", x0=x0)


# ------------------------------------------------------------------------------------ 10. the CLI --
def test_cli_experiment_fmloss(tmp_path):
    cmd = [sys.executable, os.path.join(ROOT, "test.py"), "--synthetic", "--synthetic_weights", "--experiment", "fmloss",
           "--model", "icfm", "--num_steps", "3", "--exp", "clitest"]
    env = dict(os.environ, PYTHONPATH=ROOT)
    res = subprocess.run(cmd, env=env, cwd=str(tmp_path), capture_output=True, text=True, timeout=900)
    assert res.returncode == 0, res.stdout[-1500:] + res.stderr[-3000:]
    means = re.findall(r"K=3, icfm sigma=0.0: mean l2 (\S+):", res.stdout)
    rows = re.findall(r"^  t=(\S+) l2 (\S+)$", res.stdout, flags=re.M)
    assert len(means) == 4 and len(rows) == 12, res.stdout[-1500:]            # one block per synthetic PED file, K lines each
    assert [t for t, _v in rows[:3]] == ["0.1667", "0.5000", "0.8333"]
    assert all(np.isfinite(float(v)) for v in means) and all(np.isfinite(float(v)) for _t, v in rows)
    found = []
    for root, _dirs, files in os.walk(str(tmp_path)):
        found += [np.load(os.path.join(root, f)) for f in files if f.endswith("_fmloss_l2.npy")]
    assert len(found) == 4
    for a in found:
        assert a.ndim == 2 and a.shape[1] == 3 and np.isfinite(a).all(), a.shape
    bad = subprocess.run(cmd[:-6] + ["--model", "diffusion", "--num_steps", "3"], env=env, cwd=str(tmp_path),
                         capture_output=True, text=True, timeout=600)
    assert bad.returncode != 0 and "--experiment fmloss needs a flow-matching model" in bad.stdout + bad.stderr


# ------------------------------------------------------------------------------------ 11. any callable --
def test_loss_sweep_with_a_plain_callable():
    """A foreign callable is evaluated per time and followed by codlad_fm_terms: the fused path's numbers to the
    end-to-end bound (same model underneath: the head's bits are the forward's, so the allowance is not even used up)."""
    name = "sweep_icfm_L46"
    geometry, kind, sigma, ts = fc.SWEEP_CASES[name]
    _p, batch, mask, x0, x1 = fc.inputs(geometry, 1)
    g = fc.load(name)
    model = model_of()
    kwargs = on_dev(batch, mask)
    eps = torch.from_numpy(g["eps"]).to(DEV)
    fm = MATCHER[kind](sigma)
    fused = fm.loss_sweep(model.forward, x0.to(DEV), x1.to(DEV), ts, step_noise=eps, model_kwargs=kwargs, loss_type="l1")
    calls = []

    def plain(x, t, **kw):
        calls.append(float(t[0]))
        return model(x, t, **kw)

    foreign = fm.loss_sweep(plain, x0.to(DEV), x1.to(DEV), ts, step_noise=eps, model_kwargs=kwargs, loss_type="l1")
    assert calls == [float(np.float32(v)) for v in ts]
    for k in range(len(ts)):
        allow = propagated(g["model_out"][k], g["ut"][k])
        for key in KEYS:
            a, b = fused["terms"][key][:, k].cpu().double().numpy(), foreign["terms"][key][:, k].cpu().double().numpy()
            allowed = kernel_bound(g, key) * np.abs(g["f64_" + key][k]) + np.asarray(allow[key])
            print(f"t = {ts[k]} {key}: fused - foreign {np.abs(a - b).max():.3e} (allowed {allowed.min():.3e})")
            assert (np.abs(a - b) <= allowed).all(), (key, k)
    assert np.allclose(fused["loss"].numpy(), foreign["loss"].numpy(), rtol=1e-4)
    tl = fm.training_losses(plain, x0.to(DEV), x1.to(DEV), t=torch.full((2,), 0.5, device=DEV), eps=eps[1], model_kwargs=kwargs)
    tf = fm.training_losses(model.forward, x0.to(DEV), x1.to(DEV), t=torch.full((2,), 0.5, device=DEV), eps=eps[1],
                            model_kwargs=kwargs)
    assert torch.allclose(tl["per_sample"], tf["per_sample"], rtol=1e-4)
