"""CPU checks of the flow-matching loss evaluation: the restatement (tests/flow_loss_ref.py) against the g20 goldens (the
reference's own matchers and loss_fn), the new entry points' declarations and argument checks, and the refusals of the
public interface.  No GPU compute here."""
import ctypes as C
import os
import re
import types

import numpy as np
import pytest
import torch

from codlad_amd import _lib
from codlad_amd.diffusion_and_flow import flow
from tests import flow_loss_cases as fc
from tests import flow_loss_ref as fr
from tests.cli_script import load_cli

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("codlad_fm_path", "codlad_fm_terms", "codlad_fm_loss_forward", "codlad_fm_loss_loop")


def case_arrays(name):
    geometry, kind, sigma, n_rep, case_t = fc.FM_CASES[name]
    _p, _batch, _mask, x0, x1 = fc.inputs(geometry, n_rep)
    return kind, sigma, x0, x1, fc.times(case_t, x1.shape[0]), fc.load(name)


# ------------------------------------------------------------------------------------ 1. restatement --
@pytest.mark.parametrize("name", list(fc.FM_CASES))
def test_restated_paths_against_the_reference(name):
    kind, sigma, x0, x1, t, g = case_arrays(name)
    eps = torch.from_numpy(g["eps"])
    xt, ut = fr.path(kind, sigma, x0, x1, t, eps)
    if kind != "vp":
        assert np.array_equal(xt.numpy(), g["xt"]) and np.array_equal(ut.numpy(), g["ut"])
    xt64, ut64 = fr.path(kind, sigma, x0, x1, t, eps, dtype=torch.float64)
    np.testing.assert_allclose(xt64.numpy(), g["f64_xt"], rtol=1e-13, atol=1e-15)
    np.testing.assert_allclose(ut64.numpy(), g["f64_ut"], rtol=1e-13, atol=1e-15)
    # fp32 against float64 stays inside the reference's own deviation (VP: the bound the device is held to, too)
    dev = [float(np.abs(a.double().numpy() - g[k]).max() / np.abs(g[k]).max()) for a, k in ((xt, "f64_xt"), (ut, "f64_ut"))]
    assert max(dev) <= fc.REF_DEV_FACTOR * max(g["ref_dev"][5:])


@pytest.mark.parametrize("name", list(fc.FM_CASES))
def test_restated_losses_against_the_reference(name):
    g = fc.load(name)
    vt, ut = torch.from_numpy(g["model_out"]), torch.from_numpy(g["ut"])
    t64 = fr.terms64(vt, ut)
    t32 = fr.terms32(vt, ut)
    lens = [vt.shape[1]] * vt.shape[0]
    for k in fc.LOSS_TYPES:
        np.testing.assert_allclose(t64[k].numpy(), g[f"f64_{k}"], rtol=1e-12)
        # the kernel's summation order in fp32: inside the bound the device is held to
        rel = float(((t32[k].double() - t64[k]).abs() / t64[k].abs()).max())
        assert rel <= fc.REF_DEV_FACTOR * g["ref_dev"][fc.REF_DEV_INDEX[k]], (k, rel)
        # the batch scalar from per-sample means and lengths = loss_fn on the batch: float64 rounding on the float64
        # terms; on the fp32 terms the per-sample bound (the scalar is a positive combination of them)
        want = float(g[f"f64_batch_{k}"])
        assert abs(fr.batch_scalar(t64[k], lens) - want) <= 1e-12 * abs(want)
        got = float(flow.batch_loss(torch.from_numpy(g[f"f32_{k}"]), lens))
        assert abs(got - want) <= fc.REF_DEV_FACTOR * g["ref_dev"][fc.REF_DEV_INDEX[k]] * abs(want), (k, got, want)
    assert torch.equal(t64["huber"], t64["smooth_l1"])


def test_terms64_is_differentiable_in_model_out():
    g = fc.load("icfm_s0_L46")
    vt = torch.from_numpy(g["model_out"]).double().requires_grad_(True)
    with torch.enable_grad():
        fr.terms64(vt, torch.from_numpy(g["ut"]))["log_cosh"].sum().backward()
    assert vt.grad is not None and bool(torch.isfinite(vt.grad).all()) and float(vt.grad.abs().max()) > 0


def test_goldens_hold_outputs_and_noise_only():
    for name in list(fc.FM_CASES) + list(fc.SWEEP_CASES):
        g = fc.load(name)
        assert not {"x0", "x1", "t"} & set(g.files)
        assert g["ref_dev"].shape == (7,) and np.array_equal(g["ref_dev"], fc.load("vp_s0_L46")["ref_dev"])
        assert os.path.getsize(fc.cases.npz_path(f"g20_flow_loss_{name}")) < 64 * 1024
    assert fc.load("sweep_icfm_L46")["xt"].shape == (3, 2, 46, 3)


# ------------------------------------------------------------------------------------ 2. the C ABI --
def test_new_entry_points_are_declared_exported_and_validate():
    header = open(os.path.join(ROOT, "include", "codlad_hip.h")).read()
    lib = _lib.lib()
    for name in NEW:
        assert re.search(r"\bint %s\s*\(" % name, header), name
        assert name in _lib.exported_symbols() and hasattr(lib, name)
    assert "#define CODLAD_ABI_VERSION 19\n" in header and lib.codlad_abi_version() == 19 and _lib.ABI_VERSION == 19
    for kind, value in _lib.FM_KINDS.items():
        assert f"#define CODLAD_FM_{kind.upper()} {value}\n" in header
    assert C.sizeof(_lib.FmLossOut) == 5 * 8

    one = torch.zeros(12)
    p = _lib.ptr(one)
    err = lambda: lib.codlad_last_error()                              # noqa: E731

    def path(x0=p, x1=p, eps=p, off=p, n=1, t_dev=None, t=0.5, kind=0, sigma=0.0, xt=p, ut=p):
        return lib.codlad_fm_path(x0, x1, eps, off, n, t_dev, t, kind, sigma, xt, ut, None)

    assert path(kind=7) == -1 and b"codlad_fm_path: unknown matcher kind" in err()
    assert path(kind=-1) == -1 and b"unknown matcher kind" in err()
    assert path(sigma=-0.1) == -1 and b"sigma must not be negative" in err()
    assert path(sigma=float("nan")) == -1 and b"sigma" in err()
    assert path(t=1.5) == -1 and b"t outside [0, 1]" in err()
    assert path(t=-0.01) == -1 and b"t outside [0, 1]" in err()
    assert path(x1=None) == -1 and b"null pointer" in err()
    assert path(x0=None, kind=0) == -1 and b"x0" in err()
    assert path(x0=None, kind=2) == -1 and b"x0" in err()
    assert path(eps=None, kind=0, sigma=0.1) == -1 and b"eps" in err()
    assert path(eps=None, kind=2, sigma=0.1) == -1 and b"eps" in err()
    assert path(eps=None, kind=1) == -1 and b"eps" in err()
    assert path(off=None) == -1 and path(xt=None) == -1 and path(ut=None) == -1 and path(n=0) == -1

    out = _lib.FmLossOut()
    assert lib.codlad_fm_terms(None, p, p, 1, C.byref(out), None) == -1 and b"codlad_fm_terms: null pointer" in err()
    assert lib.codlad_fm_terms(p, None, p, 1, C.byref(out), None) == -1
    assert lib.codlad_fm_terms(p, p, None, 1, C.byref(out), None) == -1
    assert lib.codlad_fm_terms(p, p, p, 1, None, None) == -1
    assert lib.codlad_fm_terms(p, p, p, 0, C.byref(out), None) == -1 and b"n_samples" in err()

    ws = _lib.Workspace()
    ws.hV = ws.hVenc = ws.S = ws.PQ = ws.hE = p
    job = C.byref(_lib.JobDesc(node_info=p, n_nodes=4, E_idx=p, h_E0=p, E1=None, n_snodes=1, ws=C.pointer(ws)))
    w = _lib.DenoiserWeights()

    def forward(out_dim=3, job=job, xt=p, ut=p, mods=p, off=p, n=1, terms=C.byref(out)):
        w.out_dim = out_dim
        return lib.codlad_fm_loss_forward(C.byref(w), job, xt, ut, mods, off, n, None, terms, None)

    assert forward(out_dim=6) == -1 and b"codlad_fm_loss_forward: the flow-matching losses need" in err()
    assert forward(job=None) == -1 and b"codlad_fm_loss_forward: null pointer" in err()
    assert forward(xt=None) == -1 and forward(ut=None) == -1 and forward(mods=None) == -1 and forward(off=None) == -1
    assert forward(terms=None) == -1 and forward(n=0) == -1

    times = (C.c_float * 3)(0.25, 0.5, 0.75)

    def loop(out_dim=3, x0=p, x1=p, eps=p, kind=0, sigma=0.0, ts=times, K=3, mods=p, off=p, n=1, xt=p, ut=p,
             tables=C.byref(out)):
        w.out_dim = out_dim
        return lib.codlad_fm_loss_loop(C.byref(w), job, x0, x1, eps, kind, sigma, ts, K, mods, off, n, xt, ut, tables, None)

    assert loop(out_dim=6) == -1 and b"codlad_fm_loss_loop: the flow-matching losses need" in err()
    assert loop(kind=5) == -1 and b"unknown matcher kind" in err()
    assert loop(kind=_lib.FM_TARGET_FLOW) == -1 and b"unknown matcher kind" in err()
    assert loop(sigma=-1.0) == -1 and b"sigma" in err()
    assert loop(ts=(C.c_float * 3)(0.25, 1.25, 0.75)) == -1 and b"t outside [0, 1]" in err()
    assert loop(ts=(C.c_float * 3)(0.25, 0.5, float("nan"))) == -1 and b"t outside [0, 1]" in err()
    assert loop(x0=None) == -1 and b"x0" in err()
    assert loop(eps=None, sigma=0.1) == -1 and b"eps" in err()
    assert loop(eps=None, kind=1) == -1 and b"eps" in err()
    assert loop(x1=None) == -1 and loop(ts=None) == -1 and loop(mods=None) == -1 and loop(off=None) == -1
    assert loop(xt=None) == -1 and loop(ut=None) == -1 and loop(tables=None) == -1 and loop(K=0) == -1 and loop(n=0) == -1


# ------------------------------------------------------------------------------------ 3. the Python interface --
def test_unbuilt_matchers_refuse_with_the_reason():
    with pytest.raises(NotImplementedError, match="POT"):
        flow.ExactOptimalTransportConditionalFlowMatcher(sigma=0.0)
    with pytest.raises(NotImplementedError, match="score head"):
        flow.SchrodingerBridgeConditionalFlowMatcher(sigma=1.0)
    with pytest.raises(NotImplementedError):
        flow.create_flow_matcher("otcfm")
    with pytest.raises(NotImplementedError):
        flow.create_flow_matcher("sbcfm")
    assert isinstance(flow.create_flow_matcher("fm"), flow.TargetConditionalFlowMatcher)
    assert type(flow.create_flow_matcher("icfm", 0.1)) is flow.ConditionalFlowMatcher
    assert isinstance(flow.create_flow_matcher("vpfm"), flow.VariancePreservingConditionalFlowMatcher)
    with pytest.raises(ValueError):
        flow.ConditionalFlowMatcher(sigma=-0.5)


@pytest.mark.parametrize("cls", [flow.ConditionalFlowMatcher, flow.TargetConditionalFlowMatcher,
                                 flow.VariancePreservingConditionalFlowMatcher])
def test_cpu_tensors_raise(cls):
    fm = cls(sigma=0.1)
    x0, x1, eps = torch.zeros(2, 5, 3), torch.ones(2, 5, 3), torch.zeros(2, 5, 3)
    t = torch.tensor([0.25, 0.5])
    with pytest.raises(RuntimeError, match="MI355X only"):
        fm.sample_location_and_conditional_flow(x0, x1, t=t)
    with pytest.raises(RuntimeError, match="MI355X only"):
        fm.sample_xt(x0, x1, t, eps)
    with pytest.raises(RuntimeError, match="MI355X only"):
        fm.compute_mu_t(x0, x1, t)
    with pytest.raises(RuntimeError, match="MI355X only"):
        fm.compute_conditional_flow(x0, x1, t, x1)
    with pytest.raises(RuntimeError, match="MI355X only"):
        fm.training_losses(lambda *a, **k: None, x0, x1, t=t, eps=eps)
    with pytest.raises(RuntimeError, match="MI355X only"):
        fm.loss_sweep(lambda *a, **k: None, x0, x1, [0.5], step_noise=eps[None])
    with pytest.raises(RuntimeError, match="MI355X only"):
        flow.loss_fn(x0, x1)
    with pytest.raises(ValueError, match="loss_type"):
        fm.training_losses(lambda *a, **k: None, x0, x1, t=t, eps=eps, loss_type="l3")


def test_engine_argument_checks():
    from codlad_amd.engine import Denoiser
    with pytest.raises(ValueError, match="kind"):
        Denoiser._fm_kind("otcfm", 0.0)
    with pytest.raises(ValueError, match="sigma"):
        Denoiser._fm_kind("icfm", -1.0)
    with pytest.raises(TypeError):
        Denoiser._fm_kind("icfm", "0.1")
    with pytest.raises(ValueError, match=r"\[0, 1\]"):
        Denoiser._fm_times([0.5, 1.5], 2, "cpu")
    with pytest.raises(ValueError, match="one per sample"):
        Denoiser._fm_times([0.5, 0.6, 0.7], 2, "cpu")
    ts, shared, dev = Denoiser._fm_times(0.37, 3, "cpu")
    assert shared == float(np.float32(0.37)) and dev is None and ts == [shared] * 3
    from codlad_amd.utils.train_module import loss_fn
    assert loss_fn is flow.loss_fn


def test_fmloss_needs_a_flow_matching_model():
    cli = load_cli("codlad_test_cli")
    base = dict(experiment="fmloss", model="icfm", vae_type="N6", synthetic=True, data_process=False, num_steps=3,
                fm_sigma=0.0)
    cli.check_fmloss(types.SimpleNamespace(**base), 1)
    assert cli.fmloss_steps(types.SimpleNamespace(**base)) == 3
    for change, world, msg in ((dict(model="diffusion"), 1, "needs a flow-matching model"),
                               (dict(model="otcfm"), 1, "POT"),
                               (dict(), 2, "one rank"),
                               (dict(vae_type="C2"), 1, "VQ-VAE"),
                               (dict(synthetic=False), 1, "input with atoms"),
                               (dict(num_steps=0), 1, "--num_steps >= 1")):
        with pytest.raises(SystemExit, match=msg):
            cli.check_fmloss(types.SimpleNamespace(**dict(base, **change)), world)
    cli.check_fmloss(types.SimpleNamespace(experiment="latent", model="diffusion"), 1)      # other experiments pass
    with pytest.raises(SystemExit, match="has no variational bound"):                        # check_bpd is as it was
        cli.check_bpd(types.SimpleNamespace(experiment="bpd", model="icfm"), 1)
