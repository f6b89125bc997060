"""The fused ODE sampler of the flow-matching models (codlad_ode_loop, codlad_ode_dopri5_attempt, Denoiser.sample_ode,
ode.ModelVelocity) on the GPU.  Fixed grids are held to the step-wise path bit for bit and to trajectories integrated over
the reference model; dopri5 to the oracle's step sequence and result; the error norm to a double sum by torch within the
worst-case bound of such a sum."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from codlad_amd import _lib, synth
from codlad_amd.diffusion_and_flow import ode
from codlad_amd.engine import Denoiser
from codlad_amd.models.latent_model import MPNN_models
from oracle import denoiser as oden
from oracle import flow as oflow
from tests import cases

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INTERVALS = {"L46_B2": 8, "L87_B2": 5}


def rel_err(a, b):
    a = torch.as_tensor(a).detach().cpu().double()
    b = torch.as_tensor(b).detach().cpu().double()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


@pytest.fixture(scope="module")
def fsd():
    return synth.denoiser_state_dict(cases.WEIGHT_SEED, flow=True)


def flow_model(sd, precision="f16x3"):
    model = MPNN_models["mpnn_diffusion"](input_size=3, unconditional=True, diffusion="fm", self_condition=False)
    model.load_state_dict(sd, strict=True)
    model = model.to(DEV).eval()
    model.precision = precision
    return model


def fields(model, name):
    """(x on the device, the fused field, the same field as a plain callable, the CPU pieces) of a FLOW_CASES shape."""
    L, B, seed, _times, _n = cases.FLOW_CASES[name]
    _prot, batch, x, _t, mask = cases.denoiser_inputs(L, B, seed)
    dbatch = {k: (v.to(DEV) if hasattr(v, "to") else v) for k, v in batch.items()}
    fused = ode.ModelVelocity(model, mask=mask.to(DEV), batch=dbatch)
    plain = lambda t, x_in: fused(t, x_in)  # noqa: E731
    return x.to(DEV), fused, plain, (batch, x, mask)


@pytest.fixture(scope="module")
def model(fsd):
    return flow_model(fsd)


@pytest.fixture(scope="module")
def oracle_dopri5(fsd):
    """The oracle's dopri5 on L46_B2, t = [0, 1], rtol = atol = 1e-5: computed once, read by the dopri5 tests."""
    L, B, seed, _times, _n = cases.FLOW_CASES["L46_B2"]
    _prot, batch, x, _t, mask = cases.denoiser_inputs(L, B, seed)
    cg_z, cg_xyz, _m = oden.batch_to_dense(batch)
    yo, n_eval = oflow.odeint_dopri5(oflow.velocity_fn(fsd, cg_xyz, cg_z, mask), x, [0.0, 1.0], 1e-5, 1e-5)
    return yo[-1], n_eval


# ---------------------------------------------------------------------------------- 1. fixed grids --
@pytest.mark.parametrize("precision", ["f16x3", "f32"])
@pytest.mark.parametrize("method", ["euler", "midpoint", "rk4"])
@pytest.mark.parametrize("name", list(INTERVALS))
def test_fixed_grid_fused_equals_stepwise(fsd, name, method, precision):
    mod = flow_model(fsd, precision)
    x, fused, plain, _cpu = fields(mod, name)
    n = INTERVALS[name]
    assert n == cases.FLOW_CASES[name][4]                  # the goldens' grids
    ts = torch.linspace(0, 1, n + 1)
    a, stats = ode.odeint(fused, x, ts, method=method, return_stats=True)
    b, stats_b = ode.odeint(plain, x, ts, method=method, return_stats=True)
    assert a.shape == (n + 1,) + tuple(x.shape)
    assert torch.equal(a, b)
    assert stats == stats_b == {"n_eval": n * {"euler": 1, "midpoint": 2, "rk4": 4}[method], "n_accept": n, "n_reject": 0}
    if method in ("euler", "rk4"):
        gold = np.load(cases.npz_path(f"g12_flow_{name}"))
        err = rel_err(a[-1], gold[method])
        print(f"{name} {method} {precision}: fused vs the reference model's trajectory {err:.3e}")
        assert err < 2e-5


# --------------------------------------------------------------------------- 2. ragged job, streams --
def test_ragged_job_streams_and_units_alone(fsd):
    den = Denoiser(fsd, DEV, precision="f16x3")
    p46 = cases.denoiser_inputs(46, 2, 12)[0]
    p87 = cases.denoiser_inputs(87, 2, 13)[0]
    xyz = [torch.from_numpy(p["xyz_full"])[0, 1:-1] for p in (p46, p87)]
    z = [torch.from_numpy(p["z_full"])[1:-1] for p in (p46, p87)]
    st = den.prepare_structures(xyz, z)
    members = [0, 1, 1]                                     # lengths 46, 87, 87: the second structure twice
    job = den.make_job(st, members)
    y0 = synth.gaussian((job.n_nodes, 3), 6100).to(DEV)
    ts = [0.0, 0.3, 0.65, 1.0]
    one, stats = den.sample_ode(job, y0, ts, method="rk4", streams=1)
    two, _ = den.sample_ode(job, y0, ts, method="rk4", streams=2)
    assert one.shape == (4, 220, 3) and bool(torch.isfinite(one).all()) and stats["n_eval"] == 12
    assert torch.equal(one, two)
    assert not torch.equal(one[:, 46:133], one[:, 133:])   # the repeated structure from different y0
    for s, m in enumerate(members):
        a, b = int(job.sample_off[s]), int(job.sample_off[s + 1])
        alone, _ = den.sample_ode(den.make_job(st, [m]), y0[a:b], ts, method="rk4")
        assert torch.equal(alone, one[:, a:b]), s


# ----------------------------------------------------------------------------------- 3. reverse grid --
def test_reverse_grid(fsd, model):
    x, fused, plain, (batch, x_cpu, mask) = fields(model, "L46_B2")
    ts = torch.linspace(1, 0, 9)
    a = ode.odeint(fused, x, ts, method="rk4")
    b = ode.odeint(plain, x, ts, method="rk4")
    assert torch.equal(a, b)
    cg_z, cg_xyz, _m = oden.batch_to_dense(batch)
    ref = oflow.odeint_fixed(oflow.velocity_fn(fsd, cg_xyz, cg_z, mask), x_cpu, ts.tolist(), "rk4")
    err = rel_err(a[-1], ref[-1])
    print(f"rk4 on linspace(1, 0, 9): fused vs oracle {err:.3e}")
    assert err < 2e-5
    for f in (fused, plain):
        with pytest.raises(ValueError, match="increasing"):
            ode.odeint(f, x, ts, rtol=1e-5, atol=1e-5, method="dopri5")


# ---------------------------------------------------------------------------------------- 4. dopri5 --
def test_dopri5_fused(model, oracle_dopri5):
    x, fused, plain, _cpu = fields(model, "L46_B2")
    yo, n_eval = oracle_dopri5
    a, stats = ode.odeint(fused, x, torch.tensor([0.0, 1.0]), rtol=1e-5, atol=1e-5, method="dopri5", return_stats=True)
    print(f"dopri5 fused: {stats}, oracle n_eval {n_eval}")
    assert stats["n_eval"] == n_eval                        # the same step sequence
    assert stats["n_eval"] == 2 + 6 * (stats["n_accept"] + stats["n_reject"])
    e_oracle = rel_err(a[-1], yo)
    fine = ode.odeint(fused, x, torch.linspace(0, 1, 65), method="rk4")[-1]
    e_fine = rel_err(a[-1], fine)
    b, stats_b = ode.odeint(plain, x, torch.tensor([0.0, 1.0]), rtol=1e-5, atol=1e-5, method="dopri5", return_stats=True)
    print(f"dopri5 fused vs oracle {e_oracle:.3e}, vs 64-interval rk4 {e_fine:.3e}, "
          f"fused - step-wise max |diff| {float((a[-1] - b[-1]).abs().max()):.3e} (rel {rel_err(a[-1], b[-1]):.3e})")
    assert e_oracle < 5e-5
    assert e_fine < 1e-3
    again = ode.odeint(fused, x, torch.tensor([0.0, 1.0]), rtol=1e-5, atol=1e-5, method="dopri5")
    assert torch.equal(a, again)                            # no floating-point atomics: two runs, the same bits


def test_dopri5_interior_output_time(model):
    x, fused, plain, _cpu = fields(model, "L46_B2")
    ts = torch.tensor([0.0, 0.4, 1.0])
    a, sa = ode.odeint(fused, x, ts, rtol=1e-5, atol=1e-5, method="dopri5", return_stats=True)
    b, sb = ode.odeint(plain, x, ts, rtol=1e-5, atol=1e-5, method="dopri5", return_stats=True)
    assert a.shape == b.shape == (3,) + tuple(x.shape) and torch.equal(a[0], x)
    print(f"dopri5 [0, 0.4, 1]: fused {sa}, step-wise {sb}; traj[1] {rel_err(a[1], b[1]):.3e}, traj[2] {rel_err(a[2], b[2]):.3e}")
    assert rel_err(a[1], b[1]) < 5e-5
    assert rel_err(a[2], b[2]) < 5e-5


# ------------------------------------------------------------------------------ 5. error norm kernel --
def error_norm(err, y, y1, rtol, atol):
    out = torch.zeros(_lib.ODE_NORM_WORDS, dtype=torch.float64, device=DEV)
    rc = _lib.lib().codlad_ode_error_norm(_lib.ptr(err), _lib.ptr(y), _lib.ptr(y1), err.numel(), C.c_float(rtol),
                                          C.c_float(atol), _lib.ptr(out), _lib.stream_ptr(torch.device(DEV)))
    _lib.check(rc, "codlad_ode_error_norm")
    return out[0].cpu()


@pytest.mark.parametrize("n", [1, 255, 256, 257, 276, 100003])
def test_error_norm_kernel(n):
    rtol, atol = 1e-5, 1e-5
    err = (synth.gaussian((n,), 9100 + n % 1000) * 1e-5).to(DEV)
    y = synth.gaussian((n,), 9200 + n % 1000).to(DEV)
    y1 = synth.gaussian((n,), 9300 + n % 1000).to(DEV)
    got = error_norm(err, y, y1, rtol, atol)
    q = err / (atol + rtol * torch.maximum(y.abs(), y1.abs()))             # fp32, as ode._dopri5 forms it
    want = q.double().pow(2).mean().sqrt().cpu()
    rel = abs(float(got) - float(want)) / float(want)
    print(f"n = {n}: kernel {float(got)!r}, torch {float(want)!r}, relative difference {rel:.3e} (bound {n * 2.0 ** -52:.3e})")
    assert float(want) > 0 and rel <= n * 2.0 ** -52
    assert got.view(torch.int64).item() == error_norm(err, y, y1, rtol, atol).view(torch.int64).item()
    bad = err.clone()
    bad[n // 2] = float("inf")
    assert not np.isfinite(float(error_norm(bad, y, y1, rtol, atol)))


# -------------------------------------------------------------------------------- 6. non-finite stop --
def test_dopri5_stops_on_a_non_finite_output():
    """Edge features of magnitude ~1e6 overflow the fp16 range of the split modes (the sentinel case of
    tests/test_precision_envelope.py): the adaptive loop must stop at once, not run its controller to max_steps."""
    sd = synth.denoiser_state_dict(cases.WEIGHT_SEED, flow=True)
    sd["features.norm_edges.weight"] = sd["features.norm_edges.weight"] * 1e6
    mod = flow_model(sd)
    x, fused, _plain, _cpu = fields(mod, "L46_B2")
    with pytest.raises(RuntimeError, match=r"dopri5: .*not finite.* t = 0\.0"):
        ode.odeint(fused, x, torch.tensor([0.0, 1.0]), rtol=1e-5, atol=1e-5, method="dopri5")
    eng, job = fused.fused_job(x)
    assert int(job.status.item()) == 0                      # cleared: the job is usable again
    # unchecked, with a given first step: the NaNs reach the device controller, which flags the first attempt
    with pytest.raises(RuntimeError, match=r"dopri5: .*not finite.*attempt (\d+)") as info:
        eng.sample_ode(job, x.reshape(-1, 3), [0.0, 1.0], method="dopri5", rtol=1e-5, atol=1e-5, check=False,
                       first_step=0.05)
    assert int(re.search(r"attempt (\d+)", str(info.value)).group(1)) < 10
    assert int(job.status.item()) == 0
    # the step-wise controller stops the same way on a callable that turns infinite after the initial step's two calls
    calls = []

    def blows_up(t, y):
        calls.append(float(t))
        return y * 0.1 if len(calls) <= 2 else torch.full_like(y, float("inf"))

    with pytest.raises(RuntimeError, match=r"dopri5: .*not finite.*attempt 1\b"):
        ode.odeint(blows_up, x, torch.tensor([0.0, 1.0]), rtol=1e-5, atol=1e-5, method="dopri5")
    assert len(calls) == 8


# ---------------------------------------------------------------------------------------------- 7. CLI --
def _cli(extra, cwd):
    cmd = [sys.executable, os.path.join(ROOT, "test.py"), "--synthetic", "--synthetic_weights", "--synthetic_frames", "1",
           "--data_type", "PED", "--vae_type", "N6", "--exp", "clitest", "--model", "fm", "--method", "euler", "--steps", "5",
           "--compute_nfe"] + extra
    os.makedirs(cwd, exist_ok=True)
    res = subprocess.run(cmd, env=dict(os.environ, PYTHONPATH=ROOT), cwd=str(cwd), capture_output=True, text=True,
                         timeout=600)
    assert res.returncode == 0, res.stdout[-1500:] + res.stderr[-3000:]
    files = [os.path.join(dp, f) for dp, _d, fs in os.walk(str(cwd)) for f in fs if f.endswith("_xyz_recon.npy")]
    return res.stdout, {os.path.basename(f): np.load(f) for f in files}


def test_cli_compute_nfe_and_fused_equals_stepwise(tmp_path):
    out, fused = _cli([], tmp_path / "fused")
    nfe = re.findall(r"NFE: (\d+) model evaluations", out)
    assert len(nfe) == 4 and set(nfe) == {"4"}              # four synthetic proteins, linspace(0, 1, 5): 4 euler steps
    out_s, stepwise = _cli(["--ode_stepwise"], tmp_path / "stepwise")
    assert re.findall(r"NFE: (\d+) model evaluations", out_s) == nfe
    assert sorted(fused) == sorted(stepwise) and len(fused) == 4
    for k in fused:
        assert np.isfinite(fused[k]).all() and np.array_equal(fused[k], stepwise[k]), k
