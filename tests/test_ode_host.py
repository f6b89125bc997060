"""CPU-only checks of the fused ODE sampler's host side: the stage-time table the fused loop's modulation rows are computed
from equals the times the step-wise `_fixed_step` evaluates the model at, the grid rules, and the C ABI's declarations."""
import ctypes as C
import os

import pytest
import torch

from codlad_amd import _lib
from codlad_amd.diffusion_and_flow import ode

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRIDS = {"increasing": torch.linspace(0, 1, 9).tolist(), "decreasing": torch.linspace(1, 0, 6).tolist(),
         "uneven": [0.0, 0.1, 0.37, 0.4, 1.0], "two": [0.25, 0.75]}


@pytest.mark.parametrize("grid", list(GRIDS))
@pytest.mark.parametrize("method", ["euler", "midpoint", "rk4"])
def test_stage_times_are_the_times_fixed_step_evaluates_at(monkeypatch, method, grid):
    ts = GRIDS[grid]
    seen = []

    def recording(t, y):
        assert t.dtype == torch.float32
        seen.append(float(t))
        return y

    monkeypatch.setattr(ode, "combine", lambda y, ks, coefs, h: y)      # the device update: not what is looked at here
    y = torch.zeros(2, 3)
    for t0, t1 in zip(ts, ts[1:]):
        ode._fixed_step(recording, method, t0, t1 - t0, t1, y)
    table = ode.stage_times(method, ts)
    assert table == seen
    assert len(table) == (len(ts) - 1) * {"euler": 1, "midpoint": 2, "rk4": 4}[method]
    assert all(v == float(torch.tensor(v, dtype=torch.float32)) for v in table)      # float32 values, as mods_kernel reads them


def test_grid_rules():
    for method in ("euler", "midpoint", "rk4"):
        ode.check_grid([0.0, 0.5, 1.0], method)
        ode.check_grid([1.0, 0.5, 0.0], method)
    ode.check_grid([0.0, 1.0], "dopri5")
    with pytest.raises(ValueError, match="increasing"):
        ode.check_grid([1.0, 0.0], "dopri5")
    for bad in ([0.0], [0.0, 0.0], [0.0, 1.0, 0.5]):
        with pytest.raises(ValueError, match="monotonic"):
            ode.check_grid(bad, "rk4")
    with pytest.raises(NotImplementedError):
        ode.check_grid([0.0, 1.0], "heun3")


def test_model_velocity_is_an_ordinary_callable():
    class Model:
        def forward(self, x, t, y, mask=None, batch=None):
            return (x, t, y, mask, batch)

    f = ode.ModelVelocity(Model(), mask="m", batch="b")
    assert f(0.5, "x") == ("x", 0.5, None, "m", "b")
    assert f.fused_job(torch.zeros(1, 2, 3)) is None       # not the HIP model: odeint steps through it


def test_new_entry_points_are_declared():
    names = _lib.exported_symbols()
    for name in ("codlad_ode_loop", "codlad_ode_dopri5_attempt", "codlad_ode_error_norm"):
        assert name in names
        assert hasattr(_lib.lib(), name)
    header = open(os.path.join(ROOT, "include", "codlad_hip.h")).read()
    assert "#define CODLAD_ABI_VERSION 19\n" in header and _lib.ABI_VERSION == 19
    assert C.sizeof(_lib.OdeState) == 96 and _lib.OdeState.hh_f.offset == 64 and _lib.OdeState.tf.offset == 68
    assert C.sizeof(_lib.OdeDopri5Bufs) == 13 * 8
    assert _lib.ODE_NORM_WORDS == int(header.split("#define CODLAD_ODE_NORM_BLOCKS ")[1].split()[0]) + 1


def test_argument_errors_are_reported_not_crashed():
    lib = _lib.lib()
    assert lib.codlad_ode_error_norm(None, None, None, 4, 1e-5, 1e-5, None, None) < 0
    assert b"null pointer" in lib.codlad_last_error()
    job = C.byref(_lib.JobDesc(None, 1, None, None, None, 1, None))
    assert lib.codlad_ode_loop(None, job, None, None, None, 0, None, 1, None, None) < 0
    assert b"null pointer" in lib.codlad_last_error()
    assert lib.codlad_ode_dopri5_attempt(None, job, None, 1.0, 1e-5, 1e-5, None) < 0
    assert b"null pointer" in lib.codlad_last_error()


# every entry point that runs the denoiser: the out_dim it wants, and its own arguments between the job and the stream
# (p = a dummy host pointer: no call below gets as far as reading one)
JOB_ENTRY_POINTS = {
    "codlad_denoiser_forward": (6, lambda p, bufs, terms: (p, None, p, p)),
    "codlad_sample_loop": (6, lambda p, bufs, terms: (p, None, p, p, p, 10)),
    "codlad_sample_loop_pinned": (6, lambda p, bufs, terms: (p, None, p, p, p, 10, p, p)),
    "codlad_ddim_loop": (6, lambda p, bufs, terms: (p, None, p, p, p, 10, 0, 0, None, None)),
    "codlad_loss_forward": (6, lambda p, bufs, terms: (p, p, p, None, p, p, 10, 3, p, 2, None, C.byref(terms))),
    "codlad_bpd_loop": (6, lambda p, bufs, terms: (p, p, p, p, p, 10, p, 2, p, p, p, p, p)),
    "codlad_ode_loop": (3, lambda p, bufs, terms: (p, p, p, 0, p, 1, p)),
    "codlad_ode_dopri5_attempt": (3, lambda p, bufs, terms: (C.byref(bufs), 1.0, 1e-5, 1e-5)),
}


@pytest.mark.parametrize("name", list(JOB_ENTRY_POINTS))
def test_a_defective_job_is_refused_under_the_callers_name(name):
    lib = _lib.lib()
    one = torch.zeros(12)
    p = _lib.ptr(one)
    out_dim, own = JOB_ENTRY_POINTS[name]
    w = _lib.DenoiserWeights()
    w.out_dim = out_dim
    ws = _lib.Workspace()
    ws.hV = ws.hVenc = ws.S = ws.PQ = ws.hE = p
    bufs, terms = _lib.OdeDopri5Bufs(), _lib.LossTerms()
    bufs.y = bufs.y1 = bufs.xin = bufs.mods = bufs.state = bufs.norm = p
    for j in range(7):
        bufs.k[j] = one.data_ptr()
    good = dict(node_info=p, n_nodes=4, E_idx=p, h_E0=p, E1=None, n_snodes=1, ws=C.pointer(ws))
    jobs = [None] + [C.byref(_lib.JobDesc(**dict(good, **bad))) for bad in (dict(ws=None), dict(node_info=None), dict(n_nodes=0))]
    for job in jobs:
        assert getattr(lib, name)(C.byref(w), job, *own(p, bufs, terms), None) == -1
        assert lib.codlad_last_error().startswith(name.encode() + b": ")
