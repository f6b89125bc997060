"""CPU-only checks of the fused ODE sampler's host side: the stage-time table the fused loop's modulation rows are computed
from equals the times the step-wise `_fixed_step` evaluates the model at, the grid rules, and the C ABI's declarations."""
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
    assert "#define CODLAD_ABI_VERSION 18\n" in header and _lib.ABI_VERSION == 18
    import ctypes as C
    assert C.sizeof(_lib.OdeState) == 96 and _lib.OdeState.hh_f.offset == 64 and _lib.OdeState.tf.offset == 68
    assert C.sizeof(_lib.OdeDopri5Bufs) == 13 * 8
    assert _lib.ODE_NORM_WORDS == int(header.split("#define CODLAD_ODE_NORM_BLOCKS ")[1].split()[0]) + 1


def test_argument_errors_are_reported_not_crashed():
    lib = _lib.lib()
    assert lib.codlad_ode_error_norm(None, None, None, 4, 1e-5, 1e-5, None, None) < 0
    assert b"null pointer" in lib.codlad_last_error()
    assert lib.codlad_ode_loop(None, None, 1, None, None, None, 1, None, None, None, 0, None, 1, None, None, None) < 0
    assert b"null pointer" in lib.codlad_last_error()
    assert lib.codlad_ode_dopri5_attempt(None, None, 1, None, None, None, 1, None, 1.0, 1e-5, 1e-5, None, None) < 0
    assert b"null pointer" in lib.codlad_last_error()
