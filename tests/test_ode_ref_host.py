"""CPU: what makes tests/ode_ref.py trustworthy, and what pins codlad_amd/diffusion_and_flow/ode.py to it.

1. The rational tableaus satisfy the order conditions of their methods, rooted tree by rooted tree, in exact arithmetic
   (and the embedded b_hat fails order 5: the error estimate is not vacuous).
2. ode.py's constants - the Dormand-Prince tables, the coefficients `_fixed_step` hands to `combine` and the stage times -
   are the reference's doubles, exactly.
3. The float64 methods converge to closed-form solutions at their orders.
4. oracle/flow.odeint_dopri5 and ode._dopri5 (over a CPU stand-in for the device's `combine`) take dopri5_64's sequence of
   accepted and rejected steps on both analytic fields and end where it ends.  Condition on the inputs, asserted: every
   float64 error ratio stays outside [1 - m, 1 + m], m = 10 x the largest relative difference between the fp32 and the
   float64 run's ratios.  At rtol = atol = 1e-5 and a state of order 1 the fp32 ratio of a smooth step is rounding noise
   (20 - 40 % between fp32 and float64, measured), so the first field runs at 1e-3 and the homogeneous front field at 1e-5
   from a state of order 3e-3, where the absolute tolerance dominates.
5. The controller restatement on a hand-made table, its powers taken by the decimal module rather than libm.
"""
import decimal
import math
from fractions import Fraction as Fr

import numpy as np
import pytest
import torch

from codlad_amd.diffusion_and_flow import ode
from oracle import flow as oflow
from tests import ode_ref as R


rel_err = R.rel_err


# ------------------------------------------------------------------------------------ 1. order conditions --
def test_rooted_trees_are_counted_right():
    trees = R.rooted_trees(5)
    assert [sum(R.tree_order(t) == o for t in trees) for o in range(1, 6)] == [1, 1, 2, 4, 9]
    assert len(set(trees)) == 17
    # the densities of the order-4 trees, by hand: the bush 4, [tau, [tau]] 8, [[tau, tau]] 12, the tall tree 24
    assert sorted(R.tree_gamma(t) for t in trees if R.tree_order(t) == 4) == [4, 8, 12, 24]


@pytest.mark.parametrize("method", list(R.TABLEAUS))
def test_tableau_shape_and_row_sums(method):
    c, A, b = R.TABLEAUS[method]
    assert len(c) == len(A) == len(b)
    for i, row in enumerate(A):
        assert len(row) == i and sum(row, Fr(0)) == c[i], (method, i)


@pytest.mark.parametrize("method", list(R.TABLEAUS))
def test_order_conditions_hold_exactly(method):
    _c, A, b = R.TABLEAUS[method]
    p = R.ORDER[method]
    defects = R.order_defects(A, b, p)
    assert len(defects) == [1, 2, 4, 8, 17][p - 1]
    assert all(v == 0 for v in defects.values()), {t: v for t, v in defects.items() if v}
    beyond = R.order_defects(A, b, p + 1)
    assert any(v != 0 for v in beyond.values())            # and no higher: the table is that method's, not a better one's


def test_dormand_prince_embedded_pair():
    c, A, b = R.TABLEAUS["dopri5"]
    assert A[6] == b[:6] and b[6] == 0 and c[6] == 1       # FSAL: the last stage's input is the step's result
    assert sum(R.DP_B_HAT, Fr(0)) == 1
    four = R.order_defects(A, R.DP_B_HAT, 4)
    assert len(four) == 8 and all(v == 0 for v in four.values())
    five = R.order_defects(A, R.DP_B_HAT, 5)
    assert any(v != 0 for t, v in five.items() if R.tree_order(t) == 5)    # else b - b_hat would estimate nothing
    # the weights torchdiffeq lists are two thirds of Dormand and Prince's own b - b_hat (b_hat_1 = 5179/57600, ...): the same
    # estimator up to a constant, typed from a second source
    classical = [Fr(71, 57600), 0, Fr(-71, 16695), Fr(71, 1920), Fr(-17253, 339200), Fr(22, 525), Fr(-1, 40)]
    assert [p - q for p, q in zip(b, R.DP_B_HAT)] == [Fr(2, 3) * v for v in classical]


def test_classical_rk4_is_fourth_order():
    _c, A, b = R.CLASSICAL_RK4
    assert all(v == 0 for v in R.order_defects(A, b, 4).values())


# ------------------------------------------------------------------------------------- 2. ode.py's tables --
def test_dormand_prince_constants_of_ode_py():
    dp = R.dp_device()
    assert tuple(ode._DP_ALPHA) == dp["alpha"]
    assert tuple(tuple(row) for row in ode._DP_BETA) == dp["beta"]
    assert tuple(ode._DP_C_SOL) == dp["c_sol"]
    assert tuple(ode._DP_C_ERR) == dp["c_err"]              # the difference of the two rounded doubles, bit for bit
    exact = [p - q for p, q in zip(R.TABLEAUS["dopri5"][2], R.DP_B_HAT)]
    for got, want in zip(dp["c_err"], exact):               # and that difference is the rational's to a few ulps of b_j
        assert abs(Fr(got) - want) <= Fr(1, 2 ** 52), (got, want)


GRIDS = {"unit": (0.0, 1.0), "uneven": (0.3, 0.65), "reverse": (0.75, 0.5), "awkward": (0.1, 0.4)}


@pytest.mark.parametrize("grid", list(GRIDS))
@pytest.mark.parametrize("method", ["euler", "midpoint", "rk4"])
def test_fixed_step_uses_the_reference_rows_and_times(monkeypatch, method, grid):
    t0, t1 = GRIDS[grid]
    slopes, times, sums = [], [], []

    def field(t, y):
        assert t.dtype == torch.float32
        times.append(float(t))
        slopes.append(torch.full((2, 3), float(len(slopes) + 1)))
        return slopes[-1]

    def recording(y, ks, coefs, h):
        which = [next(j for j, s in enumerate(slopes) if s is k) for k in ks]
        sums.append((list(zip(which, [float(c) for c in coefs])), h))
        return y

    monkeypatch.setattr(ode, "combine", recording)
    ode._fixed_step(field, method, t0, t1 - t0, t1, torch.zeros(2, 3))
    assert [terms for terms, _h in sums] == R.fixed_rows(method)
    assert all(h == t1 - t0 for _terms, h in sums)
    want = [float(np.float32(t)) for t in R.fixed_stage_times(method, t0, t1)]
    assert times == want
    assert ode.stage_times(method, [t0, t1]) == want


# -------------------------------------------------------------------------------------- 3. empirical order --
Y0 = R.Y0


@pytest.mark.parametrize("method, ns", [("euler", (8, 16, 32)), ("midpoint", (4, 8, 16)), ("rk4", (4, 8, 16))])
def test_fixed_grid_methods_converge_at_their_order(method, ns):
    field = R.DecayCos()
    exact = field.exact(1.0, Y0)
    errs = [float((R.fixed64(field, Y0, np.linspace(0, 1, n + 1), method)[-1] - exact).abs().max()) for n in ns]
    ratios = [a / b for a, b in zip(errs, errs[1:])]
    print(f"{method}: errors {errs}, ratios {ratios}")
    assert math.log2(ratios[-1]) >= R.ORDER[method] - 0.5


def test_one_dormand_prince_step_local_error_and_estimator():
    field = R.DecayCos()
    local, est = [], []
    for h in (0.4, 0.2, 0.1):
        a = R.attempt64(field, 0.0, Y0, field(0.0, Y0), h)
        local.append(float((a["y1"] - field.exact(h, Y0)).abs().max()))
        est.append(float(a["err"].abs().max()))
        assert torch.equal(a["ks"][6], field(h, a["y1"]))   # FSAL
    r_local, r_est = local[1] / local[2], est[1] / est[2]
    print(f"one DP step: local errors {local} (last ratio {r_local:.1f}), estimates {est} (last ratio {r_est:.1f})")
    assert math.log2(r_local) >= 6 - 0.5
    assert math.log2(r_est) >= 5 - 0.5
    assert est[2] > local[2]                                # the estimate is the fourth-order solution's error: the larger


def test_the_fp32_restatements_are_the_oracles_arithmetic():
    """fixed32 / dopri5_32 (numpy, over fixed_rows / dp_device) and oracle/flow.py (torch, over ode.py's constants) are two
    statements of the same fp32 arithmetic: bit for bit on an analytic field."""
    field = R.DecayCos()
    y0 = Y0.float()
    for method in ("euler", "midpoint", "rk4"):
        ts = [0.0, 0.3, 0.65, 1.0]
        a = R.fixed32(R.as_numpy_field(field), y0.numpy(), ts, method)
        b = oflow.odeint_fixed(field, y0, ts, method)
        assert np.array_equal(a, b.numpy()), method
    a, info = R.dopri5_32(R.as_numpy_field(field), y0.numpy(), [0.0, 0.4, 1.0], 1e-3, 1e-3)
    b, n_eval = oflow.odeint_dopri5(lambda t, y: field(np.float32(t).item(), y), y0, [0.0, 0.4, 1.0], 1e-3, 1e-3)
    assert n_eval == info["n_eval"] and np.array_equal(a, b.numpy())


# ------------------------------------------------------------------------------- 4. whole adaptive runs --
@pytest.mark.parametrize("ts", R.ADAPTIVE_GRIDS, ids=["one_interval", "interior_time"])
@pytest.mark.parametrize("name", list(R.ADAPTIVE))
def test_oracle_dopri5_takes_the_float64_step_sequence(name, ts):
    refs = R.adaptive_reference(name, ts)
    field, y0, tol = refs[:3]
    times = []

    def f(t, y):
        times.append(float(t))
        return field(float(t), y)

    y, n_eval = oflow.odeint_dopri5(f, y0.float(), ts, tol, tol)
    R.check_against_dopri5_64(f"oracle/flow.odeint_dopri5 {name}", times, y[-1], n_eval, refs)


@pytest.mark.parametrize("ts", R.ADAPTIVE_GRIDS, ids=["one_interval", "interior_time"])
@pytest.mark.parametrize("name", list(R.ADAPTIVE))
def test_ode_py_dopri5_takes_the_float64_step_sequence(monkeypatch, name, ts):
    refs = R.adaptive_reference(name, ts)
    field, y0, tol, y64, i64 = refs[:5]
    times = []

    def f(t, y):
        assert t.dtype == torch.float32
        times.append(float(t))
        return field(t, y)

    def cpu_combine(y, ks, coefs, h):
        return torch.from_numpy(R.combine32(y.numpy(), [k.numpy() for k in ks], [float(c) for c in coefs], float(h)))

    monkeypatch.setattr(ode, "combine", cpu_combine)
    stats = {}
    y = ode._dopri5(f, y0.float(), ts, tol, tol, stats=stats)
    assert y.shape == (len(ts),) + tuple(y0.shape)
    assert (stats["n_accept"], stats["n_reject"]) == (i64["n_accept"], i64["n_reject"])
    R.check_against_dopri5_64(f"ode._dopri5 {name}", times, y[-1], len(times), refs)
    if len(ts) > 2:                                         # the interior slot too
        assert rel_err(y[1], y64[1]) <= 4 * max(rel_err(refs[5][1], y64[1]), 1e-6)


def test_dopri5_64_converges_to_the_closed_form():
    """Tolerance-proportionality on the smooth field: a hundredth of the tolerance brings the float64 run at least ten
    times closer to the exact solution (a fifth-order pair gives about a hundred).  The front field's closed form is held
    by the classical RK4 converging to it at order 4, and the adaptive run by getting closer at the tighter tolerance."""
    field = R.DecayCos()
    errs = [rel_err(R.dopri5_64(field, Y0, [0.0, 1.0], tol, tol)[0][-1], field.exact(1.0, Y0)) for tol in (1e-5, 1e-7)]
    print(f"DecayCos: dopri5_64 against the closed form at tol 1e-5 / 1e-7: {errs}")
    assert errs[1] <= errs[0] / 10
    field, y0 = R.Front(), R.front_y0()
    exact = field.exact(1.0, y0)
    fine = [rel_err(R.fixed64(field, y0, np.linspace(0, 1, n + 1), R.CLASSICAL_RK4)[-1], exact) for n in (200, 400)]
    errs = [rel_err(R.dopri5_64(field, y0, [0.0, 1.0], tol, tol)[0][-1], exact) for tol in (1e-5, 1e-7)]
    print(f"Front: classical RK4 at 200 / 400 intervals {fine}, dopri5_64 at tol 1e-5 / 1e-7 {errs}")
    assert math.log2(fine[0] / fine[1]) >= 4 - 0.5
    assert errs[1] < errs[0]


def test_initial_step_restatement():
    field = R.DecayCos()
    h = R.initial_step64(field, 0.0, Y0, field(0.0, Y0), 1e-5, 1e-5)
    # by hand: d0, d1 are both large, so h0 = 0.01 d0 / d1; h1 from the larger of d1, d2; the result is the smaller
    scale = 1e-5 + Y0.abs() * 1e-5
    d0, d1 = float((Y0 / scale).pow(2).mean().sqrt()), float((field(0.0, Y0) / scale).pow(2).mean().sqrt())
    assert 100 * 0.01 * d0 / d1 > h > 0 and h <= (0.01 / d1) ** 0.2


# ------------------------------------------------------------------------------------------ 5. controller --
def dec_factor(ratio):
    """0.9 / ratio^(1/5) by the decimal module (40 digits): independent of libm's pow."""
    with decimal.localcontext() as ctx:
        ctx.prec = 40
        return float(decimal.Decimal("0.9") / (decimal.Decimal(ratio).ln() / 5).exp())


# (t, h, t_end, ratio) -> (clipped, accepted, new t, new h); new h approximate to 4 ulps where a power enters
CONTROLLER_TABLE = [
    ((0.0, 0.3, 1.0, 0.0), (False, True, 0.3, 0.3 * 10.0)),                        # ratio 0: the growth cap, no power
    ((0.0, 0.3, 1.0, 1.0 - 1e-6), (False, True, 0.3, 0.3)),       # just below 1: accepted; 0.9 / r^0.2 < 1 does not shrink it
    ((0.0, 0.3, 1.0, 1.0 + 1e-6), (False, False, 0.0, 0.3 * dec_factor(1.0 + 1e-6))),  # just above: rejected, shrinks
    ((0.0, 0.3, 1.0, 1.0), (False, True, 0.3, 0.3 * 0.9)),                         # exactly 1: accepted, and h x 0.9
    ((0.0, 0.3, 1.0, 1e6), (False, False, 0.0, 0.3 * 0.2)),                        # dfactor 0.2 binds
    ((0.0, 0.3, 1.0, 1e-8), (False, True, 0.3, 0.3 * 10.0)),                       # ifactor 10 binds
    ((0.0, 0.3, 0.3, 0.5), (True, True, 0.3, 0.3 * dec_factor(0.5))),              # h == t_end - t: clipped
    ((0.0, 1.0, 1.5, 3.146), (False, False, 0.0, 1.0 * dec_factor(3.146))),
    ((0.0, 1.0, 1.0, 3.146), (True, False, 0.0, 1.0 * dec_factor(3.146))),         # clipped reject: from hh, not from h
    ((0.0, 2.0, 1.0, 3.146), (True, False, 0.0, 1.0 * dec_factor(3.146))),
    ((0.0, 0.5, 0.3, 0.342), (True, True, 0.3, 0.5)),                              # clipped accept: h survives by the max
    ((0.0, 0.11, 0.1, 0.0085), (True, True, 0.1, 0.1 * dec_factor(0.0085))),       # clipped accept: hh x factor wins
    ((0.1, 0.5, 0.4, 0.5), (True, True, 0.4, 0.5)),
    ((0.15, 1.0, 0.45, 0.5), (True, True, 0.45, 1.0)),                                # lands on t_end, not on t + (t_end - t)
]


@pytest.mark.parametrize("state, want", CONTROLLER_TABLE)
def test_controller_table(state, want):
    t, h, t_end, ratio = state
    got = R.controller(dict(t=t, h=h, t_end=t_end, n_accept=3, n_reject=1), ratio)
    clipped, accepted, t_new, h_new = want
    assert (got["clipped"], got["accepted"]) == (clipped, accepted)
    assert got["t"] == t_new                                # bit for bit
    assert abs(got["h"] - h_new) <= 4 * 2.0 ** -52 * h_new, (got["h"], h_new)
    assert (got["n_accept"], got["n_reject"]) == (3 + accepted, 1 + (not accepted))
    assert got["hh"] == (t_end - t if clipped else h)


def test_controller_table_premises():
    assert 0.15 + (0.45 - 0.15) != 0.45                         # why a clipped accept assigns t_end (0.1 -> 0.4 happens to land)
    assert dec_factor(1.0 - 1e-6) < 1.0
    assert dec_factor(1e6) < 0.2 and dec_factor(1e-8) > 10.0
    assert 0.1 * dec_factor(0.0085) > 0.11 and 0.3 * dec_factor(0.342) < 0.5
