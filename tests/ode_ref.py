"""TEST INFRASTRUCTURE - an independent float64 reference of the ODE samplers (codlad_amd/diffusion_and_flow/ode.py,
ode_kernels.hip, codlad_ode_loop / codlad_ode_dopri5_attempt of denoiser_forward.hip).

Nothing here is imported from the code under test.  The Butcher tableaus are typed from the published methods as exact
rationals (Dormand & Prince 1980, J. Comp. Appl. Math. 6, table 2; Hairer, Norsett, Wanner, Solving ODEs I, II.1 for
Euler, the explicit midpoint rule and Kutta's 3/8 rule; the embedded fourth-order weights b_hat in the form torchdiffeq's
dopri5 lists them, as the difference b - b_hat).  tests/test_ode_ref_host.py proves them against the order conditions in
rational arithmetic, so a wrong digit here cannot go unnoticed either.

Three layers:
  rationals             TABLEAUS, DP_B_HAT
  the device's form     dp_device() / fixed_rows(): each coefficient as the double a single division gives (c_err: the
                        difference of two such doubles), in the order the kernels sum the terms; attempt32_from_slopes /
                        fixed32 / dopri5_32 then repeat the kernels' fp32 arithmetic in numpy, one rounding per operation
  float64               attempt64, fixed64, dopri5_64, initial_step64, controller: the same methods in double
and two analytic velocity fields with closed-form solutions.
"""
import math
from fractions import Fraction as Fr

import numpy as np
import torch

# ---------------------------------------------------------------------------------------------- rationals --
# name -> (c, A, b); A[i] = the i entries of row i
TABLEAUS = {
    "euler": ((Fr(0),), ((),), (Fr(1),)),
    "midpoint": ((Fr(0), Fr(1, 2)), ((), (Fr(1, 2),)), (Fr(0), Fr(1))),
    "rk4": ((Fr(0), Fr(1, 3), Fr(2, 3), Fr(1)),                       # Kutta's 3/8 rule (torchdiffeq's fixed-grid rk4)
            ((), (Fr(1, 3),), (Fr(-1, 3), Fr(1)), (Fr(1), Fr(-1), Fr(1))),
            (Fr(1, 8), Fr(3, 8), Fr(3, 8), Fr(1, 8))),
    "dopri5": ((Fr(0), Fr(1, 5), Fr(3, 10), Fr(4, 5), Fr(8, 9), Fr(1), Fr(1)),
               ((),
                (Fr(1, 5),),
                (Fr(3, 40), Fr(9, 40)),
                (Fr(44, 45), Fr(-56, 15), Fr(32, 9)),
                (Fr(19372, 6561), Fr(-25360, 2187), Fr(64448, 6561), Fr(-212, 729)),
                (Fr(9017, 3168), Fr(-355, 33), Fr(46732, 5247), Fr(49, 176), Fr(-5103, 18656)),
                (Fr(35, 384), Fr(0), Fr(500, 1113), Fr(125, 192), Fr(-2187, 6784), Fr(11, 84))),
               (Fr(35, 384), Fr(0), Fr(500, 1113), Fr(125, 192), Fr(-2187, 6784), Fr(11, 84), Fr(0))),
}
DP_B_HAT = (Fr(1951, 21600), Fr(0), Fr(22642, 50085), Fr(451, 720), Fr(-12231, 42400), Fr(649, 6300), Fr(1, 60))
CLASSICAL_RK4 = ((Fr(0), Fr(1, 2), Fr(1, 2), Fr(1)), ((), (Fr(1, 2),), (Fr(0), Fr(1, 2)), (Fr(0), Fr(0), Fr(1))),
                 (Fr(1, 6), Fr(1, 3), Fr(1, 3), Fr(1, 6)))            # for fine-grid solutions: a tableau nothing else uses
ORDER = {"euler": 1, "midpoint": 2, "rk4": 4, "dopri5": 5}


# ------------------------------------------------------------------------------------- order conditions --
def rooted_trees(max_order):
    """Every rooted tree with at most max_order vertices, a tree being the tuple of its root's subtrees (a multiset,
    written in non-increasing position of this very list); ordered by vertex count."""
    trees = [()]
    for order in range(2, max_order + 1):
        new = []

        def rec(remaining, max_idx, acc):
            if remaining == 0:
                new.append(tuple(acc))
                return
            for i in range(max_idx, -1, -1):
                o = tree_order(trees[i])
                if o <= remaining:
                    rec(remaining - o, i, acc + [trees[i]])

        rec(order - 1, len(trees) - 1, [])
        trees += new
    return trees


def tree_order(tree):
    return 1 + sum(tree_order(s) for s in tree)


def tree_gamma(tree):
    """The density gamma(t): the tree's order times the densities of the root's subtrees."""
    g = tree_order(tree)
    for s in tree:
        g *= tree_gamma(s)
    return g


def elementary_weight(tree, A, b):
    """sum_i b_i Phi_i(t) in exact arithmetic, Phi_i(t) = prod over the root's subtrees s of sum_j a_ij Phi_j(s)."""
    n = len(b)

    def phi(t):
        out = []
        subs = [phi(s) for s in t]
        for i in range(n):
            v = Fr(1)
            for p in subs:
                v *= sum((A[i][j] * p[j] for j in range(len(A[i]))), Fr(0))
            out.append(v)
        return out

    return sum((bi * pi for bi, pi in zip(b, phi(tree))), Fr(0))


def order_defects(A, b, order):
    """{tree: elementary weight - 1 / gamma} over every rooted tree of at most `order` vertices (all zero: the method has
    that order)."""
    return {t: elementary_weight(t, A, b) - Fr(1, tree_gamma(t)) for t in rooted_trees(order)}


# ------------------------------------------------------------------------------------ the device's form --
def dbl(q):
    """The double of a rational as the sources form it: one division of two exactly represented integers."""
    return q.numerator / q.denominator


def dp_device():
    """Dormand-Prince as ode.py and the .hip sources hold it: alpha [6], beta (rows of 1..6 doubles), c_sol [7],
    c_err [7] = dbl(b_j) - dbl(b_hat_j), a difference of two rounded doubles."""
    c, A, b = TABLEAUS["dopri5"]
    return dict(alpha=tuple(dbl(v) for v in c[1:]), beta=tuple(tuple(dbl(v) for v in row) for row in A[1:]),
                c_sol=tuple(dbl(v) for v in b), c_err=tuple(dbl(p) - dbl(q) for p, q in zip(b, DP_B_HAT)))


def fixed_rows(method):
    """The sums of a fixed-grid step in the kernels' order: per stage s (the last entry: the step's result) the list of
    (slope index, double coefficient).  The order follows torchdiffeq: ascending, except stage 3 of the 3/8 rule, which
    is written y + dt * (k2 - k1 / 3): k2 first."""
    c, A, b = TABLEAUS[method]
    rows = []
    for i in list(range(1, len(c))) + [None]:
        coefs = b if i is None else A[i]
        terms = [(j, dbl(v)) for j, v in enumerate(coefs) if v != 0]
        if method == "rk4" and i == 2:
            terms = terms[::-1]
        rows.append(terms)
    return rows


def fixed_stage_times(method, t0, t1):
    """The times a fixed-grid step evaluates the field at, in double: t0 + dt * p / q for c = p / q (left to right),
    and the grid point itself for c = 1."""
    dt = t1 - t0
    return [t1 if c == 1 else (t0 if c == 0 else t0 + dt * c.numerator / c.denominator) for c in TABLEAUS[method][0]]


def f32(v):
    return np.float32(v)


def combine32(y, ks, coefs, h_f):
    """y + sum k_j * (coef_j * h), numpy float32, one rounding per operation, left to right (ode_combine_kernel)."""
    h_f = f32(h_f)
    acc = ks[0] * (f32(coefs[0]) * h_f)
    for k, c in zip(ks[1:], coefs[1:]):
        acc = acc + k * (f32(c) * h_f)
    return (y + acc).astype(np.float32)


def error_ratio(err, y, y1, rtol, atol):
    """The double root-mean-square of the fp32 quotient err / (atol + rtol * max(|y|, |y1|))."""
    tol = f32(atol) + f32(rtol) * np.maximum(np.abs(y), np.abs(y1))
    q = (err / tol).astype(np.float32).astype(np.float64)
    return math.sqrt(float(np.sum(q * q)) / q.size)


def attempt32_from_slopes(y, ks, hh_f, rtol=1e-5, atol=1e-5):
    """y [..] and the seven slopes (numpy float32), the step as the device's float -> dict(xin = the six stage inputs,
    y1, err, ratio), in the kernels' arithmetic."""
    y = np.asarray(y, np.float32)
    ks = [np.asarray(k, np.float32) for k in ks]
    assert len(ks) == 7
    dp = dp_device()
    xin = [combine32(y, ks[:j + 1], dp["beta"][j], hh_f) for j in range(6)]
    y1 = combine32(y, ks, dp["c_sol"], hh_f)
    err = combine32(np.zeros_like(y), ks, dp["c_err"], hh_f)
    return dict(xin=xin, y1=y1, err=err, ratio=error_ratio(err, y, y1, rtol, atol))


# ----------------------------------------------------------------------------------------------- float64 --
def _t64(v):
    return torch.as_tensor(v, dtype=torch.float64)


def error_ratio64(err, y, y1, rtol, atol):
    return float((err / (atol + rtol * torch.maximum(y.abs(), y1.abs()))).pow(2).mean().sqrt())


def attempt64(f, t, y, k1, hh, rtol=1e-5, atol=1e-5):
    """One Dormand-Prince attempt in float64 (torch tensors; f(t, y) any float64 callable, t a Python double) ->
    dict(xin [6], ks [7], y1, err, ratio)."""
    c, A, b = TABLEAUS["dopri5"]
    ks, xin = [k1], []
    for i in range(1, 7):
        x = y + hh * sum(dbl(a) * k for a, k in zip(A[i], ks))
        xin.append(x)
        ks.append(f(t + dbl(c[i]) * hh, x))
    y1 = xin[5]                                             # the FSAL row: the last stage's input is the step's result
    err = hh * sum((dbl(p) - dbl(q)) * k for p, q, k in zip(b, DP_B_HAT, ks))
    return dict(xin=xin, ks=ks, y1=y1, err=err, ratio=error_ratio64(err, y, y1, rtol, atol))


def attempt32(f, t, y, k1, hh, rtol=1e-5, atol=1e-5):
    """The same attempt in the step-wise path's fp32 arithmetic (numpy; f(float32 time, float32 array))."""
    dp = dp_device()
    ks, xin = [k1], []
    for j in range(6):
        xin.append(combine32(y, ks, dp["beta"][j], hh))
        ks.append(np.asarray(f(f32(t + dp["alpha"][j] * hh), xin[-1]), np.float32))
    out = attempt32_from_slopes(y, ks, f32(hh), rtol, atol)
    out["ks"] = ks
    return out


def step_of(t, h, t_end):
    """(hh, clipped): a step that would reach or pass the output time is clipped to end on it."""
    clipped = h >= t_end - t
    return (t_end - t if clipped else h), clipped


def controller(state, ratio):
    """torchdiffeq's _optimal_step_size (safety 0.9, ifactor 10, dfactor 0.2, no shrinking after an accepted step) with
    the accept, clip and commit rules, in Python doubles.  state: dict(t, h, t_end, n_accept, n_reject) ->
    dict(t, h, hh, clipped, accepted, n_accept, n_reject)."""
    t, h, t_end = state["t"], state["h"], state["t_end"]
    hh, clipped = step_of(t, h, t_end)
    accepted = ratio <= 1.0
    if ratio == 0.0:
        factor = 10.0
    else:
        dfactor = 1.0 if ratio < 1.0 else 0.2
        factor = min(10.0, max(0.9 / ratio ** 0.2, dfactor))
    if accepted:
        t = t_end if clipped else t + hh                    # a clipped step ends on the output time, bit for bit
    # an accepted clipped step says nothing against h: the controller's own step survives it
    h = max(h, hh * factor) if (clipped and accepted) else hh * factor
    return dict(t=t, h=h, hh=hh, clipped=clipped, accepted=accepted,
                n_accept=state.get("n_accept", 0) + int(accepted), n_reject=state.get("n_reject", 0) + int(not accepted))


def _rms64(x):
    return float(torch.as_tensor(x).double().pow(2).mean().sqrt())


def initial_step64(f, t0, y0, f0, rtol, atol, order=4):
    """Hairer, Norsett, Wanner II.4, in float64."""
    scale = atol + y0.abs() * rtol
    d0, d1 = _rms64(y0 / scale), _rms64(f0 / scale)
    h0 = 1e-6 if (d0 < 1e-5 or d1 < 1e-5) else 0.01 * d0 / d1
    f1 = f(t0 + h0, y0 + h0 * f0)
    d2 = _rms64((f1 - f0) / scale) / h0
    h1 = max(1e-6, h0 * 1e-3) if (d1 <= 1e-15 and d2 <= 1e-15) else (0.01 / max(d1, d2)) ** (1.0 / (order + 1))
    return min(100 * h0, h1)


def _dopri5(f, y0, ts, rtol, atol, attempt, first_step, max_steps=10000):
    ts = [float(v) for v in ts]
    t, y = ts[0], y0
    k1 = f(t, y)
    h = first_step(f, t, y, k1)
    out, log, n_eval = [y0], [], 2
    st = dict(t=t, h=h, n_accept=0, n_reject=0)
    for t_end in ts[1:]:
        while st["t"] < t_end:
            assert len(log) < max_steps
            st["t_end"] = t_end
            hh, _clipped = step_of(st["t"], st["h"], t_end)
            a = attempt(f, st["t"], y, k1, hh, rtol, atol)
            n_eval += 6
            new = controller(st, a["ratio"])
            log.append(dict(t=st["t"], hh=hh, clipped=new["clipped"], ratio=a["ratio"], accepted=new["accepted"]))
            if new["accepted"]:
                y, k1 = a["y1"], a["ks"][6]
            st = dict(t=new["t"], h=new["h"], n_accept=new["n_accept"], n_reject=new["n_reject"])
        out.append(y)
    return out, dict(attempts=log, n_eval=n_eval, n_accept=st["n_accept"], n_reject=st["n_reject"], h0=h)


def dopri5_64(f, y0, ts, rtol, atol):
    """A whole adaptive run in float64 -> (torch [len(ts), ..], dict(attempts = [dict(t, hh, clipped, ratio, accepted)],
    n_eval, n_accept, n_reject, h0))."""
    out, info = _dopri5(f, y0.double(), ts, rtol, atol, attempt64,
                        lambda f_, t, y, k1: initial_step64(f_, t, y, k1, rtol, atol))
    return torch.stack(out), info


def dopri5_32(f, y0, ts, rtol, atol):
    """The same run in the step-wise path's fp32 arithmetic (numpy): f(float32 time, float32 array) -> float32 array."""
    def first(f_, t, y, k1):
        scale = f32(atol) + np.abs(y) * f32(rtol)
        d0, d1 = _rms64(y / scale), _rms64(k1 / scale)
        h0 = 1e-6 if (d0 < 1e-5 or d1 < 1e-5) else 0.01 * d0 / d1
        f1 = np.asarray(f_(f32(t + h0), combine32(y, [k1], [1.0], h0)), np.float32)
        d2 = _rms64((f1 - k1) / scale) / h0
        h1 = max(1e-6, h0 * 1e-3) if (d1 <= 1e-15 and d2 <= 1e-15) else (0.01 / max(d1, d2)) ** 0.2
        return min(100 * h0, h1)

    def f_np(t, y):
        return np.asarray(f(f32(t), y), np.float32)

    out, info = _dopri5(f_np, np.asarray(y0, np.float32), ts, rtol, atol, attempt32, first)
    return np.stack(out), info


def rk_step64(f, tableau, t0, t1, y):
    c, A, b = tableau
    dt = t1 - t0
    ks = []
    for i in range(len(c)):
        x = y if i == 0 else y + dt * sum(dbl(a) * k for a, k in zip(A[i], ks) if a != 0)
        ks.append(f(t1 if c[i] == 1 else t0 + dbl(c[i]) * dt, x))
    return y + dt * sum(dbl(w) * k for w, k in zip(b, ks) if w != 0)


def fixed64(f, y0, ts, method):
    """A fixed-grid run in float64 -> torch [len(ts), ..]; method a TABLEAUS name or a (c, A, b) tableau."""
    tab = TABLEAUS[method] if isinstance(method, str) else method
    ts = [float(v) for v in ts]
    out = [y0.double()]
    for t0, t1 in zip(ts, ts[1:]):
        out.append(rk_step64(f, tab, t0, t1, out[-1]))
    return torch.stack(out)


def fixed32(f, y0, ts, method):
    """The fixed-grid step-wise path in numpy fp32: stage times in double rounded once to float, every sum by combine32
    over fixed_rows(method).  f(float32 time, float32 array) -> float32 array."""
    ts = [float(v) for v in ts]
    rows = fixed_rows(method)
    out = [np.asarray(y0, np.float32)]
    for t0, t1 in zip(ts, ts[1:]):
        y, ks, x = out[-1], [], out[-1]
        for s, t in enumerate(fixed_stage_times(method, t0, t1)):
            ks.append(np.asarray(f(f32(t), x), np.float32))
            x = combine32(y, [ks[j] for j, _c in rows[s]], [c for _j, c in rows[s]], t1 - t0)
        out.append(x)
    return np.stack(out)


# --------------------------------------------------------------------------------------- analytic fields --
def _time(t, y):
    return torch.as_tensor(t, dtype=y.dtype, device=y.device)


class DecayCos:
    """y' = -2 y + cos(w t), w = (1, 2, 3) along the last axis; y(t) = C exp(-2 t) + (2 cos wt + w sin wt) / (4 + w^2)."""
    W = (1.0, 2.0, 3.0)

    def __call__(self, t, y):
        t = _time(t, y)
        w = torch.tensor(self.W, dtype=y.dtype, device=y.device)
        return -2.0 * y + torch.cos(w * t)

    def exact(self, t, y0, t0=0.0):
        y0 = y0.double()
        w = torch.tensor(self.W, dtype=torch.float64)
        part = lambda s: (2.0 * torch.cos(w * s) + w * torch.sin(w * s)) / (4.0 + w * w)  # noqa: E731
        return (y0 - part(_t64(t0))) * math.exp(-2.0 * (t - t0)) + part(_t64(t))


class Front:
    """y' = -lam(t) y with a sharp front in the decay rate: lam(t) = A + B (1 + tanh((t - 0.5) / EPS)) / 2.
    y(t) = y0 exp(-(I(t) - I(t0))), I(t) = A t + B / 2 (t + EPS log cosh((t - 0.5) / EPS))."""
    A, B, EPS = 0.5, 8.0, 0.01

    def __call__(self, t, y):
        t = _time(t, y)
        return -(self.A + self.B * 0.5 * (1.0 + torch.tanh((t - 0.5) / self.EPS))) * y

    def _integral(self, t):
        x = abs((t - 0.5) / self.EPS)
        logcosh = x + math.log1p(math.exp(-2.0 * x)) - math.log(2.0)
        return self.A * t + 0.5 * self.B * (t + self.EPS * logcosh)

    def exact(self, t, y0, t0=0.0):
        return y0.double() * math.exp(-(self._integral(t) - self._integral(t0)))


def as_numpy_field(field):
    """A torch field as f(float32 time, float32 numpy array) -> float32 numpy array (torch CPU fp32 arithmetic)."""
    def f(t, y):
        return field(torch.tensor(float(t), dtype=torch.float32), torch.from_numpy(np.ascontiguousarray(y))).numpy()
    return f


# ------------------------------------------------------------------- the adaptive runs on the analytic fields --
Y0 = torch.linspace(-1, 1, 12, dtype=torch.float64).reshape(4, 3) * 0.7 + 0.1


def front_y0():
    return Y0 * 0.003


ADAPTIVE = {"decaycos": (DecayCos, lambda: Y0, 1e-3), "front": (Front, front_y0, 1e-5)}
ADAPTIVE_GRIDS = ([0.0, 1.0], [0.0, 0.4, 1.0])


def adaptive_reference(name, ts):
    """-> (field, y0, tol, float64 run, its info, fp32 numpy run, its info, the ratio margin m); the conditions on the
    inputs are asserted here."""
    cls, y0, tol = ADAPTIVE[name]
    field, y0 = cls(), y0()
    y64, i64 = dopri5_64(field, y0, ts, tol, tol)
    y32, i32 = dopri5_32(as_numpy_field(field), y0.float().numpy(), ts, tol, tol)
    a64, a32 = i64["attempts"], i32["attempts"]
    m = 10 * max(abs(b["ratio"] - a["ratio"]) / a["ratio"] for a, b in zip(a64, a32))
    gap = min(abs(a["ratio"] - 1.0) for a in a64)
    print(f"{name} {ts}: {len(a64)} attempts ({i64['n_reject']} rejected), margin m = {m:.3f}, closest ratio to 1: {gap:.3f} away")
    assert m < gap, f"{name} {ts}: a float64 ratio lies within [1 - m, 1 + m], m = {m:.3f}"
    if name == "front":
        assert i64["n_reject"] >= 1
        if len(ts) > 2:
            assert any(a["clipped"] and a["t"] + a["hh"] < ts[-1] - 1e-9 for a in a64)    # clipped at the interior time
    return field, y0, tol, y64, i64, y32, i32, m


def attempts_from_call_times(times):
    """The (t, hh, accepted) of every attempt from the times a step-wise dopri5 evaluated the field at (after its two
    initial calls): stages 2 and 6 are at t + hh / 5 and t + hh; an attempt was accepted when the next starts later."""
    assert len(times) % 6 == 0
    att = []
    for i in range(0, len(times), 6):
        hh = (times[i + 5] - times[i]) / 0.8
        att.append((times[i] - 0.2 * hh, hh))
    return [(t, hh, i + 1 == len(att) or att[i + 1][0] > t + 0.5 * hh) for i, (t, hh) in enumerate(att)]


def rel_err(a, b):
    """max |a - b| / max |b|"""
    a, b = torch.as_tensor(a).detach().cpu().double(), torch.as_tensor(b).detach().cpu().double()
    return float((a - b).abs().max() / b.abs().max())


def check_against_dopri5_64(label, times, y_end, n_eval, refs):
    _field, _y0, _tol, y64, i64, y32, _i32, m = refs
    got = attempts_from_call_times(times[2:])
    want = i64["attempts"]
    assert n_eval == i64["n_eval"] == 2 + 6 * len(want)
    assert [a for _t, _hh, a in got] == [a["accepted"] for a in want], label
    for (_t, hh, _a), w in zip(got, want):
        assert abs(hh - w["hh"]) <= m * w["hh"]
    e32, err = rel_err(y32[-1], y64[-1]), rel_err(y_end, y64[-1])
    print(f"{label}: final state {err:.3e} from float64, the fp32 restatement {e32:.3e}")
    assert err <= 4 * max(e32, 1e-6)
