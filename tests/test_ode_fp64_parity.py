"""GPU: the ODE samplers of the flow-matching models against float64, per stage, per step and per decision.

Everything goes through the C ABI.  `Driver` allocates the codlad_ode_dopri5_bufs the way Denoiser._sample_dopri5 does,
calls codlad_ode_dopri5_attempt once and reads everything back; tests/ode_ref.py (tableaus typed from the published
methods as rationals, proven by tests/test_ode_ref_host.py) is what it is compared with.

One attempt is taken apart as follows.
  times       hh, hh_f, clipped, t_end and the six stage times tf[j] = float(t + alpha_j hh): exact.
  sums        from the DEVICE'S OWN slopes, ode_ref.attempt32_from_slopes repeats the kernels' fp32 arithmetic: the last
              stage input (xin) and y1 bit for bit, the error ratio within n 2^-52 (a double sum of n squares in another
              order, the bound of test_ode_fused.py::test_error_norm_kernel).  A wrong coefficient in the .hip copies of
              DP_BETA's last row, DP_C_SOL or DP_C_ERR fails here, one in DP_ALPHA under "times"; the inputs of stages 2 to 6
              are overwritten before anything can be read back, so a wrong coefficient in DP_BETA's rows 0 to 4 fails under
              "slopes": the device then evaluated its slope at another input than the recomputed one.
  slopes      every k[j] against the float64 oracle's forward at the (bit-exactly recomputed) stage input, with the
              substitutions and the rule of tests/test_fp64_parity.py: the device's own h_E0 rows, neighbour lists and adaLN
              row mods[j]; per node and channel within c_mode x max(e_ref[ch], 1e-6), c_mode = 4 (f32, f16x4) or 16 (f16x3).
  adaLN rows  the six rows against float64 oden.step_mods at tf[j]: 5e-6 of the maximum (test_hip_parity.py::test_step_mods).
  ratio       against ode_ref.attempt64 over the float64 oracle field (its own slopes): within 4 x max(e_ref, floor), e_ref the
              fp32 CPU oracle's own relative deviation of the ratio.  floor: the slope rule above admits an error of FLOOR =
              1e-6 of the channel's maximum in every slope, and the ratio cannot be held tighter than what such errors do
              to it: floor = rms(hh sum_j |c_err_j| 1e-6 max|k_j[:, ch]| / tol) / ratio, from the float64 slopes.  (A floor from
              the fp32 storage of the slopes alone, 2^-24 |k_j|, is too tight at hh = 1: the device's slopes differ from
              float64 by 1e-6 to 2e-6 of the channel maximum at most nodes, the CPU oracle's fp32 by that much at its worst
              node only, and random slope errors of 2e-6 injected into attempt64 on the CPU move the ratio of L46_B2 by
              7e-4 - what the device shows in all three modes; DESIGN.md has the figures.)
              Not at hh = 0.02: there the estimate is the cancellation noise of fp32 slopes (the fp32 oracle's ratio
              4.7e-5, float64's 8.7e-6), and what is derivable is asserted instead, per element:
              |err_dev - err_64| <= hh_f sum_j |c_err_j| |k_j_dev - k_j_64| + 8 ulp of sum_j |c_err_j k_j| hh_f.
  decision    accepted, clipped, the counters and the new t equal ode_ref.controller (a Python-double restatement of
              torchdiffeq's rule) fed with the device's ratio; the new h within 16 x 2^-52 (two pows a couple of ulps each,
              a division and a product); after a reject y and k[0] keep their bits, after an accept y = y1 and k[0] = k[6].

Measured figures: DESIGN.md section 2, "The ODE samplers against float64".
"""
import ctypes as C

import numpy as np
import pytest
import torch

import tests.test_fp64_parity as fp
from codlad_amd import _lib, engine, synth
from codlad_amd.diffusion_and_flow import ode
from codlad_amd.engine import Denoiser
from oracle import denoiser as oden
from oracle import flow as oflow
from tests import cases
from tests import conditioning as cond
from tests import ode_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MODES = fp.MODES
TOL = 1e-5
U24, U52 = 2.0 ** -24, 2.0 ** -52


# ---------------------------------------------------------------------------------------------- geometries --
def spec_of(name):
    """The jobs of this file, in the form tests/test_fp64_parity.py's oracle_run takes (kind "three": the flow model)."""
    base = dict(kind="three", t=0.0, x_sc=None)
    if name in ("L20_B2", "L46_B2"):
        L, B, seed = cases.DENOISER_CASES[name]
        prot, _batch, x, _t, _mask = cases.denoiser_inputs(L, B, seed)
        xyz, z = fp._frames(prot)
        return dict(base, xyz=xyz, z=[z] * B, members=list(range(B)), x=x.reshape(-1, 3))
    if name == "n15":                    # three members of a length-5 structure: a partial last block of ode_stage_kernel
        xyz, z = fp._frames(synth.make_protein(5, 75, n_frames=1))
        return dict(base, xyz=xyz, z=[z], members=[0, 0, 0], x=synth.gaussian((15, 3), 1500))
    if name == "ragged_46_87_87":        # 660 elements: three norm blocks, the last one partial
        return dict(fp.spec_of(name), **base)
    if name == "big":                    # 44 x 505 nodes = 66 660 elements: the 256-block cap of the norm, a partial last chunk
        xyz, z = fp._frames(synth.make_protein(505, 575, n_frames=1))
        return dict(base, xyz=xyz, z=[z], members=[0] * 44, x=synth.gaussian((44 * 505, 3), 1505))
    raise KeyError(name)


_sd = {}


def flow_sd(zero_head=False):
    if zero_head not in _sd:
        sd = synth.denoiser_state_dict(cases.WEIGHT_SEED, flow=True)
        if zero_head:
            sd["W_out.linear.weight"] = torch.zeros_like(sd["W_out.linear.weight"])
            sd["W_out.linear.bias"] = torch.zeros_like(sd["W_out.linear.bias"])
        _sd[zero_head] = sd
    return _sd[zero_head]


_setups = {}


def setup(name, mode, zero_head=False):
    """(engine, spec, job, the device's edge state for the oracle) - built once per geometry and mode."""
    key = (name, mode, zero_head)
    if key not in _setups:
        den = fp.engine_of("three", mode) if not zero_head else Denoiser(flow_sd(True), DEV, precision=mode)
        spec = spec_of(name)
        st = den.prepare_structures(spec["xyz"], spec["z"])
        job = den.make_job(st, spec["members"])
        rows = engine.edge_rows(st.h_E0, split=den.split_edge_state).cpu()
        idx = st.E_idx.cpu().long()
        hE0, E_idx = [], []
        for f, L in enumerate(st.lens):
            a, K = int(st.offsets[f]), min(64, L)
            hE0.append(rows[a:a + L, :K].clone())
            E_idx.append(idx[a:a + L, :K].clone())
        _setups[key] = (den, spec, job, dict(hE0=hE0, E_idx=E_idx))
    return _setups[key]


def oracle_out(spec, edge, x, mods, dtype):
    """The oracle's velocity [n_nodes, 3] in `dtype` at x from the device's edge state and the adaLN row `mods`."""
    x = torch.as_tensor(x).reshape(-1, 3)
    return fp.oracle_run(flow_sd(), dict(spec, x=x), dict(edge, mods=torch.as_tensor(mods)), dtype)[0]


def oracle_field(spec, edge, dtype):
    """f(t, y [n_nodes, 3]) in `dtype`: the oracle over the device's edge state, the adaLN row its own at its own t."""
    sdd = cond.to_dtype(flow_sd(), dtype)

    def f(t, y):
        mods = oden.step_mods(sdd, torch.tensor([float(t)], dtype=dtype))[0]
        return oracle_out(spec, edge, torch.as_tensor(y).to(dtype), mods, dtype)
    return f


def numpy_field(f32_field):
    return lambda t, y: f32_field(float(t), torch.from_numpy(np.ascontiguousarray(y))).numpy()


# -------------------------------------------------------------------------------------------------- driver --
def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


class Driver:
    """The buffers of codlad_ode_dopri5_attempt as Denoiser._sample_dopri5 allocates them, and one call at a time."""

    def __init__(self, den, job, y, t, h):
        f32 = dict(dtype=torch.float32, device=DEV)
        n = job.n_nodes
        self.den, self.job = den, job
        self.y = y.detach().clone().contiguous().float().to(DEV)
        assert self.y.shape == (n, 3)
        self.k = [den.forward(job, self.y, float(t))] + [torch.zeros(n, 3, **f32) for _ in range(6)]
        self.y1, self.xin = torch.zeros(n, 3, **f32), torch.zeros(n, 3, **f32)
        self.mods = torch.zeros(6, engine.MODS, **f32)
        self.norm = torch.zeros(_lib.ODE_NORM_WORDS, dtype=torch.float64, device=DEV)
        host = _lib.OdeState()
        host.t, host.h = float(t), float(h)
        self.state = torch.frombuffer(bytearray(bytes(host)), dtype=torch.uint8).to(DEV)
        self.bufs = _lib.OdeDopri5Bufs()
        self.bufs.y, self.bufs.y1, self.bufs.xin, self.bufs.mods, self.bufs.state, self.bufs.norm = (
            _lib.ptr(t_) for t_ in (self.y, self.y1, self.xin, self.mods, self.state, self.norm))
        for j in range(7):
            self.bufs.k[j] = self.k[j].data_ptr()
        self.desc = job.desc()
        self.k0_mods = den.step_mods([float(t)])[0].cpu().clone()      # the adaLN row Denoiser.forward used for k[0]

    def read_state(self):
        return _lib.OdeState.from_buffer_copy(self.state.cpu().numpy().tobytes())

    def attempt(self, t_end, rtol=TOL, atol=TOL):
        """-> (before, after): y, k[0] and the state block before the call; everything after it (numpy / OdeState)."""
        before = dict(y=self.y.cpu().numpy().copy(), k0=self.k[0].cpu().numpy().copy(), state=self.read_state())
        self.den._run("codlad_ode_dopri5_attempt", self.desc, C.byref(self.bufs), C.c_double(t_end), C.c_float(rtol),
                      C.c_float(atol))
        torch.cuda.synchronize()
        after = dict(y=self.y.cpu().numpy().copy(), y1=self.y1.cpu().numpy().copy(), xin=self.xin.cpu().numpy().copy(),
                     k=[k.cpu().numpy().copy() for k in self.k], mods=self.mods.cpu().clone(), state=self.read_state(),
                     norm0=float(self.norm[0]), t_end=float(t_end), rtol=rtol, atol=atol)
        return before, after


# ---------------------------------------------------------------------------------------- per-attempt checks --
def check_sums(label, before, after):
    """Times, the sums recomputed from the device's slopes, the decision and the commit -> the recomputation."""
    s0, s1, t_end = before["state"], after["state"], after["t_end"]
    hh, clipped = R.step_of(s0.t, s0.h, t_end)
    dp = R.dp_device()
    assert (s1.hh, bool(s1.clipped), s1.t_end) == (hh, clipped, t_end), label
    assert s1.hh_f == float(np.float32(hh)), label
    assert list(s1.tf) == [float(np.float32(s0.t + a * hh)) for a in dp["alpha"]], label
    ks = [before["k0"]] + after["k"][1:]
    re = R.attempt32_from_slopes(before["y"], ks, np.float32(hh), after["rtol"], after["atol"])
    re["ks"] = ks
    assert np.array_equal(bits(after["xin"]), bits(re["xin"][5])), f"{label}: the last stage input"
    assert np.array_equal(bits(after["y1"]), bits(re["y1"])), f"{label}: y1"
    n = before["y"].size
    ratio = s1.ratio
    assert after["norm0"] == ratio and not s1.nonfinite and s1.status == 0, label
    dev = abs(ratio - re["ratio"]) / re["ratio"] if re["ratio"] else abs(ratio)
    assert dev <= n * U52, f"{label}: ratio {ratio!r}, recomputed {re['ratio']!r}"
    want = R.controller(dict(t=s0.t, h=s0.h, t_end=t_end, n_accept=s0.n_accept, n_reject=s0.n_reject), ratio)
    got = (bool(s1.accepted), bool(s1.clipped), s1.n_accept, s1.n_reject, s1.t)
    assert got == (want["accepted"], want["clipped"], want["n_accept"], want["n_reject"], want["t"]), (label, got, want)
    dh = abs(s1.h - want["h"]) / want["h"]
    assert dh <= 16 * U52, f"{label}: new h {s1.h!r}, the controller's {want['h']!r}"
    if want["accepted"]:                                    # the commit: y1 -> y, k7 -> k1 (FSAL)
        assert np.array_equal(bits(after["y"]), bits(after["y1"])) and np.array_equal(bits(after["k"][0]), bits(after["k"][6]))
    else:
        assert np.array_equal(bits(after["y"]), bits(before["y"])) and np.array_equal(bits(after["k"][0]), bits(before["k0"]))
    re.update(hh=hh, ratio_dev=ratio, ratio_dev_vs_recomputed=dev / (n * U52), dh=dh / U52, want=want)
    return re


def check_slopes(label, mode, spec, edge, before, after, re, k0_mods=None):
    """Every slope against the float64 oracle at its recomputed stage input (k[0], at y, only with its adaLN row given)
    -> (worst err / max(e_ref, FLOOR), the float64 slopes)."""
    worst, k64 = 0.0, []
    for j in range(7):
        x = before["y"] if j == 0 else re["xin"][j - 1]
        mods = k0_mods if j == 0 else after["mods"][j - 1]
        if mods is None:
            k64.append(None)
            continue
        o64 = oracle_out(spec, edge, x, mods.double(), torch.float64)
        o32 = oracle_out(spec, edge, x, mods, torch.float32)
        e_ref = cond.node_channel_error(o32, o64).amax(0)
        err = cond.node_channel_error(torch.from_numpy(re["ks"][j]), o64)
        ratio = err / e_ref.clamp_min(fp.FLOOR)
        i = int(ratio.argmax())
        r = float(ratio.max())
        assert r <= fp.C_MODE[mode], (f"{label}: slope k[{j}] err/e_ref {r:.2f} at node {i // 3} channel {i % 3} "
                                      f"(err {float(err.reshape(-1)[i]):.2e}, e_ref {float(e_ref[i % 3]):.2e})")
        worst = max(worst, r)
        k64.append(o64)
    return worst, k64


def check_mods(label, after):
    sd64 = cond.to_dtype(flow_sd(), torch.float64)
    ref = oden.step_mods(sd64, torch.tensor(list(after["state"].tf), dtype=torch.float64))
    err = R.rel_err(after["mods"], ref)
    assert err < 5e-6, f"{label}: adaLN rows {err:.3e}"
    return err


def full_attempt_reference(spec, edge, before, hh):
    """attempt64 over the float64 oracle field from the device's y (its own k1 and slopes), the fp32 oracle's attempt, and
    the floor of the ratio comparison."""
    t = before["state"].t
    f64 = oracle_field(spec, edge, torch.float64)
    f32 = numpy_field(oracle_field(spec, edge, torch.float32))
    y = torch.from_numpy(before["y"]).double()
    a64 = R.attempt64(f64, t, y, f64(t, y), hh, TOL, TOL)
    a32 = R.attempt32(f32, t, before["y"], f32(np.float32(t), before["y"]), hh, TOL, TOL)
    c_err = R.dp_device()["c_err"]
    tol = TOL + TOL * torch.maximum(y.abs(), a64["y1"].abs())
    slack = hh * sum(abs(c) * fp.FLOOR * k.abs().amax(0) for c, k in zip(c_err, a64["ks"]))      # [3], per channel
    floor = float((slack / tol).pow(2).mean().sqrt()) / a64["ratio"]
    return a64, a32, floor


GEOMETRIES = ("L20_B2", "n15", "L46_B2", "ragged_46_87_87")


# ------------------------------------------------------------------------------------ 1. one attempt --
@pytest.mark.parametrize("hh", [0.1, 0.3, 1.0])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", GEOMETRIES)
def test_one_attempt_stage_by_stage(name, mode, hh):
    den, spec, job, edge = setup(name, mode)
    label = f"{name} {mode} hh {hh}"
    drv = Driver(den, job, spec["x"], 0.0, hh)
    before, after = drv.attempt(2.0)                        # t_end far away: the step is h
    re = check_sums(label, before, after)
    assert re["hh"] == hh and not after["state"].clipped
    worst, _k64 = check_slopes(label, mode, spec, edge, before, after, re, drv.k0_mods)
    e_mods = check_mods(label, after)
    a64, a32, floor = full_attempt_reference(spec, edge, before, hh)
    e_ref = abs(a32["ratio"] - a64["ratio"]) / a64["ratio"]
    dev = abs(re["ratio_dev"] - a64["ratio"]) / a64["ratio"]
    print(f"ode fp64 {label}: slopes err/e_ref {worst:.2f} (bound {fp.C_MODE[mode]:.0f}); adaLN {e_mods:.2e}; ratio device "
          f"{re['ratio_dev']:.6g} float64 {a64['ratio']:.6g}: deviation {dev:.3e}, e_ref {e_ref:.3e}, floor {floor:.3e}, "
          f"bound {4 * max(e_ref, floor):.3e}; ratio vs recomputed {re['ratio_dev_vs_recomputed']:.3f} of n 2^-52; "
          f"new h {re['dh']:.1f} x 2^-52 from the controller's")
    assert dev <= 4 * max(e_ref, floor), label


@pytest.mark.parametrize("mode", MODES)
def test_one_attempt_at_a_step_where_the_estimate_is_noise(mode):
    """hh = 0.02 on L20_B2: the error estimate is the cancellation noise of fp32 slopes, so the ratio is not compared with
    float64's.  What follows from the slopes' own errors is: per element, |err_dev - err_64| <= hh_f sum_j |c_err_j|
    |k_j_dev - k_j_64| + 8 ulp of sum_j |c_err_j k_j_dev| hh_f, err_64 the double sum over the float64 oracle's slopes at the
    device's stage inputs."""
    den, spec, job, edge = setup("L20_B2", mode)
    label = f"L20_B2 {mode} hh 0.02"
    drv = Driver(den, job, spec["x"], 0.0, 0.02)
    before, after = drv.attempt(2.0)
    re = check_sums(label, before, after)
    worst, k64 = check_slopes(label, mode, spec, edge, before, after, re, drv.k0_mods)
    hf = float(np.float32(re["hh"]))
    c_err = [float(np.float32(c)) for c in R.dp_device()["c_err"]]
    kd = [torch.from_numpy(k).double() for k in re["ks"]]
    err64 = hf * sum(c * k for c, k in zip(c_err, k64))
    bound = hf * sum(abs(c) * (a - b).abs() for c, a, b in zip(c_err, kd, k64)) + \
        8 * U24 * hf * sum(abs(c) * a.abs() for c, a in zip(c_err, kd))
    diff = (torch.from_numpy(re["err"]).double() - err64).abs()
    used = float((diff / bound).max())
    print(f"ode fp64 {label}: slopes err/e_ref {worst:.2f}; ratio {re['ratio_dev']:.4g}; |err_dev - err_64| at most {used:.3f} "
          f"of its bound (largest |err| {float(diff.max()):.2e} of {float(err64.abs().max()):.2e})")
    assert used <= 1.0


# -------------------------------------------------------------------------------------- 2. decisions --
# start (t, h, t_end) -> (clipped, accepted)
DECISIONS = {
    "unclipped_accept": ((0.0, 0.3, 1.0), (False, True)),
    "unclipped_reject": ((0.0, 1.0, 1.5), (False, False)),
    "clipped_reject": ((0.0, 1.0, 1.0), (True, False)),
    "clipped_accept_h_survives": ((0.0, 0.5, 0.3), (True, True)),
    "clipped_accept_hh_factor_wins": ((0.0, 0.11, 0.1), (True, True)),
    "boundary_h_equals_remainder": ((0.0, 0.3, 0.3), (True, True)),
    "ends_on_t_end": ((0.1, 0.5, 0.4), (True, True)),
    "ends_on_t_end_where_the_sum_misses_it": ((0.15, 1.0, 0.45), (True, True)),   # 0.15 + (0.45 - 0.15) != 0.45 in double
}


@pytest.mark.parametrize("mode", ["f16x3", "f32"])
@pytest.mark.parametrize("case", list(DECISIONS))
def test_decisions(case, mode):
    (t, h, t_end), (clipped, accepted) = DECISIONS[case]
    den, spec, job, edge = setup("L20_B2", mode)
    label = f"decision {case} {mode}"
    drv = Driver(den, job, spec["x"], t, h)
    before, after = drv.attempt(t_end)
    re = check_sums(label, before, after)
    s1 = after["state"]
    f64 = oracle_field(spec, edge, torch.float64)
    y = torch.from_numpy(before["y"]).double()
    r64 = R.attempt64(f64, t, y, f64(t, y), re["hh"], TOL, TOL)["ratio"]
    print(f"ode fp64 {label}: hh {re['hh']!r}, ratio device {s1.ratio:.6g} float64 {r64:.6g}, accepted {s1.accepted}, "
          f"clipped {s1.clipped}, t {before['state'].t!r} -> {s1.t!r}, h {before['state'].h!r} -> {s1.h!r} "
          f"({re['dh']:.1f} x 2^-52 from the controller's)")
    assert not 0.5 <= r64 <= 2.0, f"{label}: the float64 ratio {r64} is too close to 1 for a decision test"
    assert (bool(s1.clipped), bool(s1.accepted)) == (clipped, accepted) == (re["want"]["clipped"], r64 <= 1.0)
    if accepted and clipped:
        assert s1.t == t_end                                # bit for bit
    if case == "clipped_accept_h_survives":
        assert s1.h == h
    if case == "clipped_accept_hh_factor_wins":
        assert s1.h > h


@pytest.mark.parametrize("mode", ["f16x3", "f32"])
def test_decision_at_ratio_zero(mode):
    """A model whose final Linear is zero: every slope is zero, the ratio is exactly 0, the step grows tenfold."""
    den, spec, job, _edge = setup("L20_B2", mode, zero_head=True)
    drv = Driver(den, job, spec["x"], 0.0, 0.05)
    before, after = drv.attempt(1.0)
    re = check_sums(f"ratio zero {mode}", before, after)
    s1 = after["state"]
    assert all(not k.any() for k in re["ks"])
    assert s1.ratio == 0.0 and s1.accepted == 1 and s1.clipped == 0 and s1.h == 0.05 * 10.0 and s1.t == 0.05
    assert np.array_equal(bits(after["y"]), bits(before["y"]))


# --------------------------------------------------------------------------------------- 3. a whole run --
@pytest.fixture(scope="module")
def float64_runs():
    """L20_B2 over the float64 oracle (its own features): the classical RK4 - a tableau nothing else here uses - at 32
    intervals, and dopri5_64 at tol 1e-5 on both grids."""
    L, B, seed = cases.DENOISER_CASES["L20_B2"]
    _prot, batch, x, _t, mask = cases.denoiser_inputs(L, B, seed)
    cg_z, cg_xyz, _m = oden.batch_to_dense(batch)
    sd64 = cond.to_dtype(flow_sd(), torch.float64)

    def f(t, y):
        tt = torch.full((B,), float(t), dtype=torch.float64)
        return oden.forward(sd64, y, tt, cg_xyz.double(), cg_z, mask)

    fine = R.fixed64(f, x.double(), np.linspace(0.0, 1.0, 33), R.CLASSICAL_RK4)[-1]
    half = R.fixed64(f, x.double(), np.linspace(0.0, 1.0, 17), R.CLASSICAL_RK4)[-1]
    runs = {len(ts): R.dopri5_64(f, x.double(), ts, TOL, TOL) for ts in ([0.0, 1.0], [0.0, 0.4, 1.0])}
    return dict(fine=fine.reshape(-1, 3), self_consistency=R.rel_err(half, fine) / 15.0, runs=runs)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("ts", [[0.0, 1.0], [0.0, 0.4, 1.0]], ids=["one_interval", "interior_time"])
def test_a_whole_run_attempt_by_attempt(float64_runs, ts, mode):
    den, spec, job, edge = setup("L20_B2", mode)
    label = f"run {ts} {mode}"
    y0 = spec["x"].to(DEV)
    traj, stats = den.sample_ode(job, y0, ts, method="dopri5", rtol=TOL, atol=TOL)
    traj = traj.cpu().numpy()
    k0 = den.forward(job, y0, ts[0])
    h0 = ode._initial_step(lambda t, y: den.forward(job, y, float(t)), ts[0], y0, k0, TOL, TOL)
    drv = Driver(den, job, y0, ts[0], h0)
    nxt, log, worst = 1, [], 0.0
    while nxt < len(ts):
        assert len(log) < 40
        before, after = drv.attempt(ts[nxt])
        re = check_sums(f"{label} attempt {len(log) + 1}", before, after)
        w, _k64 = check_slopes(f"{label} attempt {len(log) + 1}", mode, spec, edge, before, after, re,
                               drv.k0_mods if not log else None)
        check_mods(label, after)
        worst = max(worst, w)
        s1 = after["state"]
        log.append((before["state"].t, re["hh"], bool(s1.clipped), s1.ratio, bool(s1.accepted)))
        if s1.accepted and s1.t >= ts[nxt]:
            assert s1.t == ts[nxt]
            assert np.array_equal(bits(after["y"]), bits(traj[nxt])), f"{label}: slot {nxt} is not sample_ode's"
            nxt += 1
    s1 = after["state"]
    assert s1.n_accept + s1.n_reject == len(log)
    assert stats == {"n_eval": 2 + 6 * len(log), "n_accept": s1.n_accept, "n_reject": s1.n_reject}
    y64, i64 = float64_runs["runs"][len(ts)]
    fine = float64_runs["fine"]
    e64 = R.rel_err(y64[-1].reshape(-1, 3), fine)
    err = R.rel_err(after["y"], fine)
    print(f"ode fp64 {label}: {len(log)} attempts (t, hh, clipped, ratio, accepted) {log}; float64 run: "
          f"{[(a['t'], a['hh'], a['clipped'], a['ratio'], a['accepted']) for a in i64['attempts']]}; slopes err/e_ref "
          f"{worst:.2f}; y(1) {err:.3e} from the fine grid, dopri5_64 {e64:.3e}, the fine grid's own error about "
          f"{float64_runs['self_consistency']:.1e}")
    assert float64_runs["self_consistency"] <= 1e-7
    assert err <= 4 * e64, label


# ------------------------------------------------------------------------- 4. a state above the block cap --
def test_state_above_the_norm_block_cap():
    """66 660 elements: 256 norm blocks of 261 elements, the last one of 105; sums, ratio and decision as above (no CPU
    oracle at this size)."""
    den, spec, job, _edge = setup("big", "f16x3")
    assert job.n_nodes * 3 == 66660 > 256 * 256
    drv = Driver(den, job, spec["x"], 0.0, 0.3)
    before, after = drv.attempt(1.0)
    re = check_sums("big", before, after)
    print(f"ode fp64 big: ratio {re['ratio_dev']:.6g}, {re['ratio_dev_vs_recomputed']:.4f} of n 2^-52 from the recomputation; "
          f"new h {re['dh']:.1f} x 2^-52 from the controller's")
    _setups.pop(("big", "f16x3", False))                    # 0.7 GB of edge state: not kept for the rest of the session


# ------------------------------------------------------------------------------ 5. fixed grids, slot by slot --
FIXED_GRIDS = {"linspace5": np.linspace(0.0, 1.0, 5).tolist(), "reverse5": np.linspace(1.0, 0.0, 5).tolist(),
               "uneven": [0.0, 0.3, 0.65, 1.0]}


@pytest.mark.parametrize("mode", ["f16x3", "f32"])
@pytest.mark.parametrize("grid", list(FIXED_GRIDS))
@pytest.mark.parametrize("method", ["euler", "midpoint", "rk4"])
@pytest.mark.parametrize("name", ["L20_B2", "n15"])
def test_fixed_grids_against_float64_slot_by_slot(name, method, grid, mode):
    """codlad_ode_loop against fixed64 over the float64 oracle field, every slot within 4 x max(e_ref, 5e-6) of its maximum,
    e_ref the fp32 CPU oracle loop's own distance (the rule of test_dpm_solver.py::test_order2_against_the_oracle; a case
    whose e_ref alone exceeded 2e-5 would be replaced, not given a wider bound)."""
    den, spec, job, edge = setup(name, mode)
    ts = FIXED_GRIDS[grid]
    traj, stats = den.sample_ode(job, spec["x"].to(DEV), ts, method=method, streams=1)
    assert stats["n_eval"] == (len(ts) - 1) * len(R.TABLEAUS[method][0])
    y64 = R.fixed64(oracle_field(spec, edge, torch.float64), spec["x"].double(), ts, method)
    y32 = oflow.odeint_fixed(oracle_field(spec, edge, torch.float32), spec["x"].float(), ts, method)
    assert torch.equal(traj[0].cpu(), spec["x"].float())
    figures = []
    for i in range(1, len(ts)):
        e_ref, err = R.rel_err(y32[i], y64[i]), R.rel_err(traj[i], y64[i])
        figures.append((err, e_ref))
    print(f"ode fp64 fixed {name} {method} {grid} {mode}: (device, e_ref) per slot " +
          ", ".join(f"({e:.2e}, {r:.2e})" for e, r in figures))
    for err, e_ref in figures:
        assert e_ref <= 2e-5, "the reference side alone is off: replace the case"
        assert err <= 4 * max(e_ref, 5e-6)


# ------------------------------------------------------------------ 6. the step-wise path on analytic fields --
def device_y0(y0):
    return y0.float().to(DEV)


@pytest.mark.parametrize("grid", list(FIXED_GRIDS))
@pytest.mark.parametrize("method", ["euler", "midpoint", "rk4"])
@pytest.mark.parametrize("name", list(R.ADAPTIVE))
def test_stepwise_fixed_grids_on_analytic_fields(name, method, grid):
    """A plain CUDA callable: ode._fixed_step and codlad_ode_combine as shipped, every slot within 4 x max(e32, 1e-6) of
    fixed64, e32 the numpy fp32 restatement's own distance."""
    cls, y0, _tol = R.ADAPTIVE[name]
    field, y0, ts = cls(), y0(), FIXED_GRIDS[grid]
    got = ode.odeint(field, device_y0(y0), ts, method=method)
    y64 = R.fixed64(field, y0, ts, method)
    y32 = R.fixed32(R.as_numpy_field(field), y0.float().numpy(), ts, method)
    figures = [(R.rel_err(got[i], y64[i]), R.rel_err(y32[i], y64[i])) for i in range(1, len(ts))]
    print(f"ode fp64 step-wise {name} {method} {grid}: (device, e32) per slot " + ", ".join(f"({e:.2e}, {r:.2e})" for e, r in figures))
    for err, e32 in figures:
        assert err <= 4 * max(e32, 1e-6)


@pytest.mark.parametrize("ts", R.ADAPTIVE_GRIDS, ids=["one_interval", "interior_time"])
@pytest.mark.parametrize("name", list(R.ADAPTIVE))
def test_stepwise_dopri5_on_analytic_fields(name, ts):
    """ode._dopri5 / _initial_step over codlad_ode_combine and a plain CUDA callable: dopri5_64's sequence of accepted and
    rejected steps and its n_eval (the ratio margins: tests/test_ode_ref_host.py), the final state within
    4 x max(e32, 1e-6)."""
    refs = R.adaptive_reference(name, ts)
    field, y0, tol, _y64, i64 = refs[:5]
    times = []

    def f(t, y):
        assert t.dtype == torch.float32 and y.is_cuda
        times.append(float(t))
        return field(t, y)

    got, stats = ode.odeint(f, device_y0(y0), ts, rtol=tol, atol=tol, method="dopri5", return_stats=True)
    assert stats == {"n_eval": i64["n_eval"], "n_accept": i64["n_accept"], "n_reject": i64["n_reject"]}
    R.check_against_dopri5_64(f"step-wise dopri5 {name} {ts}", times, got[-1], stats["n_eval"], refs)


@pytest.mark.parametrize("name", list(R.ADAPTIVE))
def test_initial_step_against_float64(name):
    cls, y0, tol = R.ADAPTIVE[name]
    field, y0 = cls(), y0()
    yd = device_y0(y0)
    got = ode._initial_step(field, 0.0, yd, field(0.0, yd), tol, tol)
    want = R.initial_step64(field, 0.0, y0, field(0.0, y0), tol, tol)
    print(f"ode fp64 initial step {name}: device {got!r}, float64 {want!r}, relative {abs(got - want) / want:.3e}")
    assert abs(got - want) <= 1e-5 * want
