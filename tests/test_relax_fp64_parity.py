"""The relaxation kernels (codlad_relax, codlad_relax_energy, csrc/relax_kernels.hip) against float64: per atom, per term and
per step, all through codlad_amd.metrics.

Rule 1 (tests/relax_cases.py, relax_ref.conditioning): everything in float64 from the float32 inputs the device is handed.
Every atom has a scale_a = 2^-24 (S_a + K_a) - the force magnitudes and the stiffness x length of the terms that touch it -
and every energy a scale_E; r_a = max_c |g[a, c] - g64[a, c]| / scale_a, E_ref = the numpy float32 restatement's largest r_a on
the same structure (0.05 to 0.86: tests/test_relax_cases_host.py).  Asserted, for every structure:
  free atoms  r_a <= 4 max(E_ref, 0.25)       fixed atoms  exactly 0       gmax == the device gradient's own maximum
  energies    |e - e64| <= 4 scale_E each; a class without a member is exactly 0.0
on the nine cases of tests/test_relax.py (whose pooled bound stays where it is) and on the designed cases.  One quad per
structure of `weight_threshold` lies within 2 float32 ulp of the weight threshold: there the device is held to the float64
result of one of the two weights, every other quad being in both.

The loop (rule 3) is teacher-forced from the device's own state: relax(n_iter = k) for k = 0 .. 24 gives every accepted
state x_k; each iteration's energy, gmax, trial, decision and next state are then held to float64 and to the stated update,
the trial and the next state bit for bit.

Figures of one run on an MI355X are in DESIGN.md, "The relaxation kernels against float64"."""
import numpy as np
import pytest
import torch

from codlad_amd import metrics
from tests import relax_cases as rc
from tests import relax_ref as rr
from tests import test_relax as tr

F32 = np.float32
cuda, bits = tr.cuda, tr.bits
SINGLE = [k for k in rc.CASES if k != "batch"]
TRACE_KEYS = ("trace_energy", "trial_energy", "step", "accepted", "gmax")


def evaluate(c, lo=0, hi=None):
    out = metrics.relax_energy_lists(cuda(c["xyz"][lo:hi]), c["radius"], c["bonds"], c["quads"], xyz0=cuda(c["xyz0"][lo:hi]),
                                     fixed=c["fixed"])
    S, n = c["xyz"][lo:hi].shape[:2]
    assert out["energy"].dtype == torch.float64 and out["energy"].shape == (S, 3) and out["grad"].shape == (S, n, 3)
    assert torch.equal(out["total"], (out["energy"][:, 0] + out["energy"][:, 1]) + out["energy"][:, 2])
    return out


def hold(name, c, out, lo=0):
    """Rule 1 on every structure of one evaluation -> (worst gradient figure, worst energy ratios [3], reference taken [S])."""
    e, g, gmax = out["energy"].cpu().numpy(), out["grad"].cpu().numpy(), out["gmax"].cpu().numpy()
    worst_g, worst_e, taken, failed = 0.0, np.zeros(3), [], []
    for k in range(len(e)):
        refs = c["refs"][lo + k]
        figs = [rc.judge(r, e[k], g[k]) for r in refs]
        ok = [rc.passes(f) for f in figs]
        pick = ok.index(True) if any(ok) else 0
        taken.append(pick)
        worst_g, worst_e = max(worst_g, figs[pick][0]), np.maximum(worst_e, figs[pick][1])
        if not any(ok):
            failed.append((lo + k, figs))
        assert not g[k][c["fixed"]].any(), (name, lo + k)
        assert gmax[k] == np.abs(g[k]).max(), (name, lo + k)
    print(f"{name}: worst r_a / max(E_ref, 0.25) {worst_g:.3f} (bound 4), energies / scale_E {np.round(worst_e, 3)} (bound 4)")
    assert not failed, (name, failed)
    return worst_g, worst_e, taken


# ------------------------------------------------------------------------------------------- rule 1: one evaluation
@pytest.mark.gpu
@pytest.mark.parametrize("n", tr.SIZES)
def test_cases_of_the_pooled_test_per_atom_and_per_term(n):
    c = rc.existing(n)
    hold(f"case({n})", c, evaluate(c))


@pytest.mark.gpu
@pytest.mark.parametrize("name", SINGLE)
def test_designed_case_per_atom_and_per_term(name):
    c = rc.get(name)
    out = evaluate(c)
    _g, _e, taken = hold(name, c, out)
    e, g = out["energy"].cpu().numpy(), out["grad"].cpu().numpy()
    if name == "tiny_n1":
        assert not e.any() and not g.any() and not out["gmax"].cpu().numpy().any()
    if name == "many_quads_0":
        assert not e[:, 1].any()
    if name == "start":
        assert not e[:, :2].any() and (e[:, 2] > 0).all()                   # the restraint terms are exactly 0 at the start
        for s in range(3):
            assert not g[s][~c["refs"][s][0]["contact"]].any(), s
    if name == "weight_threshold":
        und = [s for s, u in enumerate(c["undecided"]) if u is not None]
        print(f"weight_threshold: {len(und)} undecided quads, the device's weights {[taken[s] for s in und]}")
        assert all(taken[s] == 0 for s in range(3) if c["undecided"][s] is None)


# ---------------------------------------------------------------------------------------------------------- batch
@pytest.mark.gpu
@pytest.mark.parametrize("S", rc.BATCH_SIZES)
def test_batch_evaluation_reaches_every_block_of_the_finish_kernel(S):
    c = rc.get("batch")
    out = evaluate(c, 0, S)
    hold(f"batch S={S}", c, out)
    for s in rc.BATCH_ALONE(S):
        one = evaluate(c, s, s + 1)
        for k in ("energy", "grad", "gmax", "total"):
            assert torch.equal(bits(one[k][0]), bits(out[k][s])), (k, s)


@pytest.mark.gpu
@pytest.mark.parametrize("S", rc.BATCH_SIZES)
def test_batch_loop_is_each_structure_alone(S):
    c, n_iter = rc.get("batch"), rc.BATCH_ITER
    x = cuda(c["xyz_loop"][:S])
    out = metrics.relax_lists(x, c["radius"], c["bonds"], c["quads"], n_iter=n_iter)
    tr.check_rule(out, n_iter)
    assert out["xyz"].shape == (S, rc.BATCH_N, 3) and out["converged"].shape == (S,) and out["converged"].dtype == torch.uint8
    planted = [s in rc.BATCH_PLANTED for s in range(S)]
    assert out["converged"].tolist() == [int(not p) for p in planted]
    assert (out["accepted"].sum(1) > 0).tolist() == planted
    clean = [s for s in range(S) if not planted[s]]
    assert torch.equal(bits(out["xyz"][clean]), bits(x[clean])) and not out["trace_energy"][clean].any()
    for s in rc.BATCH_ALONE(S):
        one = metrics.relax_lists(x[s:s + 1], c["radius"], c["bonds"], c["quads"], n_iter=n_iter)
        for k in TRACE_KEYS + ("xyz", "converged"):
            assert torch.equal(bits(one[k][0]), bits(out[k][s])), (k, s)


# ---------------------------------------------------------------------------------- rule 3: the loop, step by step
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["r32", "c257"])
def test_loop_per_step_from_the_device_state(name):
    r, K = rc.loop_runs()[name], rc.LOOP_K
    T, fixed, x_np = r["T"], r["fixed"], r["xyz"]
    x_in = cuda(x_np)
    S = len(x_np)
    if name == "r32":
        top = r["planted"]["top"]
        relax = lambda k: metrics.relax(x_in, top, n_iter=k)                                                   # noqa: E731
        energy = lambda x: metrics.relax_energy(x, top, xyz0=x_in)                                             # noqa: E731
    else:
        c = r["case"]
        relax = lambda k: metrics.relax_lists(x_in, c["radius"], c["bonds"], c["quads"], fixed=fixed, n_iter=k,  # noqa: E731
                                              **r["constants"])
        energy = lambda x: metrics.relax_energy_lists(x, c["radius"], c["bonds"], c["quads"], xyz0=x_in, fixed=fixed)  # noqa: E731
    h = {**rr.DEFAULTS, **r["constants"]}
    runs = [relax(k) for k in range(K + 1)]
    full = runs[K]
    tr.check_rule(full, K, h["h0"], h["h_max"])
    for k in range(K + 1):                                                   # prefix: a shorter run is the start of a longer one
        tr.check_rule(runs[k], k, h["h0"], h["h_max"])
        for key in TRACE_KEYS:
            assert torch.equal(bits(runs[k][key]), bits(full[key][:, :k + (key == "trace_energy")])), (key, k)
    assert torch.equal(bits(runs[0]["xyz"]), bits(x_in))
    e_tr, e_trial = full["trace_energy"].cpu().numpy(), full["trial_energy"].cpu().numpy()
    step, gmax, acc = full["step"].cpu().numpy(), full["gmax"].cpu().numpy(), full["accepted"].cpu().numpy().astype(bool)
    total = lambda ref: float((ref["e"][0] + ref["e"][1]) + ref["e"][2])                                       # noqa: E731
    bound_e = lambda ref: float(rc.FACTOR * ref["scale_E"].sum())                                              # noqa: E731
    close = np.zeros(S, dtype=int)
    worst = dict(energy=0.0, trial=0.0, gmax=0.0)
    for k in range(K):
        xk_t = runs[k]["xyz"]
        xk = xk_t.cpu().numpy()
        ev = energy(xk_t)
        assert torch.equal(bits(ev["total"]), bits(full["trace_energy"][:, k])), k          # the loop runs the entry point's kernel
        assert torch.equal(bits(ev["gmax"]), bits(full["gmax"][:, k])), k
        g = ev["grad"].cpu().numpy()
        move = gmax[:, k] > 0
        scale = np.where(move, step[:, k] / np.where(move, gmax[:, k], F32(1)), F32(0)).astype(F32)          # fl32(h / gmax)
        trial = (xk - (scale[:, None, None] * g).astype(F32)).astype(F32)                    # one multiply, one subtract
        ev_t = energy(cuda(trial))
        assert torch.equal(bits(ev_t["total"]), bits(full["trial_energy"][:, k])), k
        nxt = runs[k + 1]["xyz"].cpu().numpy()
        for s in range(S):
            ref_k = rc.structure_ref(xk[s], x_np[s], T, fixed)
            ref_t = rc.structure_ref(trial[s], x_np[s], T, fixed)
            bk, bt = bound_e(ref_k), bound_e(ref_t)
            assert abs(e_tr[s, k] - total(ref_k)) <= bk, (k, s, e_tr[s, k], total(ref_k), bk)
            assert abs(e_trial[s, k] - total(ref_t)) <= bt, (k, s, e_trial[s, k], total(ref_t), bt)
            worst["energy"] = max(worst["energy"], abs(e_tr[s, k] - total(ref_k)) / bk * rc.FACTOR)
            worst["trial"] = max(worst["trial"], abs(e_trial[s, k] - total(ref_t)) / bt * rc.FACTOR)
            g_abs = np.abs(ref_k["g"]).max(-1)
            lo, hi = float((g_abs - ref_k["bound"]).max()), float((g_abs + ref_k["bound"]).max())
            assert lo <= gmax[s, k] <= hi, (k, s, lo, gmax[s, k], hi)
            a = int(np.argmax(g_abs))
            worst["gmax"] = max(worst["gmax"], abs(gmax[s, k] - g_abs[a]) / ref_k["bound"][a] * rc.FACTOR)
            if abs(total(ref_t) - total(ref_k)) > bk + bt:
                assert acc[s, k] == (total(ref_t) < total(ref_k)), (k, s)
            else:
                close[s] += 1
            want = trial[s] if acc[s, k] else xk[s]
            assert np.array_equal(nxt[s].view(np.int32), want.view(np.int32)), (k, s)
    print(f"{name}: {K} iterations x {S} structures, rejected {(~acc).sum(1).tolist()}, decisions inside the energy bounds "
          f"{close.tolist()}; worst |E - E64| {worst['energy']:.3f}, trial {worst['trial']:.3f}, gmax {worst['gmax']:.3f} "
          f"of the unit their bound is 4 of")
    assert (close <= K // 10).all()
    assert (~acc).sum() > 0
