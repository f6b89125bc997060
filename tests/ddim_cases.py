"""DDIM sampling and inversion: the cases of the g18 goldens, shared by the generator (tools/gen_golden.py, which runs the
reference's own p_mean_variance / condition_score / _predict_eps_from_xstart with them on the CPU and restates only the
DDIM update) and the tests.  Inputs come from seeds (tests/cases.py); the hooks are those of tests/guidance_cases.py.

Every case: T = 10 respaced from 1000 (`respacing`), linear schedule, the seeded denoiser weights of cases.WEIGHT_SEED.
    name -> (reverse, n_cg, n_frames, seed, respacing, create_diffusion kwargs, eta, clip_denoised, model, hooks)
reverse: False = ddim_sample_loop from x_T (z of cases.loop_noise), True = ddim_reverse_sample_loop from x_0 (that z).
model / hooks as in guidance_cases: "eps" (6 outputs), "selfcond", "three" (3-output head); "pin", "tanh", "cond",
"cond+pin" or None.
"""
from tests import guidance_cases as gc

T = 10
DDIM_CASES = {
    "fwd_L46": (False, 46, 2, 101, "10", dict(), 0.0, False, "eps", None),
    "fwd_eta1_L46": (False, 46, 2, 102, "10", dict(), 1.0, False, "eps", None),
    "fwd_selfcond_clip_eta05_L46": (False, 46, 2, 103, "10", dict(self_condition=True), 0.5, True, "selfcond", None),
    "fwd_xstart_L87": (False, 87, 1, 104, "10", dict(predict_xstart=True), 0.0, False, "eps", None),
    "fwd_fixed_small_L46": (False, 46, 2, 105, "10", dict(learn_sigma=False, sigma_small=True), 0.0, False, "three", None),
    "fwd_ddim10_L46": (False, 46, 2, 106, "ddim10", dict(), 0.0, False, "eps", None),
    "fwd_pin_L46": (False, 46, 2, 107, "10", dict(), 0.0, False, "eps", "pin"),
    "fwd_tanh_L46": (False, 46, 2, 108, "10", dict(), 0.0, False, "eps", "tanh"),
    "fwd_cond_L46": (False, 46, 2, 109, "10", dict(), 0.0, False, "eps", "cond"),
    "fwd_cond_pin_eta05_L87": (False, 87, 1, 110, "10", dict(), 0.5, False, "eps", "cond+pin"),
    "rev_L46": (True, 46, 2, 111, "10", dict(), 0.0, False, "eps", None),
    "rev_selfcond_L46": (True, 46, 2, 112, "10", dict(self_condition=True), 0.0, False, "selfcond", None),
    "rev_xstart_clip_L46": (True, 46, 2, 113, "10", dict(predict_xstart=True), 0.0, True, "eps", None),
    "rev_pin_L46": (True, 46, 2, 114, "10", dict(), 0.0, False, "eps", "pin"),
    "rev_cond_L46": (True, 46, 2, 115, "10", dict(), 0.0, False, "eps", "cond"),
}
# GPU tolerance of a case's trajectory against the reference's where it is not the default 2e-5 (with the measured reason)
# fwd_fixed_small_L46 / fwd_ddim10_L46: the denoiser FORWARD (f16x3, unchanged by DDIM) differs from the reference's by
# 4.9e-4 / 1.8e-3 of the output's max at two nodes of these inputs at their first step (2.4e-6 on fwd_L46's); the
# deterministic DDIM step carries that into the trajectory: 4.7e-4 / 3.5e-4 measured on both paths.
DDIM_TOL = {"fwd_fixed_small_L46": 1e-3, "fwd_ddim10_L46": 1e-3}


def hooks_for(name, device="cpu"):
    """(denoised_fn, cond_fn) of a case, on `device` (guidance_cases' hooks on this case's geometry and seed)."""
    _rev, L, B, seed, _resp, _kw, _eta, _clip, _model, hooks = DDIM_CASES[name]
    denoised_fn = cond_fn = None
    if hooks and "pin" in hooks:
        x0, mask = gc.pin_inputs(L, B, seed)
        denoised_fn = gc.PinLatents(x0.to(device), mask.to(device))
    if hooks == "tanh":
        denoised_fn = gc.tanh_denoised_fn
    if hooks and "cond" in hooks:
        cond_fn = gc.PullToTarget(gc.cond_target(L, B, seed).to(device))
    return denoised_fn, cond_fn
