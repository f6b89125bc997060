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
# GPU tolerance of a case's trajectory against the reference's where it is not the default 2e-5, with the cause.
#
# Both exceptions come from ONE pair of edges each, between two neighbouring residues of frame 1 whose local frames are
# partly zeroed (a CA step outside the 3.6-4.0 A window): R = O_i^T O_j is then symmetric with trace -1 in exact
# arithmetic, so all three sign arguments s_k are exactly 0 and 1 + trace(R) is pure rounding noise.  The reference's
# quaternion is normalize(0, 0, 0, sqrt(relu(1 + trace R)) / 2): (0, 0, 0, 1) if the noise came out positive, the zero
# quaternion if not - a jump of 0.2 of h_E0's maximum in that edge's row.  tests/conditioning.py calls all four edges
# ill-conditioned (|1 + trace R| < 1e-3).  Established on the CPU and on MI355X (all three contraction modes alike):
#
# fwd_fixed_small_L46 (seed 105, t 999): edges 29 <-> 30 of frame 1.  float64: 1 + trace R = 0, zero quaternion; the
#   device: the same (its rows are within 1.4e-5 of float64 on every ill-conditioned edge); the REFERENCE's fp32 gets a
#   positive noise value and (0, 0, 0, 1): its h_E0 rows are 0.20 / 0.23 of the maximum from float64 there and its
#   forward 4.9e-4 / 3.9e-4 of the output's maximum from the float64 forward at nodes 76 / 75 (4.9e-5 next, median
#   2.8e-6).  The golden carries the reference's rounding, not an error of the kernels.
# fwd_ddim10_L46 (seed 106, t 900): edges 12 <-> 13 of frame 1.  float64: 1 + trace R = 2.2e-16, (0, 0, 0, 1), and so the
#   reference's fp32 (its forward is within 1.3e-5 of float64 at every node); the device's fp32 evaluation of the same
#   formula gets a value <= 0 and the zero quaternion: its two rows equal the float64 rows recomputed with the zero
#   quaternion to 2.6e-7 of the maximum, and the float64 forward from the device's features differs from the plain
#   float64 forward by 1.8e-3 / 1.0e-3 at nodes 59 / 58 (6.5e-5 next, median 4e-8) - the whole of the deviation.
#   These are the edges of FEATURE_DISCONTINUITY_EDGES below, which test_features_prepass_edge_by_edge admits as "the
#   reference's discontinuity taken the other way" and nothing else.
#
# Everything after the features meets the tight per-node bound against float64 on both inputs, in every mode and with
# the large-job kernels (tests/test_fp64_parity.py: at most 2.6 x the fp32 oracle's own error, bound 4 / 16).  The
# deterministic DDIM step carries the first-step difference into the trajectory: 4.7e-4 / 3.5e-4 measured on both paths.
DDIM_TOL = {"fwd_fixed_small_L46": 1e-3, "fwd_ddim10_L46": 1e-3}
# geometry -> (frame, node, neighbour) of the edges where the device takes a discontinuity of the reference's quaternion
# the other way than float64 does (see above); an edge that is not listed here must meet the ordinary per-edge bounds
FEATURE_DISCONTINUITY_EDGES = {"fwd_ddim10_L46": ((1, 12, 13), (1, 13, 12))}


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
