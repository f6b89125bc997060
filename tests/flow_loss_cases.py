"""Flow-matching loss evaluation: the cases of the g20 goldens, shared by the generator (tools/gen_golden.py, which runs the
reference's own diffusion_and_flow.flow matchers, its flow model and utils.train_module.loss_fn with them on the CPU) and
the tests.  Inputs come from seeds (tests/cases.py); the goldens hold the reference's outputs and the noise it drew.

Geometries: cases.FLOW_CASES' L46_B2 (seed 12) and L87_B2 (seed 13), which g12 already runs clear of the reference's
quaternion discontinuity; the generator asserts it with tests/conditioning.py's edge quantities, as g19 does.

FM_CASES: name -> (geometry, matcher kind, sigma, n_rep, times)
  n_rep: the batch of the geometry's frames is repeated n_rep times along the sample axis (as loss_cases does), so that
  four times fit on two frames; times: one per sample, or a single shared time.
SWEEP_CASES: name -> (geometry, matcher kind, sigma, times): one noise draw per time, every time shared by the samples.
"""
import numpy as np
import torch

from codlad_amd import synth
from tests import cases

GEOMETRIES = {"L46_B2": (46, 2, 12), "L87_B2": (87, 2, 13)}
TIMES4 = (0.12, 0.37, 0.5, 0.93)
FM_CASES = {
    "icfm_s0_L46": ("L46_B2", "icfm", 0.0, 2, TIMES4),
    "icfm_s01_L87": ("L87_B2", "icfm", 0.1, 1, (0.37,)),
    "target_s0_L87": ("L87_B2", "target", 0.0, 1, (0.5,)),
    "target_s01_L46": ("L46_B2", "target", 0.1, 2, TIMES4),
    "vp_s0_L46": ("L46_B2", "vp", 0.0, 2, TIMES4),
}
SWEEP_CASES = {"sweep_icfm_L46": ("L46_B2", "icfm", 0.1, (0.25, 0.5, 0.75))}
LOSS_TYPES = ("l2", "l1", "huber", "smooth_l1", "log_cosh")
REF_MATCHER = {"icfm": "ConditionalFlowMatcher", "target": "TargetConditionalFlowMatcher",
               "vp": "VariancePreservingConditionalFlowMatcher"}

# Bounds.  ref_dev (in every golden, float64 [7]: the five loss types in LOSS_TYPES' order, then VP's xt and ut) is the
# reference's OWN fp32-against-float64 deviation, the class-wide maximum over the g20 cases (the rule of
# tests/loss_cases.py):
#   loss types  relative, per sample: |f32 - f64| / |f64| of loss_fn on the fp32 model output against loss_fn on its
#               .double(), both the reference's code;
#   VP xt, ut   relative to the quantity's largest magnitude in the case: max |f32 - f64| / max |f64| of the matcher run on
#               fp32 tensors against the same matcher on their .double() (an element next to a zero crossing has no
#               relative accuracy of its own in either arithmetic: cos and sin of the fp32 product h t carry an absolute
#               error of the order of an ulp of 1).
# The kernel-level tests allow REF_DEV_FACTOR x ref_dev.  The device's measured deviation is printed by the tests before
# they assert.
REF_DEV_FACTOR = 4.0
REF_DEV_INDEX = {k: i for i, k in enumerate(LOSS_TYPES + ("vp_xt", "vp_ut"))}
# the end-to-end allowance of tests/test_losses.py: the forward's error bound relative to the output's maximum
FORWARD_BOUND = 1e-5


def inputs(geometry, n_rep, n_steps=1):
    """prot, batch (randn repeated as the reference's doubled batches), mask [N, L], x0, x1 [N, L, 3]; N = B * n_rep."""
    L, B, seed = GEOMETRIES[geometry]
    prot, batch, _x, _t, mask = cases.denoiser_inputs(L, B, seed)
    N = B * n_rep
    batch = dict(batch)
    batch["randn"] = torch.cat([batch["randn"]] * n_rep)
    mask = torch.cat([mask] * n_rep)
    x1 = synth.gaussian((N, L, 3), 7000 + seed)
    x0 = synth.gaussian((N, L, 3), 7500 + seed)
    return prot, batch, mask, x0, x1


def times(case_times, N):
    """The case's times as fp32 [N]."""
    t = case_times * N if len(case_times) == 1 else case_times
    assert len(t) == N
    return torch.tensor(t, dtype=torch.float64).float()


def noise_seed(name):
    """The seed of the generator's torch.manual_seed before the reference draws the case's noise (stored in the golden)."""
    return 20000 + sorted(list(FM_CASES) + list(SWEEP_CASES)).index(name)


def load(name):
    return np.load(cases.npz_path(f"g20_flow_loss_{name}"))
