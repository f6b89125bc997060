"""Guided sampling (denoised_fn / cond_fn, residue pinning): the cases of the g17 goldens and their deterministic hooks,
shared by the generator (tools/gen_golden.py, which runs the reference's own p_sample_loop_progressive with them on the
CPU) and the tests.  Inputs come from seeds (tests/cases.py); the hooks are plain torch, valid for both samplers.

Every case: T = 10 respaced from 1000, linear schedule, the seeded denoiser weights of cases.WEIGHT_SEED.
    name -> (n_cg, n_frames, seed, create_diffusion kwargs, clip_denoised, model, hooks)
model: "eps" = the 6-output diffusion model, "selfcond" = the same built with self_condition (its sampler feeds each step
the previous pred_xstart), "three" = the 3-output head (no variance channels) a fixed-variance sampler needs.
hooks: "pin" = PinLatents(pin_x0, pin_mask), "tanh" = 0.9 tanh(1.5 x), "cond" = PullToTarget, "cond+pin" = both.
"""
import torch

from codlad_amd import synth
from codlad_amd.diffusion_and_flow import PinLatents

T = 10
GUIDANCE_CASES = {
    "pin_eps_L46": (46, 2, 81, dict(), False, "eps", "pin"),
    "pin_clip_selfcond_L46": (46, 2, 82, dict(self_condition=True), True, "selfcond", "pin"),
    "pin_xstart_L87": (87, 1, 83, dict(predict_xstart=True), False, "eps", "pin"),
    "pin_fixed_small_L46": (46, 2, 84, dict(learn_sigma=False, sigma_small=True), False, "three", "pin"),
    "denoised_tanh_L46": (46, 2, 85, dict(), False, "eps", "tanh"),
    "cond_L46": (46, 2, 86, dict(), False, "eps", "cond"),
    "cond_fixed_large_L46": (46, 2, 87, dict(learn_sigma=False), False, "three", "cond"),
    "cond_pin_L87": (87, 1, 88, dict(), False, "eps", "cond+pin"),
}
# GPU tolerance of a case's trajectory against the reference's where it is not the default 2e-5 (with the measured reason)
GUIDANCE_TOL = {}
COND_SCALE = 1.5


def pin_inputs(n_cg, n_frames, seed):
    """Known latents and the pin mask of a case: x0 ~ 1.2 N(0, 1) (so that some entries lie outside [-1, 1], where
    clip_denoised acts on them after the pin), every fourth residue pinned, at a different phase in each frame."""
    x0 = synth.gaussian((n_frames, n_cg, 3), 9000 + seed) * 1.2
    r = torch.arange(n_cg)[None, :]
    f = torch.arange(n_frames)[:, None]
    return x0, (r + f) % 4 == 1


def tanh_denoised_fn(x):
    return 0.9 * torch.tanh(1.5 * x)


class PullToTarget:
    """cond_fn = s (target - x) t / 1000: a gradient that scales with the ORIGINAL-process timestep, so a sampler that
    handed it the respaced t (0..9 instead of 0..999) would be visibly off.  Takes the model's kwargs like the
    reference's cond_fn (y, mask, batch)."""

    def __init__(self, target, scale=COND_SCALE):
        self.target, self.scale = target, scale
        self.timesteps = []

    def __call__(self, x, t, y=None, mask=None, batch=None):
        assert mask is not None and batch is not None, "cond_fn receives the sampler's model_kwargs"
        self.timesteps.append(int(t.reshape(-1)[0]))
        tt = t.to(x.dtype).view(-1, *([1] * (x.dim() - 1))) / 1000.0
        return self.scale * (self.target.to(x.device) - x) * tt


def cond_target(n_cg, n_frames, seed):
    return synth.gaussian((n_frames, n_cg, 3), 9500 + seed) * 0.5


def hooks_for(name, device="cpu"):
    """(denoised_fn, cond_fn) of a case, on `device`."""
    L, B, seed, _kw, _clip, _model, hooks = GUIDANCE_CASES[name]
    denoised_fn = cond_fn = None
    if "pin" in hooks:
        x0, mask = pin_inputs(L, B, seed)
        denoised_fn = PinLatents(x0.to(device), mask.to(device))
    if hooks == "tanh":
        denoised_fn = tanh_denoised_fn
    if "cond" in hooks:
        cond_fn = PullToTarget(cond_target(L, B, seed).to(device))
    return denoised_fn, cond_fn
