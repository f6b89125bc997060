"""Drop-in for the reference's `diffusion_and_flow.create_diffusion` (sampling and forward-only loss evaluation).

Same call surface as the reference (`diffusion_and_flow/__init__.py:10-60`): the returned object has
`.p_sample_loop(model, shape, noise, clip_denoised, denoised_fn, cond_fn, model_kwargs, device,
progress)`, `.p_sample_loop_progressive`, `.p_sample`, the schedule tables and `timestep_map`.
The arithmetic is on the GPU: when `model` is the forward of a codlad_amd `ProteinMPNN_diffusion_new`
the whole loop is one `codlad_sample_loop` call; any other CUDA callable is stepped with
`codlad_ddpm_update`.  The reference's hooks are honoured: `denoised_fn` rewrites the x_0 prediction before the
clamp and `cond_fn` adds variance * gradient to the posterior mean (gaussian_diffusion.py:335-349, 374-384); a
`PinLatents` denoised_fn on the HIP model without cond_fn is fused into the loop (`codlad_sample_loop_pinned`), any
other callable runs between the two halves of the split step (`codlad_ddpm_pred_xstart` /
`codlad_ddpm_posterior_step`).  DDIM (the IDDPM release's `ddim_sample`, `ddim_reverse_sample`, `ddim_sample_loop`,
`ddim_sample_loop_progressive`, with `eta`; `ddim_reverse_sample_loop` returns x_T) follows the same rule: the loop is
one `codlad_ddim_loop` call for the HIP model with no hook or only a `PinLatents`, any other case steps through the
model and `codlad_ddpm_pred_xstart` / `codlad_ddim_step`.  DPM-Solver++(2M) (`dpm_solver_sample_loop`,
`dpm_solver_sample_loop_progressive`, `order` 1 or 2; Lu et al. 2022 - not in the reference) follows it too:
`codlad_dpm_loop`, or the model and `codlad_ddpm_pred_xstart` / `codlad_dpm_step` per step; the respacing spec "logsnrN"
(steps uniform in log-SNR) is the spacing it is meant for.  The forward process and the losses (`q_mean_variance`,
`q_sample`, `q_posterior_mean_variance`, `_vb_terms_bpd`, `training_losses`, and the IDDPM release's `calc_bpd_loop`) are
evaluated forward-only: the HIP model runs `codlad_loss_forward` per group of equal timesteps and `codlad_bpd_loop` for the
whole bound, any other CUDA callable is followed by `codlad_vb_terms`.  Gradients and training are out of scope; forward-only
loss evaluation is built - for the flow-matching models in `flow.py` (the reference's matchers, `training_losses`,
`loss_sweep`), which takes the same two paths.
"""
import enum
import random

import torch

from .schedule import Tables, logsnr_timesteps, named_betas, space_timesteps


class ModelMeanType(enum.Enum):
    PREVIOUS_X = enum.auto()
    START_X = enum.auto()
    EPSILON = enum.auto()


class ModelVarType(enum.Enum):
    LEARNED = enum.auto()
    FIXED_SMALL = enum.auto()
    FIXED_LARGE = enum.auto()
    LEARNED_RANGE = enum.auto()


class LossType(enum.Enum):
    MSE = enum.auto()            # raw MSE (and the vb term when the variance is learned)
    RESCALED_MSE = enum.auto()   # raw MSE, the vb term scaled by T / 1000
    KL = enum.auto()             # the variational bound
    RESCALED_KL = enum.auto()    # like KL, times T: an estimate of the full bound

    def is_vb(self):
        return self in (LossType.KL, LossType.RESCALED_KL)


class PinLatents:
    """Residue pinning as a `denoised_fn`: the x_0 prediction of the residues where `mask` is set is replaced by the known
    latents `x0` at every step, so they end the loop on them (unless clip_denoised clamps them) and the other residues
    are sampled conditioned on them.  An ordinary callable, `torch.where(mask[..., None], x0, x)`, so it is a valid
    denoised_fn for the reference's sampler too; given to `p_sample_loop` with the codlad_amd model and no cond_fn it
    runs fused into the loop.  x0 [N, L, C] floating point (the sampler's normalised latent space), mask [N, L] bool."""

    def __init__(self, x0, mask):
        if not isinstance(x0, torch.Tensor) or not x0.is_floating_point():
            raise TypeError(f"PinLatents: x0 must be a floating-point tensor, got "
                            f"{x0.dtype if isinstance(x0, torch.Tensor) else type(x0).__name__}")
        if not isinstance(mask, torch.Tensor) or mask.dtype != torch.bool:
            raise TypeError(f"PinLatents: mask must be a bool tensor, got "
                            f"{mask.dtype if isinstance(mask, torch.Tensor) else type(mask).__name__}")
        if x0.dim() < 2 or tuple(mask.shape) != tuple(x0.shape[:-1]):
            raise ValueError(f"PinLatents: mask must have the shape of x0 without its channel axis: x0 {tuple(x0.shape)}, "
                             f"mask {tuple(mask.shape)}")
        if x0.device != mask.device:
            raise ValueError(f"PinLatents: x0 ({x0.device}) and mask ({mask.device}) are on different devices")
        self.x0, self.mask = x0, mask

    def __call__(self, x):
        if tuple(x.shape) != tuple(self.x0.shape):
            raise ValueError(f"PinLatents: pred_xstart {tuple(x.shape)} does not match x0 {tuple(self.x0.shape)}")
        return torch.where(self.mask[..., None], self.x0, x)


def _check_hook_output(v, x, what):
    if not isinstance(v, torch.Tensor) or tuple(v.shape) != tuple(x.shape) or not v.is_floating_point() or not v.is_cuda:
        desc = f"{v.dtype} {tuple(v.shape)} on {v.device}" if isinstance(v, torch.Tensor) else type(v).__name__
        raise ValueError(f"{what} must return a floating-point CUDA tensor of the sample's shape {tuple(x.shape)}, got {desc}")


# -- forward process and losses (forward-only) ---------------------------------------------------
def _flat3(x, what):
    """[N, L, 3] latents -> ([N * L, 3], nodes per sample); the refusals every loss entry point shares."""
    if not x.is_cuda:
        raise RuntimeError(f"{what} (codlad_amd) runs on the MI355X only")
    if x.dim() != 3 or x.shape[-1] != 3:
        raise NotImplementedError(f"{what}: latents [N, L, 3] only (the reference's angle wrap for a channel width of 2 is "
                                  f"not built), got {tuple(x.shape)}")
    return x.reshape(-1, 3), [int(x.shape[1])] * int(x.shape[0])


class _LossEvaluation:
    """The forward process and the forward-only losses of SpacedDiffusion (its second base class)."""

    def loss_coefs(self, clip_denoised):
        """The [T, 16] table of the loss kernels for this diffusion's branches (schedule.Tables.loss_coefficients)."""
        cache = self.__dict__.setdefault("_loss_tables", {})
        key = bool(clip_denoised)
        if key not in cache:
            var = {ModelVarType.FIXED_SMALL: "fixed_small",
                   ModelVarType.FIXED_LARGE: "fixed_large"}.get(self.model_var_type, "learned_range")
            cache[key] = self.loss_coefficients(predict_xstart=self.model_mean_type is ModelMeanType.START_X, var_type=var,
                                                clip_denoised=key)
        return cache[key]

    def q_mean_variance(self, x_start, t):
        """q(x_t | x_0): (mean, variance, log_variance), each of x_start's shape (gaussian_diffusion.py:211-221)."""
        from ..engine import Denoiser
        flat, lens = _flat3(x_start, "q_mean_variance")
        return tuple(v.view(x_start.shape) for v in Denoiser.q_affine("q_sample", flat, None, lens, t, self.loss_coefs(False)))

    def q_sample(self, x_start, t, noise=None):
        """A sample of q(x_t | x_0) (gaussian_diffusion.py:223-238); t [N] int64, values may differ per sample."""
        from ..engine import Denoiser
        flat, lens = _flat3(x_start, "q_sample")
        if noise is None:
            noise = torch.randn_like(x_start)
        if tuple(noise.shape) != tuple(x_start.shape):
            raise ValueError(f"q_sample: noise {tuple(noise.shape)} does not match x_start {tuple(x_start.shape)}")
        return Denoiser.q_affine("q_sample", flat, noise.reshape(-1, 3), lens, t, self.loss_coefs(False))[0].view(x_start.shape)

    def q_posterior_mean_variance(self, x_start, x_t, t):
        """q(x_{t-1} | x_t, x_0): (mean, variance, log_variance clipped) (gaussian_diffusion.py:240-260)."""
        from ..engine import Denoiser
        flat, lens = _flat3(x_start, "q_posterior_mean_variance")
        if tuple(x_t.shape) != tuple(x_start.shape):
            raise ValueError(f"q_posterior_mean_variance: x_t {tuple(x_t.shape)} does not match x_start {tuple(x_start.shape)}")
        return tuple(v.view(x_start.shape)
                     for v in Denoiser.q_affine("q_posterior", flat, x_t.reshape(-1, 3), lens, t, self.loss_coefs(False)))

    def _map_t(self, t):
        return torch.tensor(self.timestep_map, device=t.device, dtype=t.dtype)[t]          # respace.py:124-129

    def _loss_terms(self, model, x_start, x_t, t, noise, clip_denoised, model_kwargs, x_self_cond=None):
        """The loss kernels' terms for model(x_t, t): the HIP model through codlad_loss_forward (grouped by timestep), any
        other callable through its output and codlad_vb_terms."""
        from ..engine import Denoiser
        flat, lens = _flat3(x_start, "the loss evaluation")
        coef = self.loss_coefs(clip_denoised)
        mod = self._hip_module(model)
        nz = None if noise is None else noise.reshape(-1, 3)
        if mod is not None:
            job, _pin = self._fused_job(mod, x_start, model_kwargs, None)
            sc = None if x_self_cond is None else x_self_cond.reshape(-1, 3)
            return mod.engine().loss_terms(job, flat, t, nz, self, coef=coef, x_t=x_t.reshape(-1, 3), x_self_cond=sc)
        kwargs = dict(model_kwargs)
        if self.self_condition:
            kwargs["x_self_cond"] = x_self_cond
        model_out = model(x_t, self._map_t(t), **kwargs)
        width = 3 if self.fixed_variance else 6
        if not isinstance(model_out, torch.Tensor) or tuple(model_out.shape) != tuple(x_start.shape[:-1]) + (width,):
            raise ValueError(f"the model must return a tensor {tuple(x_start.shape[:-1]) + (width,)} (a fixed-variance "
                             "diffusion takes a model without variance channels)")
        return Denoiser.vb_terms(model_out.reshape(-1, width), flat, x_t.reshape(-1, 3), nz, lens, t, coef)

    def _vb_terms_bpd(self, model, x_start, x_t, t, clip_denoised=True, model_kwargs=None):
        """One term of the variational bound in bits per dimension: {"output": [N] (the decoder NLL where t == 0, else the
        KL), "pred_xstart"} (gaussian_diffusion.py:549-596).  Unlike the reference, whose own call drops model_kwargs and
        so cannot run with this model, the model receives model_kwargs."""
        r = self._loss_terms(model, x_start, x_t, t, None, clip_denoised, dict(model_kwargs or {}))
        return {"output": r["vb"], "pred_xstart": r["pred_xstart"].view(x_start.shape)}

    def training_losses(self, model, x_start, t, model_kwargs=None, noise=None):
        """The training losses of one batch, forward-only (gaussian_diffusion.py:598-725): {"loss", "mse" [N], and "vb" for
        a learned variance}; t [N] int64 may differ per sample.  RESCALED_MSE scales vb by T / 1000, RESCALED_KL the loss
        by T.  A self-conditioned diffusion draws `random() < 0.5` from Python's global `random` where the reference does.
        KL / RESCALED_KL: the vb term is computed from the model's actual output on (x_t, t, **model_kwargs); the
        reference's own path for them hands model_kwargs=None to the model and cannot run with this model."""
        _flat3(x_start, "training_losses")
        if not isinstance(self.loss_type, LossType):
            raise NotImplementedError(self.loss_type)
        model_kwargs = dict(model_kwargs or {})
        model_kwargs.pop("epoch", None)
        if noise is None:
            noise = torch.randn_like(x_start)
        x_t = self.q_sample(x_start, t, noise=noise)
        x_self_cond = None
        if self.self_condition and random.random() < 0.5 and not self.loss_type.is_vb():
            x_self_cond = self._loss_terms(model, x_start, x_t, t, None, False, model_kwargs)["pred_xstart"].view(x_start.shape)
        r = self._loss_terms(model, x_start, x_t, t, noise, False, model_kwargs, x_self_cond=x_self_cond)
        terms = {}
        if self.loss_type.is_vb():
            terms["loss"] = r["vb"] * self.num_timesteps if self.loss_type is LossType.RESCALED_KL else r["vb"]
            return terms
        terms["mse"] = r["mse"]
        if not self.fixed_variance:
            terms["vb"] = r["vb"] * (self.num_timesteps / 1000.0) if self.loss_type is LossType.RESCALED_MSE else r["vb"]
            terms["loss"] = terms["mse"] + terms["vb"]
        else:
            terms["loss"] = terms["mse"]
        return terms

    def calc_bpd_loop(self, model, x_start, clip_denoised=True, model_kwargs=None, step_noise=None):
        """The whole variational bound in bits per dimension (the IDDPM release's calc_bpd_loop): {"total_bpd", "prior_bpd"
        [N]; "vb", "xstart_mse", "mse" [N, T], column k = step T-1-k, the order the loop visits them}.  One
        codlad_bpd_loop call when `model` is the HIP model's forward; `step_noise` [T, *x_start.shape] optionally gives
        the per-step noise (loop order) instead of T draws of randn_like(x_start)."""
        from ..engine import Denoiser
        flat, lens = _flat3(x_start, "calc_bpd_loop")
        model_kwargs = dict(model_kwargs or {})
        T = self.num_timesteps
        eps = step_noise if step_noise is not None else self._draw_noise(x_start)
        if tuple(eps.shape) != (T,) + tuple(x_start.shape):
            raise ValueError(f"step_noise must be [T, *x_start.shape] = {(T,) + tuple(x_start.shape)}, got {tuple(eps.shape)}")
        layout = lambda a: a.flip(0).t().contiguous()                      # noqa: E731  [T, N] by step -> [N, T] in loop order
        mod = self._hip_module(model)
        if mod is not None:
            job, _pin = self._fused_job(mod, x_start, model_kwargs, None)
            r = mod.engine().bpd(job, flat, eps.reshape(T, -1, 3), self, coef=self.loss_coefs(clip_denoised))
            return {"total_bpd": r["total_bpd"], "prior_bpd": r["prior_bpd"], "vb": layout(r["vb"]),
                    "xstart_mse": layout(r["xstart_mse"]), "mse": layout(r["mse"])}
        from .. import _lib
        import numpy as np
        rows = {"vb": [], "xstart_mse": [], "eps_mse": []}
        for k, i in enumerate(range(T - 1, -1, -1)):
            t = torch.full((x_start.shape[0],), i, device=x_start.device, dtype=torch.int64)
            x_t = self.q_sample(x_start, t, noise=eps[k])
            r = self._loss_terms(model, x_start, x_t, t, eps[k], clip_denoised, model_kwargs)
            for key in rows:
                rows[key].append(r[key])
        coef = torch.from_numpy(np.ascontiguousarray(self.loss_coefs(clip_denoised))).to(x_start.device)
        prior = torch.empty(len(lens), dtype=torch.float32, device=x_start.device)
        rc = _lib.lib().codlad_prior_bpd(_lib.ptr(flat.contiguous().float()), _lib.ptr(coef), T,
                                         _lib.ptr(Denoiser.sample_offsets(lens, x_start.device)), len(lens), _lib.ptr(prior),
                                         _lib.stream_ptr(x_start.device))
        _lib.check(rc, "codlad_prior_bpd")
        vb = torch.stack(rows["vb"], dim=1)
        return {"total_bpd": vb.sum(dim=1) + prior, "prior_bpd": prior, "vb": vb,
                "xstart_mse": torch.stack(rows["xstart_mse"], dim=1), "mse": torch.stack(rows["eps_mse"], dim=1)}


class SpacedDiffusion(_LossEvaluation, Tables):
    """Respaced ancestral sampler (reference respace.py:65-114 + gaussian_diffusion.py:404-547) with every branch of
    p_mean_variance that `create_diffusion` can select (gaussian_diffusion.py:303-349): the model predicts the noise
    (EPSILON, the default) or x_0 (START_X, test.py --predict_xstart); the variance is the learned range
    (LEARNED_RANGE; LEARNED takes the same formula in the reference) or fixed (FIXED_SMALL / FIXED_LARGE, with a
    model whose head has no variance channels); pred_xstart is optionally clipped into [-1, 1] (clip_denoised).
    denoised_fn / cond_fn as in the reference (see the module docstring)."""

    def __init__(self, use_timesteps, betas, model_mean_type=ModelMeanType.EPSILON,
                 model_var_type=ModelVarType.LEARNED_RANGE, loss_type=None, self_condition=False):
        if model_mean_type is ModelMeanType.PREVIOUS_X:
            raise NotImplementedError("ModelMeanType.PREVIOUS_X: create_diffusion never selects it and the reference's "
                                      "p_mean_variance has no branch for it either (gaussian_diffusion.py:343-349)")
        super().__init__(betas, set(use_timesteps))
        self.use_timesteps = set(use_timesteps)
        self.original_num_steps = len(betas)
        self.model_mean_type, self.model_var_type = model_mean_type, model_var_type
        # reference gaussian_diffusion.py:172, 530-547: each step is conditioned on the previous pred_xstart
        self.loss_type, self.self_condition = loss_type, bool(self_condition)

    @property
    def fixed_variance(self):
        return self.model_var_type in (ModelVarType.FIXED_SMALL, ModelVarType.FIXED_LARGE)

    def coefficients(self, clip_denoised):
        """The [T, 8] step table of the kernels for this sampler's branches (schedule.Tables.step_coefficients)."""
        var = {ModelVarType.FIXED_SMALL: "fixed_small", ModelVarType.FIXED_LARGE: "fixed_large"}.get(self.model_var_type,
                                                                                                      "learned_range")
        return self.step_coefficients(predict_xstart=self.model_mean_type is ModelMeanType.START_X, var_type=var,
                                      clip_denoised=bool(clip_denoised))

    def fixed_variances(self):
        """[T] fp32 table variance of a fixed-variance sampler (the factor of cond_fn's gradient; zeros otherwise)."""
        var = {ModelVarType.FIXED_SMALL: "fixed_small", ModelVarType.FIXED_LARGE: "fixed_large"}.get(self.model_var_type,
                                                                                                      "learned_range")
        return self.step_variances(var)

    def ddim_coefs(self, clip_denoised, eta=0.0, reverse=False):
        """The [T, 8] DDIM table of the kernels for this sampler's branches (schedule.Tables.ddim_coefficients)."""
        key = (bool(clip_denoised), float(eta), bool(reverse))
        cache = self.__dict__.setdefault("_ddim_tables", {})
        if key not in cache:
            var = {ModelVarType.FIXED_SMALL: "fixed_small",
                   ModelVarType.FIXED_LARGE: "fixed_large"}.get(self.model_var_type, "learned_range")
            cache[key] = self.ddim_coefficients(eta=eta, reverse=reverse,
                                                predict_xstart=self.model_mean_type is ModelMeanType.START_X,
                                                var_type=var, clip_denoised=bool(clip_denoised))
        return cache[key]

    @staticmethod
    def _check_eta(eta, reverse):
        if not isinstance(eta, (int, float)) or isinstance(eta, bool):
            raise TypeError(f"eta must be a number, got {type(eta).__name__}")
        if eta < 0:
            raise ValueError(f"eta must be >= 0, got {eta}")
        if reverse and eta != 0:
            raise ValueError(f"the reverse DDIM step is the deterministic ODE: eta must be 0, got {eta}")

    # ------------------------------------------------------------------------------------------
    @staticmethod
    def _hip_module(model):
        from ..models.latent_model import ProteinMPNN_diffusion_new
        owner = getattr(model, "__self__", model)
        return owner if isinstance(owner, ProteinMPNN_diffusion_new) else None

    @staticmethod
    def _check_args(clip_denoised, denoised_fn, cond_fn):
        for name, fn in (("denoised_fn", denoised_fn), ("cond_fn", cond_fn)):
            if fn is not None and not callable(fn):
                raise TypeError(f"{name} must be callable or None, got {type(fn).__name__}")

    def _draw_noise(self, x, generator=None):
        """T draws of randn_like(x), in loop order, consuming the device RNG stream exactly as the
        reference's per-step `th.randn_like(x)` does (gaussian_diffusion.py:440)."""
        return torch.stack([torch.randn(x.shape, device=x.device, dtype=x.dtype, generator=generator)
                            for _ in range(self.num_timesteps)])

    def p_sample_loop(self, model, shape, noise=None, clip_denoised=True, denoised_fn=None, cond_fn=None,
                      model_kwargs=None, device=None, progress=False, step_noise=None):
        """Returns x_0 with `shape`.  `step_noise` [T, *shape] optionally supplies the per-step noise
        explicitly (loop order) instead of drawing it from the device RNG."""
        self._check_args(clip_denoised, denoised_fn, cond_fn)
        model_kwargs = model_kwargs or {}
        mod = self._hip_module(model)
        pinned = isinstance(denoised_fn, PinLatents) and cond_fn is None
        if mod is None or (denoised_fn is not None and not pinned) or cond_fn is not None:
            # any model callable, or a hook that is not the fused pin: step by step (the HIP model's forward per step)
            final = None
            for final in self.p_sample_loop_progressive(model, shape, noise=noise, clip_denoised=clip_denoised,
                                                        denoised_fn=denoised_fn, cond_fn=cond_fn,
                                                        model_kwargs=model_kwargs, device=device,
                                                        step_noise=step_noise):
                pass
            return final["sample"]
        if device is None:
            device = next(mod.parameters()).device
        img = noise if noise is not None else torch.randn(*shape, device=device)
        if not img.is_cuda:
            raise RuntimeError("p_sample_loop (codlad_amd) runs on the MI355X only")
        eps = step_noise if step_noise is not None else self._draw_noise(img)
        job, pin = self._fused_job(mod, img, model_kwargs, denoised_fn if pinned else None)
        T = self.num_timesteps
        x0 = mod.engine().sample(job, img.reshape(-1, img.shape[-1]), eps.reshape(T, -1, img.shape[-1]), self,
                                 coef=self.coefficients(clip_denoised), pin=pin)
        return x0.view(img.shape)

    def _fused_job(self, mod, img, model_kwargs, pin_fn):
        """The engine job of a fused loop on `img` [N, L, C] and its pin arrays (pin_fn: a PinLatents or None)."""
        batch = model_kwargs["batch"]
        n_rep = img.shape[0] // int(batch["num_CGs"].shape[0])
        job, lens = mod.job_for(batch, n_rep)
        mod._check_mask(model_kwargs.get("mask"), lens, n_rep)
        if self.self_condition != mod.self_condition:
            raise ValueError("create_diffusion(self_condition=...) and the model's self_condition differ: the fused "
                             "loop conditions exactly when the model was built for it (test.py:297-303)")
        if len(set(lens)) != 1:
            raise NotImplementedError("fused loop on a padded mixed-length batch; pass equal-length "
                                      "structures per call (what the reference's loaders produce)")
        pin = None
        if pin_fn is not None:
            if tuple(pin_fn.x0.shape) != tuple(img.shape) or not pin_fn.x0.is_cuda:
                raise ValueError(f"PinLatents: x0 must be a CUDA tensor of the sample's shape {tuple(img.shape)}, got "
                                 f"{tuple(pin_fn.x0.shape)} on {pin_fn.x0.device}")
            pin = (pin_fn.x0.reshape(-1, img.shape[-1]), pin_fn.mask.reshape(-1))
        return job, pin

    def p_sample_loop_progressive(self, model, shape, noise=None, clip_denoised=True, denoised_fn=None,
                                  cond_fn=None, model_kwargs=None, device=None, progress=False,
                                  step_noise=None):
        """Generic stepping for any CUDA model callable: model(x, t, **kwargs) -> [N,L,2C]."""
        self._check_args(clip_denoised, denoised_fn, cond_fn)
        model_kwargs = model_kwargs or {}
        img = noise if noise is not None else torch.randn(*shape, device=device)
        x_start = None
        for k, i in enumerate(range(self.num_timesteps - 1, -1, -1)):
            t = torch.tensor([i] * shape[0], device=img.device)
            eps = step_noise[k] if step_noise is not None else torch.randn_like(img)
            out = self.p_sample(model, img, t, clip_denoised=clip_denoised, denoised_fn=denoised_fn, cond_fn=cond_fn,
                                model_kwargs=model_kwargs, noise=eps, x_self_cond=x_start if self.self_condition else None)
            yield out
            img = out["sample"]
            x_start = out["pred_xstart"]

    def p_sample(self, model, x, t, clip_denoised=True, denoised_fn=None, cond_fn=None, model_kwargs=None,
                 x_self_cond=None, noise=None):
        self._check_args(clip_denoised, denoised_fn, cond_fn)
        if not x.is_cuda:
            raise RuntimeError("p_sample (codlad_amd) runs on the MI355X only")
        from .. import _lib
        i = int(t.reshape(-1)[0])
        map_t = torch.tensor(self.timestep_map, device=t.device, dtype=t.dtype)[t]   # respace.py:124-129
        kwargs = dict(model_kwargs or {})
        if x_self_cond is not None:
            kwargs["x_self_cond"] = x_self_cond
        model_out = model(x, map_t, **kwargs)
        C = x.shape[-1]
        assert C == 3 and model_out.shape[-1] == (C if self.fixed_variance else 2 * C), \
            "latent_size 3 only; a fixed-variance sampler takes a model without variance channels " \
            "(gaussian_diffusion.py:321-334)"
        import ctypes
        import numpy as np
        coef = np.ascontiguousarray(self.coefficients(clip_denoised)[i])
        if denoised_fn is not None or cond_fn is not None:
            # split step: raw pred_xstart -> denoised_fn -> clamp / posterior mean (+ variance * cond_fn) / noise, on the
            # device; cond_fn sees x_t, the original-process timesteps and the model's kwargs (respace.py:99-100, 117-129)
            from ..engine import Denoiser
            raw = Denoiser.ddpm_pred_xstart(x, model_out, coef).view(x.shape)
            pred = raw
            if denoised_fn is not None:
                pred = denoised_fn(raw)
                _check_hook_output(pred, x, "denoised_fn")
            if noise is None:                           # drawn where the reference draws it (gaussian_diffusion.py:440)
                noise = torch.randn_like(x)
            grad = None
            if cond_fn is not None:
                grad = cond_fn(x, map_t, **(model_kwargs or {}))
                _check_hook_output(grad, x, "cond_fn")
            sample, x_start = Denoiser.ddpm_posterior_step(x, pred, model_out, noise, coef, grad=grad,
                                                           fixed_variance=float(self.fixed_variances()[i]))
            return {"sample": sample.view(x.shape), "pred_xstart": x_start.view(x.shape)}
        if noise is None:
            noise = torch.randn_like(x)
        xs = x.contiguous().float()
        out = torch.empty_like(xs)
        x_start = torch.empty_like(xs)
        rc = _lib.lib().codlad_ddpm_update(_lib.ptr(xs), _lib.ptr(model_out.contiguous().float()),
                                           _lib.ptr(noise.contiguous().float()),
                                           coef.ctypes.data_as(ctypes.c_void_p), xs.numel() // 3,
                                           _lib.ptr(out), _lib.ptr(x_start), _lib.stream_ptr(x.device))
        _lib.check(rc, "codlad_ddpm_update")
        return {"sample": out, "pred_xstart": x_start}

    # -- DDIM -----------------------------------------------------------------------------------
    def condition_score(self, cond_fn, p_mean_var, x, t, model_kwargs=None):
        """gaussian_diffusion.py:386-402 (Song et al. 2020): what p_mean_variance would have returned had the model's
        score been conditioned by cond_fn - eps from pred_xstart, eps -= sqrt(1 - acp) * grad, pred_xstart from eps, the
        posterior mean of that.  cond_fn receives the original-process timesteps (respace.py:102-103).  On the device:
        codlad_ddim_step's condition_score and codlad_ddpm_posterior_step's mean (no clamp, no noise)."""
        if not callable(cond_fn):
            raise TypeError(f"cond_fn must be callable, got {type(cond_fn).__name__}")
        if not x.is_cuda:
            raise RuntimeError("condition_score (codlad_amd) runs on the MI355X only")
        from ..engine import Denoiser
        i = int(t.reshape(-1)[0])
        map_t = torch.tensor(self.timestep_map, device=t.device, dtype=t.dtype)[t]
        grad = cond_fn(x, map_t, **(model_kwargs or {}))
        _check_hook_output(grad, x, "cond_fn")
        row = self.ddim_coefs(False)[i].copy()
        row[7] = int(row[7]) & ~4                            # condition_score does not clamp again
        zeros = torch.zeros_like(x)
        _, pred = Denoiser.ddim_step(x, p_mean_var["pred_xstart"], zeros, row, grad=grad)
        post = self.coefficients(False)[i].copy()
        post[6] = 0.0                                        # the posterior mean alone
        post[7] = 2                                          # fixed-variance row: model_out is not read for it
        mean, _ = Denoiser.ddpm_posterior_step(x, pred, zeros, zeros, post)
        out = dict(p_mean_var)
        out["pred_xstart"] = pred.view(x.shape)
        out["mean"] = mean.view(x.shape)
        return out

    def _ddim_step(self, model, x, t, clip_denoised, denoised_fn, cond_fn, model_kwargs, eta, x_self_cond, noise,
                   reverse):
        """One DDIM step on the device: the model, the raw pred_xstart (codlad_ddpm_pred_xstart), denoised_fn, cond_fn's
        gradient, then codlad_ddim_step (clamp, condition_score, eps, update)."""
        self._check_args(clip_denoised, denoised_fn, cond_fn)
        self._check_eta(eta, reverse)
        if not x.is_cuda:
            raise RuntimeError("ddim_sample (codlad_amd) runs on the MI355X only")
        import numpy as np
        from ..engine import Denoiser
        i = int(t.reshape(-1)[0])
        map_t = torch.tensor(self.timestep_map, device=t.device, dtype=t.dtype)[t]   # respace.py:124-129
        kwargs = dict(model_kwargs or {})
        if x_self_cond is not None:
            kwargs["x_self_cond"] = x_self_cond
        model_out = model(x, map_t, **kwargs)
        C = x.shape[-1]
        assert C == 3 and model_out.shape[-1] == (C if self.fixed_variance else 2 * C), \
            "latent_size 3 only; a fixed-variance sampler takes a model without variance channels " \
            "(gaussian_diffusion.py:303-306, 321-334)"
        coef = np.ascontiguousarray(self.ddim_coefs(clip_denoised, eta, reverse)[i])
        pred = Denoiser.ddpm_pred_xstart(x, model_out, coef).view(x.shape)
        if denoised_fn is not None:
            pred = denoised_fn(pred)
            _check_hook_output(pred, x, "denoised_fn")
        grad = None
        if cond_fn is not None:
            grad = cond_fn(x, map_t, **(model_kwargs or {}))
            _check_hook_output(grad, x, "cond_fn")
        if not reverse and noise is None:
            noise = torch.randn_like(x)                  # drawn where the released ddim_sample draws it, also at eta = 0
        sample, x_start = Denoiser.ddim_step(x, pred, None if reverse else noise, coef, grad=grad, reverse=reverse)
        return {"sample": sample.view(x.shape), "pred_xstart": x_start.view(x.shape)}

    def ddim_sample(self, model, x, t, clip_denoised=True, denoised_fn=None, cond_fn=None, model_kwargs=None, eta=0.0,
                    x_self_cond=None, noise=None):
        """x_{t-1} from x_t by DDIM: {"sample", "pred_xstart"}.  noise: this step's draw (None: randn_like(x))."""
        return self._ddim_step(model, x, t, clip_denoised, denoised_fn, cond_fn, model_kwargs, eta, x_self_cond, noise,
                               reverse=False)

    def ddim_reverse_sample(self, model, x, t, clip_denoised=True, denoised_fn=None, cond_fn=None, model_kwargs=None,
                            eta=0.0, x_self_cond=None):
        """x_{t+1} from x_t by the reverse DDIM ODE (eta must be 0): {"sample", "pred_xstart"}."""
        return self._ddim_step(model, x, t, clip_denoised, denoised_fn, cond_fn, model_kwargs, eta, x_self_cond, None,
                               reverse=True)

    def _ddim_fusable(self, mod, denoised_fn, cond_fn):
        return mod is not None and cond_fn is None and (denoised_fn is None or isinstance(denoised_fn, PinLatents))

    def ddim_sample_loop(self, model, shape, noise=None, clip_denoised=True, denoised_fn=None, cond_fn=None,
                         model_kwargs=None, device=None, progress=False, eta=0.0, step_noise=None):
        """Returns x_0 with `shape`, sampled by DDIM.  `step_noise` [T, *shape] as for p_sample_loop.  One randn_like(x)
        is drawn per step at any eta, as the released ddim_sample does, on both paths."""
        self._check_args(clip_denoised, denoised_fn, cond_fn)
        self._check_eta(eta, False)
        model_kwargs = model_kwargs or {}
        mod = self._hip_module(model)
        if not self._ddim_fusable(mod, denoised_fn, cond_fn):
            final = None
            for final in self.ddim_sample_loop_progressive(model, shape, noise=noise, clip_denoised=clip_denoised,
                                                           denoised_fn=denoised_fn, cond_fn=cond_fn,
                                                           model_kwargs=model_kwargs, device=device, eta=eta,
                                                           step_noise=step_noise):
                pass
            return final["sample"]
        if device is None:
            device = next(mod.parameters()).device
        img = noise if noise is not None else torch.randn(*shape, device=device)
        if not img.is_cuda:
            raise RuntimeError("ddim_sample_loop (codlad_amd) runs on the MI355X only")
        eps = step_noise if step_noise is not None else self._draw_noise(img)
        job, pin = self._fused_job(mod, img, model_kwargs, denoised_fn)
        T = self.num_timesteps
        x0 = mod.engine().sample(job, img.reshape(-1, img.shape[-1]), eps.reshape(T, -1, img.shape[-1]), self,
                                 coef=self.ddim_coefs(clip_denoised, eta), pin=pin, kind="ddim")
        return x0.view(img.shape)

    def ddim_sample_loop_progressive(self, model, shape, noise=None, clip_denoised=True, denoised_fn=None, cond_fn=None,
                                     model_kwargs=None, device=None, progress=False, eta=0.0, step_noise=None):
        """Generic DDIM stepping for any CUDA model callable; yields each step's {"sample", "pred_xstart"}."""
        self._check_args(clip_denoised, denoised_fn, cond_fn)
        self._check_eta(eta, False)
        model_kwargs = model_kwargs or {}
        img = noise if noise is not None else torch.randn(*shape, device=device)
        x_start = None
        for k, i in enumerate(range(self.num_timesteps - 1, -1, -1)):
            t = torch.tensor([i] * shape[0], device=img.device)
            out = self.ddim_sample(model, img, t, clip_denoised=clip_denoised, denoised_fn=denoised_fn, cond_fn=cond_fn,
                                   model_kwargs=model_kwargs, eta=eta,
                                   x_self_cond=x_start if self.self_condition else None,
                                   noise=step_noise[k] if step_noise is not None else None)
            yield out
            img = out["sample"]
            x_start = out["pred_xstart"]

    def ddim_reverse_sample_loop(self, model, x, clip_denoised=True, denoised_fn=None, cond_fn=None, model_kwargs=None,
                                 device=None, progress=False, eta=0.0):
        """DDIM inversion: x_0 [N, L, C] -> x_T along the deterministic ODE (eta must be 0), steps i = 0 .. T-1.  The
        HIP model with no hook or only a PinLatents runs fused (codlad_ddim_loop, reverse); anything else step by step."""
        self._check_args(clip_denoised, denoised_fn, cond_fn)
        self._check_eta(eta, True)
        model_kwargs = model_kwargs or {}
        mod = self._hip_module(model)
        if not self._ddim_fusable(mod, denoised_fn, cond_fn):
            final = None
            for final in self.ddim_reverse_sample_loop_progressive(model, x, clip_denoised=clip_denoised,
                                                                   denoised_fn=denoised_fn, cond_fn=cond_fn,
                                                                   model_kwargs=model_kwargs, device=device, eta=eta):
                pass
            return final["sample"]
        if not x.is_cuda:
            raise RuntimeError("ddim_reverse_sample_loop (codlad_amd) runs on the MI355X only")
        job, pin = self._fused_job(mod, x, model_kwargs, denoised_fn)
        xT = mod.engine().sample(job, x.reshape(-1, x.shape[-1]), None, self, coef=self.ddim_coefs(clip_denoised, 0.0, True),
                                 pin=pin, kind="ddim_reverse")
        return xT.view(x.shape)

    def ddim_reverse_sample_loop_progressive(self, model, x, clip_denoised=True, denoised_fn=None, cond_fn=None,
                                             model_kwargs=None, device=None, progress=False, eta=0.0):
        """Generic reverse DDIM stepping; yields each step's {"sample", "pred_xstart"} (the last sample is x_T)."""
        self._check_args(clip_denoised, denoised_fn, cond_fn)
        self._check_eta(eta, True)
        img, x_start = x, None
        for i in range(self.num_timesteps):
            t = torch.tensor([i] * x.shape[0], device=img.device)
            out = self.ddim_reverse_sample(model, img, t, clip_denoised=clip_denoised, denoised_fn=denoised_fn,
                                           cond_fn=cond_fn, model_kwargs=model_kwargs, eta=eta,
                                           x_self_cond=x_start if self.self_condition else None)
            yield out
            img = out["sample"]
            x_start = out["pred_xstart"]


    # -- DPM-Solver++(2M) ----------------------------------------------------------------------
    def dpm_solver_coefs(self, clip_denoised, order=2):
        """The [T, 8] DPM-Solver++ table of the kernels for this sampler's branches (Tables.dpm_solver_coefficients)."""
        self._check_order(order)
        key = (bool(clip_denoised), int(order))
        cache = self.__dict__.setdefault("_dpm_tables", {})
        if key not in cache:
            var = {ModelVarType.FIXED_SMALL: "fixed_small",
                   ModelVarType.FIXED_LARGE: "fixed_large"}.get(self.model_var_type, "learned_range")
            cache[key] = self.dpm_solver_coefficients(order=int(order),
                                                      predict_xstart=self.model_mean_type is ModelMeanType.START_X,
                                                      var_type=var, clip_denoised=bool(clip_denoised))
        return cache[key]

    @staticmethod
    def _check_order(order):
        if isinstance(order, bool) or not isinstance(order, int):
            raise TypeError(f"order must be an int, got {type(order).__name__}")
        if order not in (1, 2):
            raise ValueError(f"DPM-Solver++ order must be 1 or 2, got {order}")

    def dpm_solver_sample_loop(self, model, shape, noise=None, clip_denoised=True, denoised_fn=None, cond_fn=None,
                               model_kwargs=None, device=None, progress=False, order=2):
        """Returns x_0 with `shape`, sampled by DPM-Solver++(2M) (order=1: DDIM at eta 0): deterministic given `noise`
        (x_T), one model evaluation per step.  Meant for 10-25 steps on the "logsnrN" respacing.  The HIP model with no
        hook or only a PinLatents runs fused (codlad_dpm_loop); anything else step by step."""
        self._check_args(clip_denoised, denoised_fn, cond_fn)
        self._check_order(order)
        model_kwargs = model_kwargs or {}
        mod = self._hip_module(model)
        if not self._ddim_fusable(mod, denoised_fn, cond_fn):
            final = None
            for final in self.dpm_solver_sample_loop_progressive(model, shape, noise=noise, clip_denoised=clip_denoised,
                                                                 denoised_fn=denoised_fn, cond_fn=cond_fn,
                                                                 model_kwargs=model_kwargs, device=device, order=order):
                pass
            return final["sample"]
        if device is None:
            device = next(mod.parameters()).device
        img = noise if noise is not None else torch.randn(*shape, device=device)
        if not img.is_cuda:
            raise RuntimeError("dpm_solver_sample_loop (codlad_amd) runs on the MI355X only")
        job, pin = self._fused_job(mod, img, model_kwargs, denoised_fn)
        x0 = mod.engine().sample(job, img.reshape(-1, img.shape[-1]), None, self,
                                 coef=self.dpm_solver_coefs(clip_denoised, order), pin=pin, kind="dpmpp")
        return x0.view(img.shape)

    def dpm_solver_sample_loop_progressive(self, model, shape, noise=None, clip_denoised=True, denoised_fn=None,
                                           cond_fn=None, model_kwargs=None, device=None, progress=False, order=2):
        """Generic DPM-Solver++ stepping for any CUDA model callable; yields each step's {"sample", "pred_xstart"}: the
        model, the raw pred_xstart (codlad_ddpm_pred_xstart), denoised_fn, cond_fn's gradient, then codlad_dpm_step with
        the previous step's pred_xstart."""
        self._check_args(clip_denoised, denoised_fn, cond_fn)
        self._check_order(order)
        import numpy as np
        from ..engine import Denoiser
        model_kwargs = model_kwargs or {}
        img = noise if noise is not None else torch.randn(*shape, device=device)
        if not img.is_cuda:
            raise RuntimeError("dpm_solver_sample_loop (codlad_amd) runs on the MI355X only")
        table = self.dpm_solver_coefs(clip_denoised, order)
        x_start = None
        for i in range(self.num_timesteps - 1, -1, -1):
            t = torch.tensor([i] * shape[0], device=img.device)
            map_t = torch.tensor(self.timestep_map, device=t.device, dtype=t.dtype)[t]   # respace.py:124-129
            kwargs = dict(model_kwargs)
            if self.self_condition and x_start is not None:
                kwargs["x_self_cond"] = x_start
            model_out = model(img, map_t, **kwargs)
            C = img.shape[-1]
            assert C == 3 and model_out.shape[-1] == (C if self.fixed_variance else 2 * C), \
                "latent_size 3 only; a fixed-variance sampler takes a model without variance channels " \
                "(gaussian_diffusion.py:303-306, 321-334)"
            coef = np.ascontiguousarray(table[i])
            pred = Denoiser.ddpm_pred_xstart(img, model_out, coef).view(img.shape)
            if denoised_fn is not None:
                pred = denoised_fn(pred)
                _check_hook_output(pred, img, "denoised_fn")
            grad = None
            if cond_fn is not None:
                grad = cond_fn(img, map_t, **model_kwargs)
                _check_hook_output(grad, img, "cond_fn")
            sample, used = Denoiser.dpm_step(img, pred, x_start if coef[4] != 0 else None, coef, grad=grad)
            img, x_start = sample.view(img.shape), used.view(img.shape)
            yield {"sample": img, "pred_xstart": x_start}


def _use_timesteps(diffusion_steps, timestep_respacing, betas):
    """The base steps a respacing spec keeps: "logsnrN" is N steps uniform in log-SNR on this schedule
    (schedule.logsnr_timesteps), every other spec is the reference's (space_timesteps)."""
    if isinstance(timestep_respacing, str) and timestep_respacing.startswith("logsnr"):
        try:
            n = int(timestep_respacing[len("logsnr"):])
        except ValueError:
            raise ValueError(f"respacing spec {timestep_respacing!r}: logsnr takes a step count, as in \"logsnr20\"") from None
        return logsnr_timesteps(betas, n)
    return space_timesteps(diffusion_steps, timestep_respacing)


def create_diffusion(timestep_respacing, noise_schedule="linear", use_kl=False, rescale_learned_sigmas=False,
                     sigma_small=False, predict_xstart=False, learn_sigma=True, diffusion_steps=1000,
                     self_condition=False):
    if timestep_respacing is None or timestep_respacing == "":
        timestep_respacing = [diffusion_steps]
    # reference diffusion_and_flow/__init__.py:28-43
    mean_type = ModelMeanType.START_X if predict_xstart else ModelMeanType.EPSILON
    var_type = ModelVarType.LEARNED_RANGE if learn_sigma else (ModelVarType.FIXED_SMALL if sigma_small
                                                               else ModelVarType.FIXED_LARGE)
    # reference diffusion_and_flow/__init__.py:44-50
    loss_type = LossType.RESCALED_KL if use_kl else (LossType.RESCALED_MSE if rescale_learned_sigmas else LossType.MSE)
    betas = named_betas(noise_schedule, diffusion_steps)
    return SpacedDiffusion(use_timesteps=_use_timesteps(diffusion_steps, timestep_respacing, betas), betas=betas,
                           model_mean_type=mean_type, model_var_type=var_type,
                           loss_type=loss_type, self_condition=self_condition)
