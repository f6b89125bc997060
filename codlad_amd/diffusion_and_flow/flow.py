"""Drop-in for the reference's `diffusion_and_flow.flow` (conditional flow matchers), forward-only.

Same classes and call surface as the reference (`diffusion_and_flow/flow.py`): `ConditionalFlowMatcher` (--model icfm),
`TargetConditionalFlowMatcher` (--model fm) and `VariancePreservingConditionalFlowMatcher` (--model vpfm), each with
`compute_mu_t`, `compute_sigma_t`, `sample_xt`, `compute_conditional_flow` and
`sample_location_and_conditional_flow(x0, x1, t=None, return_noise=False)`.  The arithmetic is on the GPU, through
`codlad_fm_path`, every operation rounded separately in the reference's order; CPU tensors raise - there is no fallback.

Added for scoring a checkpoint without sampling from it (the reference's validation pass, train_latent.py:302-350):
`training_losses` (one time per sample, the reference's `loss_fn(vt, ut)`) and `loss_sweep` (the loss at every time of a
list, the flow-model counterpart of calc_bpd_loop's per-step table).  When `model` is the forward of the codlad_amd
`ProteinMPNN_diffusion_new` both run fused (`codlad_fm_loss_forward` per group of equal times, one
`codlad_fm_loss_loop` for a sweep); any other CUDA callable is followed by `codlad_fm_terms`.  Gradients, training and
timestep samplers are out of scope.

`ExactOptimalTransportConditionalFlowMatcher` and `SchrodingerBridgeConditionalFlowMatcher` exist and refuse: see their
docstrings.
"""
import torch

from .. import _lib

LOSS_TYPES = ("l2", "l1", "huber", "smooth_l1", "log_cosh")


def _lat3(x, what):
    """[N, L, 3] device latents -> ([N * L, 3] fp32, nodes per sample)."""
    if not isinstance(x, torch.Tensor):
        raise TypeError(f"{what} must be a tensor, got {type(x).__name__}")
    if not x.is_cuda:
        raise RuntimeError(f"{what}: the flow matchers (codlad_amd) run on the MI355X only")
    if x.dim() != 3 or x.shape[-1] != 3:
        raise NotImplementedError(f"{what}: latents [N, L, 3] only, got {tuple(x.shape)}")
    return x.reshape(-1, 3), [int(x.shape[1])] * int(x.shape[0])


def _same_shape(a, b, what):
    if tuple(a.shape) != tuple(b.shape):
        raise ValueError(f"{what} {tuple(a.shape)} does not match x1 {tuple(b.shape)}")


def _check_loss_type(loss_type):
    if loss_type not in LOSS_TYPES:
        raise ValueError(f"loss_type must be one of {LOSS_TYPES}, got {loss_type!r}")


def batch_loss(per_sample, lens):
    """The reference's batch scalar loss_fn(vt, ut) with an all-true mask - the sum over all elements divided by their
    count - formed on the host in float64 from the per-sample means [..., N] and the samples' lengths."""
    w = torch.as_tensor([3 * int(n) for n in lens], dtype=torch.float64)
    v = per_sample.detach().to("cpu", torch.float64)
    return (v * w).sum(dim=-1) / w.sum()


def loss_fn(pred, target, mask=None, loss_type="l2"):
    """utils/train_module.py loss_fn on the device (codlad_fm_terms): the mean of the chosen regression loss over all
    elements of pred / target [N, L, 3] -> a 0-dim float64 tensor (the per-sample means are fp32 sums in the kernel's
    fixed order; the batch scalar is formed from them on the host in float64).  mask: None or all true (the ragged HIP
    path has no padded positions to mask out)."""
    from ..engine import Denoiser
    _check_loss_type(loss_type)
    flat, lens = _lat3(pred, "loss_fn: pred")
    tflat, _ = _lat3(target, "loss_fn: target")
    _same_shape(pred, target, "pred")
    if mask is not None and not bool(torch.as_tensor(mask).bool().all()):
        raise NotImplementedError("loss_fn: a mask with false entries (padded batches are not built on the ragged HIP path)")
    return batch_loss(Denoiser.fm_terms(flat, tflat, lens)[loss_type], lens)


def _hip_module(model):
    from ..models.latent_model import ProteinMPNN_diffusion_new
    owner = getattr(model, "__self__", model)
    return owner if isinstance(owner, ProteinMPNN_diffusion_new) else None


def _fused_job(mod, x, model_kwargs):
    """The engine job of the HIP model for latents x [N, L, 3] (model_kwargs: batch=, mask= as the model's forward)."""
    batch = (model_kwargs or {}).get("batch")
    if batch is None:
        raise ValueError("the HIP model needs model_kwargs['batch']")
    B = int(batch["num_CGs"].shape[0])
    if x.shape[0] % B:
        raise ValueError("x batch size must be a multiple of the number of structures in batch")
    n_rep = x.shape[0] // B
    job, lens = mod.job_for(batch, n_rep)
    mod._check_mask(model_kwargs.get("mask"), lens, n_rep)
    if len(set(lens)) != 1:
        raise NotImplementedError("fused loss on a padded mixed-length batch; pass equal-length structures per call "
                                  "(what the reference's loaders produce)")
    return job


class ConditionalFlowMatcher:
    """Independent conditional flow matching (Tong et al. 2023): the path N(t x1 + (1 - t) x0, sigma), the flow x1 - x0."""

    kind = "icfm"

    def __init__(self, sigma=0.0):
        if isinstance(sigma, bool) or not isinstance(sigma, (int, float)):
            raise TypeError(f"sigma must be a number, got {type(sigma).__name__}")
        if not sigma >= 0:
            raise ValueError(f"sigma must be >= 0, got {sigma}")
        self.sigma = sigma

    # -- the reference's pieces, each through codlad_fm_path ----------------------------------
    def _path(self, x0, x1, t, eps, sigma=None):
        from ..engine import Denoiser
        flat1, lens = _lat3(x1, "x1")
        f0 = fe = None
        if x0 is not None:
            f0 = _lat3(x0, "x0")[0]
            _same_shape(x0, x1, "x0")
        if eps is not None:
            fe = _lat3(eps, "epsilon")[0]
            _same_shape(eps, x1, "epsilon")
        xt, ut = Denoiser.fm_path(self.kind, self.sigma if sigma is None else sigma, f0, flat1, fe, lens, t)
        return xt.view(x1.shape), ut.view(x1.shape)

    def compute_mu_t(self, x0, x1, t):
        """The mean of the path at t (one value or [N]): xt at sigma = 0."""
        return self._path(x0, x1, t, None, sigma=0.0)[0]

    def compute_sigma_t(self, t):
        del t
        return self.sigma

    def sample_xt(self, x0, x1, t, epsilon):
        return self._path(x0, x1, t, epsilon)[0]

    def compute_conditional_flow(self, x0, x1, t, xt):
        del xt
        return self._path(x0, x1, t, None, sigma=0.0)[1]

    def sample_noise_like(self, x):
        return torch.randn_like(x)

    def _draw_t(self, x0):
        # reference flow.py:187-190: one standard normal per sample from the CPU's global generator, moved to x0's device
        # and type, then the logistic function (its `* 1 + 0` changes no value)
        return torch.sigmoid(torch.randn(int(x0.shape[0])).type_as(x0))

    def sample_location_and_conditional_flow(self, x0, x1, t=None, return_noise=False):
        """(t [N], xt, ut (, eps)): t drawn as sigmoid(randn) when None, eps = randn_like(x0), both where the reference
        draws them; xt and ut from one codlad_fm_path call."""
        _lat3(x0, "x0")
        if t is None:
            t = self._draw_t(x0)
        if not isinstance(t, torch.Tensor):
            t = torch.as_tensor(t, dtype=torch.float32, device=x0.device).reshape(-1)
        if t.numel() != x0.shape[0]:
            raise ValueError(f"t must hold one time per sample ({x0.shape[0]}), got {t.numel()}")
        eps = self.sample_noise_like(x0)
        xt, ut = self._path(x0, x1, t, eps)
        return (t, xt, ut, eps) if return_noise else (t, xt, ut)

    # -- forward-only loss evaluation -------------------------------------------------------------
    def _result(self, terms, lens, loss_type, t=None):
        out = {"loss": batch_loss(terms[loss_type], lens), "per_sample": terms[loss_type],
               "terms": {k: terms[k] for k in LOSS_TYPES}}
        if t is not None:
            out["t"] = t
        return out

    def training_losses(self, model, x0, x1, t=None, eps=None, model_kwargs=None, loss_type="l2"):
        """The reference's validation loss of one batch (train_latent.py:338-350), forward-only: t [N] (None: drawn as
        the reference draws it), xt, ut from the path, vt = model(xt, t, **model_kwargs), loss_fn(vt, ut) ->
        {"loss": 0-dim float64 (the batch scalar, all-true mask: formed on the host from the per-sample means and
        lengths), "per_sample" [N], "t" [N], "terms": {l2, l1, huber, smooth_l1, log_cosh: [N]}}.  eps: the path's noise
        (None: randn_like(x1)).  The HIP model's forward runs fused, samples grouped by equal time (N distinct times cost
        N small forwards: `loss_sweep` is the fast path); any other callable receives (xt, t) with per-sample t."""
        from ..engine import Denoiser
        _check_loss_type(loss_type)
        flat1, lens = _lat3(x1, "x1")
        model_kwargs = dict(model_kwargs or {})
        if t is None:
            t = self._draw_t(x1)
        if not isinstance(t, torch.Tensor):
            t = torch.as_tensor(t, dtype=torch.float32, device=x1.device).reshape(-1)
        t = t.to(x1.device, torch.float32)
        if t.numel() != x1.shape[0]:
            raise ValueError(f"t must hold one time per sample ({x1.shape[0]}), got {t.numel()}")
        if eps is None:
            eps = torch.randn_like(x1)
        _same_shape(eps, x1, "eps")
        f0 = None
        if x0 is not None:
            f0 = _lat3(x0, "x0")[0]
            _same_shape(x0, x1, "x0")
        fe = _lat3(eps, "eps")[0]
        mod = _hip_module(model)
        if mod is not None:
            job = _fused_job(mod, x1, model_kwargs)
            r = mod.engine().fm_loss_terms(job, flat1, t, kind=self.kind, sigma=self.sigma, x0=f0, eps=fe)
            return self._result(r, lens, loss_type, t)
        xt, ut = Denoiser.fm_path(self.kind, self.sigma, f0, flat1, fe, lens, t)
        vt = model(xt.view(x1.shape), t, **model_kwargs)
        return self._result(self._foreign_terms(vt, ut, x1, lens), lens, loss_type, t)

    @staticmethod
    def _foreign_terms(vt, ut, x1, lens):
        from ..engine import Denoiser
        if not isinstance(vt, torch.Tensor) or tuple(vt.shape) != tuple(x1.shape):
            raise ValueError(f"the model must return the velocity, a tensor {tuple(x1.shape)}")
        return Denoiser.fm_terms(vt.reshape(-1, 3), ut, lens)

    def loss_sweep(self, model, x0, x1, ts, step_noise=None, loss_type="l2", model_kwargs=None):
        """The loss at every time of `ts` (host floats in [0, 1], each shared by all samples) -> {"loss" [K] float64 (the
        batch scalar per time), "per_sample" [N, K], "terms": {...: [N, K]}}: the error per time, the flow-model
        counterpart of calc_bpd_loop's per-step table.  step_noise [K, *x1.shape]: the path's noise per time (None: K
        draws of randn_like(x1)).  One codlad_fm_loss_loop call when `model` is the HIP model's forward; any other
        callable is evaluated once per time on (xt, t [N])."""
        from ..engine import Denoiser
        _check_loss_type(loss_type)
        flat1, lens = _lat3(x1, "x1")
        model_kwargs = dict(model_kwargs or {})
        ts = [float(v) for v in ts]
        K = len(ts)
        if step_noise is None:
            step_noise = torch.stack([torch.randn_like(x1) for _ in range(K)])
        if tuple(step_noise.shape) != (K,) + tuple(x1.shape):
            raise ValueError(f"step_noise must be [K, *x1.shape] = {(K,) + tuple(x1.shape)}, got {tuple(step_noise.shape)}")
        if not step_noise.is_cuda:
            raise RuntimeError("step_noise: the flow matchers (codlad_amd) run on the MI355X only")
        f0 = None
        if x0 is not None:
            f0 = _lat3(x0, "x0")[0]
            _same_shape(x0, x1, "x0")
        eps = step_noise.reshape(K, -1, 3)
        mod = _hip_module(model)
        if mod is not None:
            job = _fused_job(mod, x1, model_kwargs)
            r = mod.engine().fm_loss_sweep(job, flat1, ts, kind=self.kind, sigma=self.sigma, x0=f0, eps=eps)
            terms = {k: r[k].t().contiguous() for k in LOSS_TYPES}
        else:
            rows = []
            for k, tv in enumerate(ts):
                xt, ut = Denoiser.fm_path(self.kind, self.sigma, f0, flat1, eps[k], lens, tv)
                t = torch.full((x1.shape[0],), tv, dtype=torch.float32, device=x1.device)
                rows.append(self._foreign_terms(model(xt.view(x1.shape), t, **model_kwargs), ut, x1, lens))
            terms = {k: torch.stack([r[k] for r in rows], dim=1) for k in LOSS_TYPES}
        return {"loss": batch_loss(terms[loss_type].t(), lens), "per_sample": terms[loss_type], "terms": terms}


class TargetConditionalFlowMatcher(ConditionalFlowMatcher):
    """Lipman et al. 2023 (the reference's --model fm): the path N(t x1, 1 - (1 - sigma) t), the flow
    (x1 - (1 - sigma) xt) / (1 - (1 - sigma) t).  x0 is not read (the reference deletes it)."""

    kind = "target"

    def compute_mu_t(self, x0, x1, t):
        del x0
        return self._path(None, x1, t, torch.zeros_like(x1))[0]            # t x1 + sigma_t * 0

    def compute_sigma_t(self, t):
        """1 - (1 - sigma) t, [N] on the device of t: the path of x1 = 0, eps = 1."""
        if not isinstance(t, torch.Tensor):
            raise TypeError("compute_sigma_t: t must be a device tensor [N]")
        if not t.is_cuda:
            raise RuntimeError("compute_sigma_t: the flow matchers (codlad_amd) run on the MI355X only")
        n = t.numel()
        zero = torch.zeros(n, 1, 3, dtype=torch.float32, device=t.device)
        return self._path(None, zero, t, torch.ones_like(zero))[0][:, 0, 0].reshape(t.shape)

    def sample_xt(self, x0, x1, t, epsilon):
        del x0
        return self._path(None, x1, t, epsilon)[0]

    def compute_conditional_flow(self, x0, x1, t, xt):
        """The flow of a GIVEN location xt (codlad_fm_path, kind CODLAD_FM_TARGET_FLOW)."""
        from ..engine import Denoiser
        del x0
        flat1, lens = _lat3(x1, "x1")
        flat_t = _lat3(xt, "xt")[0].contiguous().float()
        _same_shape(xt, x1, "xt")
        flat1 = flat1.contiguous().float()
        _ts, shared, t_dev = Denoiser._fm_times(t, len(lens), x1.device)
        ut = torch.empty_like(flat1)
        rc = _lib.lib().codlad_fm_path(None, _lib.ptr(flat1), None, _lib.ptr(Denoiser.sample_offsets(lens, x1.device)),
                                       len(lens), _lib.ptr(t_dev), 0.0 if shared is None else shared, _lib.FM_TARGET_FLOW,
                                       float(self.sigma), _lib.ptr(flat_t), _lib.ptr(ut), _lib.stream_ptr(x1.device))
        _lib.check(rc, "codlad_fm_path")
        return ut.view(x1.shape)

    def _path(self, x0, x1, t, eps, sigma=None):
        return super()._path(None, x1, t, eps, sigma)


class VariancePreservingConditionalFlowMatcher(ConditionalFlowMatcher):
    """Albergo et al. 2023 trigonometric interpolants: the path N(cos(pi t / 2) x0 + sin(pi t / 2) x1, sigma), the flow
    pi / 2 (cos(pi t / 2) x1 - sin(pi t / 2) x0)."""

    kind = "vp"


class ExactOptimalTransportConditionalFlowMatcher(ConditionalFlowMatcher):
    """Not built: OT-CFM couples x0 and x1 by the exact optimal-transport plan of the minibatch, which the reference
    takes from the POT package (`ot.emd`); that package is not part of this project's environment and its solver cannot
    be pinned to the reference's, so the coupling - and every number after it - would be unpinned."""

    def __init__(self, sigma=0.0):
        raise NotImplementedError("ExactOptimalTransportConditionalFlowMatcher needs the POT package's exact transport "
                                  "plan (ot.emd) for its minibatch coupling; it is absent here and cannot be pinned to the "
                                  "reference's, so OT-CFM is not built")


class SchrodingerBridgeConditionalFlowMatcher(ConditionalFlowMatcher):
    """Not built: SB-CFM trains a score head beside the velocity (`vt, st = model(...)`, train_latent.py:336) and its
    loss needs that second output; the mpnn_diffusion model has no score head.  Its coupling needs the POT package too."""

    def __init__(self, sigma=1.0, ot_method="exact"):
        raise NotImplementedError("SchrodingerBridgeConditionalFlowMatcher needs a model with a score head beside the "
                                  "velocity (and the POT package's entropic plan); the mpnn_diffusion model has none, so "
                                  "SB-CFM is not built")


MATCHERS = {"fm": TargetConditionalFlowMatcher, "icfm": ConditionalFlowMatcher,
            "vpfm": VariancePreservingConditionalFlowMatcher}


def create_flow_matcher(model, sigma=0.0):
    """The matcher of a --model name (reference train_latent.py: fm / icfm / vpfm; otcfm and sbcfm refuse)."""
    if model == "otcfm":
        return ExactOptimalTransportConditionalFlowMatcher(sigma)
    if model == "sbcfm":
        return SchrodingerBridgeConditionalFlowMatcher(sigma)
    if model not in MATCHERS:
        raise ValueError(f"no flow matcher for --model {model!r}: fm, icfm and vpfm are built")
    return MATCHERS[model](sigma)
