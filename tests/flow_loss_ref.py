"""CPU restatement of the flow-matching probability paths and regression losses (Tong et al. 2023, Lipman et al. 2023,
Albergo et al. 2023; the losses are the textbook l2 / l1 / Huber / smooth-l1 / log-cosh), written from the formulas:
in fp32 with one rounding per operation in the order the formulas are written (which is the device kernels' order), and in
float64, where the losses are differentiable in `model_out` - the propagated bound of the end-to-end tests needs that.

t: [N] (one time per sample) for latents [N, L, 3].
"""
import math

import torch

LOSS_TYPES = ("l2", "l1", "huber", "smooth_l1", "log_cosh")


def _pad(t, x):
    return torch.as_tensor(t, dtype=x.dtype).reshape(-1, 1, 1)


def path(kind, sigma, x0, x1, t, eps, dtype=torch.float32):
    """(xt, ut) of the matcher `kind` ("icfm", "target", "vp") in `dtype`.  The scalars enter as the reference's Python
    floats do: sigma, 1 - sigma (formed in double) and pi / 2 are rounded to `dtype` when they meet a tensor."""
    cast = lambda a: None if a is None else a.to(dtype)               # noqa: E731
    x0, x1, eps = cast(x0), cast(x1), cast(eps)
    t = _pad(torch.as_tensor(t).to(dtype), x1)
    sc = lambda v: torch.tensor(v, dtype=torch.float64).to(dtype)     # noqa: E731
    if kind == "icfm":
        mu = t * x1 + (1 - t) * x0
        xt = mu + sc(sigma) * eps if sigma != 0 else mu
        return xt, x1 - x0
    if kind == "target":
        c = sc(1.0 - sigma)
        sigma_t = 1 - c * t
        xt = t * x1 + sigma_t * eps
        return xt, (x1 - c * xt) / (1 - c * t)
    if kind == "vp":
        h = sc(math.pi / 2)
        cs, sn = torch.cos(h * t), torch.sin(h * t)
        mu = cs * x0 + sn * x1
        xt = mu + sc(sigma) * eps if sigma != 0 else mu
        return xt, h * (cs * x1 - sn * x0)
    raise ValueError(kind)


def elements(model_out, ut):
    """The five losses per element, in the dtype of the operands."""
    d = model_out - ut
    ad, dd = d.abs(), d * d
    hub = torch.where(ad < 1, 0.5 * dd, ad - 0.5)
    return dict(l2=dd, l1=ad, huber=hub, smooth_l1=hub, log_cosh=torch.log(torch.cosh(d)))


def terms64(model_out, ut):
    """model_out, ut [N, L, 3] -> dict of float64 [N]: the mean of every loss over the sample's elements.  Differentiable
    in model_out."""
    e = elements(model_out.double(), ut.double())
    return {k: v.mean(dim=(1, 2)) for k, v in e.items()}


def terms32(model_out, ut):
    """The same in fp32, summed per sample in the device kernel's fixed order: half wave w of eight takes nodes w, w + 8,
    ..., lane k component k; then (lane 0 + lane 1) + lane 2 per half wave, then half waves 0 .. 7 in order."""
    e = elements(model_out.float(), ut.float())
    N, L, _ = model_out.shape
    out = {}
    for k, v in e.items():
        res = []
        for s in range(N):
            parts = []
            for w in range(8):
                acc = torch.zeros(3, dtype=torch.float32)
                for n in range(w, L, 8):
                    acc = acc + v[s, n]
                parts.append((acc[0] + acc[1]) + acc[2])
            tot = parts[0]
            for w in range(1, 8):
                tot = tot + parts[w]
            res.append(tot / torch.tensor(float(3 * L), dtype=torch.float32))
        out[k] = torch.stack(res)
    return out


def batch_scalar(per_sample, lens):
    """The batch scalar of loss_fn with an all-true mask from per-sample means [N] and lengths: float64."""
    w = torch.tensor([3.0 * n for n in lens], dtype=torch.float64)
    return float((per_sample.double() * w).sum() / w.sum())
