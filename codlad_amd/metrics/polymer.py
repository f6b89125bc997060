"""Chain statistics of disordered ensembles (csrc/polymer_kernels.hip; the arithmetic and its bounds are stated in
include/codlad_hip.h): per structure and per sequence separation the sums of r^2 and 1 / r over an ordered atom selection
(chain_sums), the hydrodynamic radius by Kirkwood's double sum (hydrodynamic_radius), the gyration tensor with its shape
descriptors and the end-to-end distance (gyration_tensor), the internal distance scaling R(s) of an ensemble
(distance_scaling) and the Flory exponent fitted to it (flory_fit).  The selection is ORDERED: position k of `sel` is chain
position k (the CA atoms in sequence order, say).  Every sum has one order, a function of the selection's size alone: the
bits repeat from call to call and a structure's results do not depend on the other structures of the call."""
import numpy as np
import torch

from .. import _lib
from . import _inputs
from .ensemble import _moments

POLYMER_MAX_SEL, POLYMER_SPLIT_MAX_N, POLYMER_SPLIT_MIN_SEL = _lib.POLYMER_MAX_SEL, _lib.POLYMER_SPLIT_MAX_N, _lib.POLYMER_SPLIT_MIN_SEL

__all__ = ["POLYMER_MAX_SEL", "POLYMER_SPLIT_MAX_N", "POLYMER_SPLIT_MIN_SEL", "chain_sums", "hydrodynamic_radius",
           "gyration_tensor", "distance_scaling", "flory_fit"]


def _chain(xyz, sel, what, m_min):
    """(the checked structures, sel on the device, n_sel, m); ValueError unless m_min <= m <= POLYMER_MAX_SEL."""
    x = _inputs.structures(xyz, f"{what}: xyz")
    sel, n_sel = _inputs.selection(sel, x.shape[1], x.device)
    m = n_sel or x.shape[1]
    if not m_min <= m <= POLYMER_MAX_SEL:
        raise ValueError(f"{what}: {m_min} .. {POLYMER_MAX_SEL} selected atoms, got {m}")
    return x, sel, n_sel, m


def _f64(v, dev):
    return torch.tensor(float(v), dtype=torch.float64, device=dev)


def _used(finite, w, what):
    """The structures that enter an ensemble value - finite, and of positive weight where there are weights - as a bool
    mask, their weights (1 without weights) and their number; ValueError when there is none."""
    use = finite if w is None else finite & (w > 0)
    n = int(use.sum())
    if n == 0:
        raise ValueError(f"{what}: no finite structure of positive weight")
    wu = torch.where(use, torch.ones_like(use, dtype=torch.float64) if w is None else w, torch.zeros((), dtype=torch.float64, device=use.device))
    return use, wu, n


def chain_sums(xyz, sel=None):
    """xyz [N, n_atoms, 3] (device), sel: the ordered selection of m atoms (default: all) -> dict of device tensors, the
    raw sums of codlad_chain_sums:
      sep_r2 float64 [N, m - 1]    column s - 1: the sum of r^2(k, k + s) over the m - s pairs at separation s
      sep_inv float64 [N, m - 1]   the same sum of 1 / r
      inv_sum float64 [N]          the sum of sep_inv over s, in ascending s: half of Kirkwood's double sum
      finite bool [N]              False: a selected atom has a NaN or +-inf coordinate - the structure's rows are NaN
    Coincident selected atoms are no error: +inf in that separation of sep_inv and in inv_sum."""
    return _chain_launch(*_chain(xyz, sel, "chain_sums", 2))


def _chain_launch(x, sel, n_sel, m):
    N, n, dev = x.shape[0], x.shape[1], x.device
    sep_r2 = torch.empty(N, m - 1, dtype=torch.float64, device=dev)
    sep_inv = torch.empty(N, m - 1, dtype=torch.float64, device=dev)
    inv_sum = torch.empty(N, dtype=torch.float64, device=dev)
    finite = _inputs.flags(N, dev)
    p = _lib.ptr
    rc = _lib.lib().codlad_chain_sums(p(x), N, n, p(sel), n_sel, p(sep_r2), p(sep_inv), p(inv_sum), p(finite), _lib.stream_ptr(dev))
    _lib.check(rc, "codlad_chain_sums")
    return dict(sep_r2=sep_r2, sep_inv=sep_inv, inv_sum=inv_sum, finite=finite.to(torch.bool))


def hydrodynamic_radius(xyz, sel=None, weights=None):
    """The hydrodynamic radius of every structure by Kirkwood's double sum over the m selected atoms,
      1 / Rh = (1 / m^2) sum_{i != j} 1 / r_ij = 2 inv_sum / m^2
    -> dict: rh float64 [N] (A, device), inv_rh float64 [N], finite bool [N], and the ensemble value rh_mean (0-dim) = 1 /
    (weighted mean of inv_rh over the finite structures of positive weight): the harmonic mean, which is what diffusion
    measures.  weights [N]: finite, >= 0, one at least > 0; None: equal weights.
    This is the Kirkwood BEAD estimate on the chosen atoms - any selection; one bead per residue at CA is the usual
    choice - without hydration, bead radii or masses: no shell model, no empirical Rg -> Rh conversion.  Coincident beads
    give Rh = 0 (1 / r = inf); a structure that is not finite gives NaN and is left out of rh_mean."""
    x, sel, n_sel, m = _chain(xyz, sel, "hydrodynamic_radius", 2)
    w = _inputs.weights(weights, x.shape[0], x.device, "hydrodynamic_radius", need_positive=True)
    out = _chain_launch(x, sel, n_sel, m)
    inv_rh = 2.0 * out["inv_sum"] / _f64(m * m, x.device)          # a tensor divisor: the correctly rounded quotient
    use, wu, _n = _used(out["finite"], w, "hydrodynamic_radius")
    mean = torch.where(use, wu * inv_rh, torch.zeros_like(inv_rh)).sum() / wu.sum()
    return dict(rh=1.0 / inv_rh, inv_rh=inv_rh, finite=out["finite"], rh_mean=1.0 / mean)


def gyration_tensor(xyz, sel=None):
    """xyz [N, n_atoms, 3] (device) -> dict of float64 device tensors, per structure, over the atoms `sel` (default: all):
      tensor [N, 6]       (xx, yy, zz, xy, xz, yz) of sum (x - c)(x - c)^T / m about the unweighted centroid c
      eig [N, 3]          its eigenvalues l1 <= l2 <= l3 (cyclic Jacobi on the device, clamped at 0)
      rg2 [N]             l1 + l2 + l3, the squared radius of gyration
      asphericity [N]     l3 - (l1 + l2) / 2
      acylindricity [N]   l2 - l1
      kappa2 [N]          1 - 3 (l1 l2 + l2 l3 + l3 l1) / (l1 + l2 + l3)^2, the relative shape anisotropy: 0 sphere .. 1 rod
      prolateness [N]     prod (3 l_i - T) / T^3 with T = l1 + l2 + l3: -1/4 (oblate) .. 2 (prolate)
      ree [N]             the distance between the first and the last selected atom
      finite bool [N]     False: a selected atom has a NaN or +-inf coordinate - everything above is NaN
    The four shape numbers are float64 torch on the device from eig; they are NaN where rg2 is 0 (all atoms coincide)."""
    x, sel, n_sel, m = _chain(xyz, sel, "gyration_tensor", 1)
    N, n, dev = x.shape[0], x.shape[1], x.device
    mom = _moments(x, N, n, sel, n_sel)
    tensor = torch.empty(N, 6, dtype=torch.float64, device=dev)
    eig = torch.empty(N, 3, dtype=torch.float64, device=dev)
    ree = torch.empty(N, dtype=torch.float64, device=dev)
    finite = _inputs.flags(N, dev)
    p = _lib.ptr
    rc = _lib.lib().codlad_gyration(p(x), N, n, p(sel), n_sel, p(mom), p(tensor), p(eig), p(ree), p(finite), _lib.stream_ptr(dev))
    _lib.check(rc, "codlad_gyration")
    l1, l2, l3 = eig[:, 0], eig[:, 1], eig[:, 2]
    T = (l1 + l2) + l3
    nan = torch.full((), float("nan"), dtype=torch.float64, device=dev)

    def shaped(v):
        return torch.where(T > 0, v, nan)
    return dict(tensor=tensor, eig=eig, rg2=T, asphericity=shaped(l3 - (l1 + l2) / 2.0), acylindricity=shaped(l2 - l1),
                kappa2=shaped(1.0 - 3.0 * ((l1 * l2 + l2 * l3) + l3 * l1) / (T * T)),
                prolateness=shaped((3.0 * l1 - T) * (3.0 * l2 - T) * (3.0 * l3 - T) / (T * T * T)), ree=ree,
                finite=finite.to(torch.bool))


def distance_scaling(xyz, sel=None, weights=None):
    """The internal distance scaling of an ensemble: xyz [N, n_atoms, 3] (device) -> dict: sep int64 [m - 1] = 1 .. m - 1,
    r_rms float64 [m - 1] (both on the device),
      r_rms[s] = sqrt(sum_j w_j sep_r2[j, s] / (W (m - s)))
    over the finite structures of positive weight, W the sum of their weights (None: equal weights); n_struct = their
    number.  The quotient is taken by tensors (correctly rounded)."""
    x, sel, n_sel, m = _chain(xyz, sel, "distance_scaling", 2)
    w = _inputs.weights(weights, x.shape[0], x.device, "distance_scaling", need_positive=True)
    out = _chain_launch(x, sel, n_sel, m)
    use, wu, n = _used(out["finite"], w, "distance_scaling")
    sep = torch.arange(1, m, dtype=torch.int64, device=x.device)
    num = torch.where(use[:, None], wu[:, None] * out["sep_r2"], torch.zeros((), dtype=torch.float64, device=x.device)).sum(0)
    return dict(sep=sep, r_rms=torch.sqrt(num / (wu.sum() * (m - sep).to(torch.float64))), n_struct=n)


def flory_fit(sep, r_rms, s_min=5, s_max=None, r0=None):
    """The Flory exponent of R(s) = R0 s^nu: the closed-form least-squares fit of ln R = ln R0 + nu ln s over the
    separations s_min <= s <= s_max (default s_max: m // 2 with m = len(sep) + 1; the long separations have few pairs and
    feel the chain ends), in float64 on the host (one short copy of sep and r_rms, as distance_scaling returns them) ->
    dict: nu, r0 (floats), n_points.  With r0 given only nu is fitted (nu = sum x (y - ln r0) / sum x^2, x = ln s).
    nu is about 1/3 for a compact globule, 1/2 for an ideal chain and 0.6 for an expanded coil.  Separations whose R is
    not a positive finite number are left out; ValueError when fewer than two separations remain."""
    def host(v):
        return np.asarray(v.detach().cpu().numpy() if torch.is_tensor(v) else v, dtype=np.float64).reshape(-1)
    s, R = host(sep), host(r_rms)
    if s.shape != R.shape:
        raise ValueError(f"flory_fit: sep and r_rms must have one length, got {s.shape[0]} and {R.shape[0]}")
    s_max = (s.shape[0] + 1) // 2 if s_max is None else s_max
    with np.errstate(invalid="ignore"):
        keep = (s >= s_min) & (s <= s_max) & (s > 0) & np.isfinite(R) & (R > 0)
    if int(keep.sum()) < 2:
        raise ValueError(f"flory_fit: fewer than two separations in {s_min} .. {s_max} to fit, got {int(keep.sum())}")
    x, y = np.log(s[keep]), np.log(R[keep])
    if r0 is None:
        xm, ym = x.mean(), y.mean()
        nu = float(((x - xm) * (y - ym)).sum() / ((x - xm) ** 2).sum())
        r0_fit = float(np.exp(ym - nu * xm))
    else:
        r0_fit = _inputs.positive(r0, "r0", "flory_fit")
        nu = float((x * (y - np.log(r0_fit))).sum() / (x * x).sum())
    return dict(nu=nu, r0=r0_fit, n_points=int(keep.sum()))
