"""Ensemble analysis: the superposed RMSD of many pairs per launch (codlad_ens_*, csrc/ensemble_kernels.hip), alignment,
the pairwise RMSD table and the diversity score of reference test.py:37-95."""
import torch

from .. import _lib
from . import _inputs


def superposed_rmsd(a, b):
    """Minimal RMSD of two conformations [n_atoms, 3] after optimal rigid superposition (what mdtraj's md.rmsd
    returns for single-frame trajectories, reference test.py:52-53, 74-75): Kabsch, RMSD^2 = (|a|^2 + |b|^2 -
    2 (s1 + s2 + sign(det) s3)) / n with s the singular values of the 3x3 covariance of the centred coordinates.
    mdtraj is not available offline: PARITY UNPINNED (published algorithm)."""
    a = a.to(torch.float64) - a.to(torch.float64).mean(0)
    b = b.to(torch.float64) - b.to(torch.float64).mean(0)
    cov = (a.t() @ b).cpu()
    u, sv, vt = torch.linalg.svd(cov)
    d = torch.sign(torch.linalg.det(u @ vt))
    e0 = float((a * a).sum() + (b * b).sum())
    msd = max(e0 - 2.0 * float(sv[0] + sv[1] + d * sv[2]), 0.0) / a.shape[0]
    return msd ** 0.5


# --- Superposition on the device (codlad_ens_*, csrc/ensemble_kernels.hip): minimal RMSD under a proper rotation plus
# translation for many pairs per launch, fp64 after an exact conversion of the fp32 coordinates, deterministic sums.

_selection = _inputs.selection        # the name the tests and metrics/__init__.py reach it by


def _moments(x, n_conf, n_atoms, sel, n_sel):
    mom = torch.empty(n_conf, 4, dtype=torch.float64, device=x.device)
    _lib.check(_lib.lib().codlad_ens_moments(_lib.ptr(x), n_conf, n_atoms, _lib.ptr(sel), n_sel, _lib.ptr(mom),
                                             _lib.stream_ptr(x.device)), "codlad_ens_moments")
    return mom


def _pair_msd(A, B, pairs, sel, n_sel, squared, want_transform):
    """A [nA, n, 3], B [nB, n, 3] fp32 pools, pairs int32 [P, 2] (device) -> out [P] (and Rt [P, 12] or None)."""
    nA, n_atoms, nB, P = A.shape[0], A.shape[1], B.shape[0], pairs.shape[0]
    momA, momB = _moments(A, nA, n_atoms, sel, n_sel), _moments(B, nB, n_atoms, sel, n_sel)
    out = torch.empty(P, dtype=torch.float64, device=A.device)
    Rt = torch.empty(P, 12, dtype=torch.float64, device=A.device) if want_transform else None
    rc = _lib.lib().codlad_ens_pair_msd(_lib.ptr(A), _lib.ptr(momA), nA, _lib.ptr(B), _lib.ptr(momB), nB, n_atoms,
                                        _lib.ptr(sel), n_sel, _lib.ptr(pairs), P, int(bool(squared)), _lib.ptr(out),
                                        _lib.ptr(Rt), _lib.stream_ptr(A.device))
    _lib.check(rc, "codlad_ens_pair_msd")
    return out, Rt


def _one_to_one(a, b, what):
    """a [P, n, 3], b [P, n, 3] or [n, 3] -> fp32 pools and the pair list (k, k) or (k, 0)."""
    a = _inputs.structures(a, f"{what}: a")
    b = _inputs.structures(b, f"{what}: b", dims=b.dim() if b.dim() in (2, 3) else 3)
    if b.dim() == 2:
        b = b[None]
    P, n = a.shape[0], a.shape[1]
    if b.shape[1] != n or b.shape[0] not in (1, P) or b.device != a.device:
        raise ValueError(f"{what}: b {tuple(b.shape)} does not match a {tuple(a.shape)} (b is [P, n, 3] or [n, 3], same device)")
    k = torch.arange(P, dtype=torch.int32, device=a.device)
    pairs = torch.stack((k, k if b.shape[0] == P else torch.zeros_like(k)), 1).contiguous()
    return a, b, pairs


def superposed_rmsd_batch(a, b, sel=None, squared=False, return_transform=False):
    """Minimal RMSD of a[k] onto b[k] (b [P, n, 3]) or onto the one target b [n, 3], after the optimal proper rotation
    plus translation, for all P pairs in one launch set.  -> float64 [P] on the device (the msd with squared=True);
    with return_transform also float64 R [P, 3, 3] and t [P, 3] such that a @ R.T + t is superposed on b.  sel: the atom
    indices the fit and the RMSD use (default: all)."""
    a, b, pairs = _one_to_one(a, b, "superposed_rmsd_batch")
    sel, n_sel = _selection(sel, a.shape[1], a.device)
    out, Rt = _pair_msd(a, b, pairs, sel, n_sel, squared, return_transform)
    if return_transform:
        return out, Rt[:, :9].reshape(-1, 3, 3), Rt[:, 9:]
    return out


def superpose(a, b, sel=None):
    """-> fp32 [P, n, 3]: ALL atoms of every a[k] moved by the transform that superposes its atoms `sel` (default: all)
    on those of b[k] (or of the one target b [n, 3]); computed in fp64 and rounded once."""
    a, b, pairs = _one_to_one(a, b, "superpose")
    sel, n_sel = _selection(sel, a.shape[1], a.device)
    _out, Rt = _pair_msd(a, b, pairs, sel, n_sel, True, True)
    moved = torch.empty_like(a)
    _lib.check(_lib.lib().codlad_ens_apply(_lib.ptr(a), _lib.ptr(Rt), a.shape[0], a.shape[1], _lib.ptr(moved),
                                           _lib.stream_ptr(a.device)), "codlad_ens_apply")
    return moved


def pairwise_rmsd(x, sel=None):
    """x [G, F, n, 3] (members x frames) -> float64 [F, G, G]: the superposed RMSD of every pair of members of a frame.
    The upper triangle is computed (bit for bit what superposed_rmsd_batch gives for the pair) and mirrored; the diagonal
    is written as 0."""
    x = _inputs.structures(x, "pairwise_rmsd: x", dims=4)
    G, F, n = x.shape[:3]
    sel, n_sel = _selection(sel, n, x.device)
    mom = _moments(x, G * F, n, sel, n_sel)
    out = torch.empty(F, G, G, dtype=torch.float64, device=x.device)
    _lib.check(_lib.lib().codlad_ens_pairwise(_lib.ptr(x), _lib.ptr(mom), G, F, n, _lib.ptr(sel), n_sel, 0,
                                              _lib.ptr(out), _lib.stream_ptr(x.device)), "codlad_ens_pairwise")
    return out


def diversity_terms(gen, ref):
    """The two RMSD tables of the diversity score.  gen [G, F, n, 3] (or a list of G [F, n, 3]), ref [F, n, 3] ->
    float64 [G, F] RMSD of gen[g, p] to ref[p], and [G, F] RMSD of gen[g, p] to the UNALIGNED member mean gen.mean(0)[p]
    (the reference takes np.mean of the raw structures).  One launch set for both tables."""
    if isinstance(gen, (list, tuple)):
        gen = torch.stack([torch.as_tensor(g) for g in gen])
    gen = _inputs.structures(gen, "diversity_terms: gen", dims=4)
    ref = _inputs.structures(ref, "diversity_terms: ref")
    G, F, n = gen.shape[:3]
    if tuple(ref.shape) != (F, n, 3) or ref.device != gen.device:
        raise ValueError(f"diversity_terms: ref {tuple(ref.shape)} does not match gen {tuple(gen.shape)}")
    targets = torch.cat((ref, gen.mean(0)))                      # [2 F, n, 3]: pool B
    k = torch.arange(G * F, dtype=torch.int32, device=gen.device)
    p = k % F
    pairs = torch.cat((torch.stack((k, p), 1), torch.stack((k, p + F), 1))).contiguous()
    out, _ = _pair_msd(gen.reshape(G * F, n, 3), targets, pairs, None, 0, False, False)
    return out[:G * F].reshape(G, F), out[G * F:].reshape(G, F)


def compute_div(gen_structures, ref_structure):
    """Diversity score of reference test.py:37-95: 1 - (mean RMSD of every generated frame to the mean generated
    structure) / (mean RMSD of every generated frame to the reference frame).  gen_structures: list (ensemble members)
    of [n_frames, n_atoms, 3]; ref_structure [n_frames, n_atoms, 3].  CUDA tensors take the device path
    (diversity_terms: two launches for all G x F x 2 superpositions, one transfer of the final scalar); CPU tensors the
    float64 SVD loop over superposed_rmsd."""
    gen = [torch.as_tensor(g) for g in gen_structures]
    ref = torch.as_tensor(ref_structure)
    if ref.is_cuda:
        to_ref, to_mean = diversity_terms(gen, ref)
        return float(1.0 - to_mean.mean() / to_ref.mean())
    mean_gen = torch.stack(gen).mean(0)
    to_ref = [superposed_rmsd(g[p], ref[p]) for g in gen for p in range(g.shape[0])]
    to_mean = [superposed_rmsd(g[p], mean_gen[p]) for g in gen for p in range(g.shape[0])]
    return 1.0 - (sum(to_mean) / len(to_mean)) / (sum(to_ref) / len(to_ref))
