"""Which edges of a structure have ill-conditioned quaternion features, decided from the reference's own formulas.

The reference's `_quaternions` (protein_mpnn_utils.py:369-395; oracle/denoiser.py `_quaternions`) turns the relative
rotation R = O_i^T O_j of two local frames into

    q = normalize( sign(s_k) * 0.5 * sqrt|r_k|  (k = 0..2),   0.5 * sqrt(relu(1 + trace R)) )

    r_k = 1 + (+-Rxx +-Ryy +-Rzz)            the three radicands
    s_k = R_ab - R_ba                        the three sign arguments

A square root has an unbounded derivative at 0 and sign() a jump there, so an edge whose r_k, 1 + trace(R) or s_k is
rounding noise (a self edge, a neighbour with a parallel frame, a frame that the 3.6-4.0 A window has partly zeroed)
gets features that no two evaluations agree on: fp32 and float64 of the reference itself differ there by up to 0.23 of
the tensor's maximum.  `edge_conditioning` restates those quantities in float64 from the coordinates alone - it never
sees the output of a kernel - and names the edges where one of them is that small.

The thresholds are validated by tests/test_fp64_oracle.py (on the edges called well-conditioned, the fp32 and float64
oracles agree within 2e-6 of the maximum; at most 10 % of a case's edges are called ill-conditioned), and may be
refined against that test only.
"""
import torch
import torch.nn.functional as F

from oracle import denoiser as oden

R_MIN = 1e-3          # |r_k| and |1 + trace R| below this: the square root amplifies rounding noise
S_MIN = 1e-5          # 0 < |s_k| below this: the sign is rounding noise ...
MAG_MIN = 1e-3        # ... and matters when the magnitude 0.5 sqrt|r_k| it multiplies exceeds this
MAX_ILL_SHARE = 0.10  # a case where more edges than this are ill-conditioned is no parity case


def edge_quantities(cg_xyz, E_idx):
    """cg_xyz [N,L,3], E_idx [N,L,K] -> dict of float64 tensors: r [N,L,K,3], s [N,L,K,3], tr1 [N,L,K] (= 1 + trace R)
    and R [N,L,K,3,3], as oracle/denoiser.py orientation_features / _quaternions form them."""
    X = cg_xyz.double()
    dX = X[:, 1:, :] - X[:, :-1, :]
    n = torch.norm(dX, dim=-1)
    dX = dX * ((3.6 < n) & (n < 4.0))[:, :, None]
    U = F.normalize(dX, dim=-1)
    u_2, u_1 = U[:, :-2, :], U[:, 1:-1, :]
    n_2 = F.normalize(torch.linalg.cross(u_2, u_1), dim=-1)
    o_1 = F.normalize(u_2 - u_1, dim=-1)
    O = torch.stack((o_1, n_2, torch.linalg.cross(o_1, n_2)), dim=2)
    O = F.pad(O.reshape(O.shape[0], O.shape[1], 9), (0, 0, 1, 2), "constant", 0)
    O_nb = oden.gather_nodes(O, E_idx).view(*E_idx.shape, 3, 3)
    O = O.view(O.shape[0], O.shape[1], 3, 3)
    R = torch.matmul(O.unsqueeze(2).transpose(-1, -2), O_nb)
    diag = torch.diagonal(R, dim1=-2, dim2=-1)
    Rxx, Ryy, Rzz = diag.unbind(-1)
    r = 1 + torch.stack([Rxx - Ryy - Rzz, -Rxx + Ryy - Rzz, -Rxx - Ryy + Rzz], -1)
    s = torch.stack([R[..., 2, 1] - R[..., 1, 2], R[..., 0, 2] - R[..., 2, 0], R[..., 1, 0] - R[..., 0, 1]], -1)
    return dict(r=r, s=s, tr1=1 + diag.sum(-1), R=R)


def edge_conditioning(cg_xyz, E_idx):
    """-> bool [N,L,K]: True where the edge's quaternion features are ill-conditioned (see the module docstring).
    An s_k that is exactly zero is structural (both entries are zeros of a masked frame) and not a noise sign."""
    q = edge_quantities(cg_xyz, E_idx)
    r, s = q["r"], q["s"]
    small_r = (r.abs() < R_MIN).any(-1)
    noise_sign = ((s != 0) & (s.abs() < S_MIN) & (0.5 * r.abs().sqrt() > MAG_MIN)).any(-1)
    small_w = q["tr1"].abs() < R_MIN
    return small_r | noise_sign | small_w


# ------------------------------------------------------------------------------------------------------------------
# shared by tests/test_fp64_oracle.py (CPU) and the per-edge / per-node GPU tests
# ------------------------------------------------------------------------------------------------------------------
def to_dtype(sd, dtype):
    """A state dict with every floating-point tensor cast to `dtype` (float64: the oracle then runs in float64)."""
    return {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in sd.items()}


def feature_geometries():
    """name -> (n_cg, n_frames, protein seed) of every geometry the per-edge feature test runs: the four DENOISER_CASES
    and the geometries of the two DDIM cases whose trajectories carry a wider bound (tests/ddim_cases.py)."""
    from tests import cases, ddim_cases
    geoms = dict(cases.DENOISER_CASES)
    for name in ("fwd_fixed_small_L46", "fwd_ddim10_L46"):
        _rev, L, B, seed = ddim_cases.DDIM_CASES[name][:4]
        geoms[name] = (L, B, seed)
    return geoms


def edge_state(sd, cg_xyz, mask, E_idx=None):
    """h_E0 = W_e(CA features) [N,L,K,128] and E_idx, in the dtype of `sd` (cg_xyz is cast to it)."""
    dtype = sd["W_e.weight"].dtype
    E, E_idx = oden.ca_features(sd, cg_xyz.to(dtype), mask.int(), E_idx=E_idx)
    return oden._lin(sd, "W_e", E), E_idx


def edge_row_error(a, b):
    """[N,L,K]: largest |a - b| of each edge row, as a fraction of the largest |b| of the case."""
    a, b = a.double(), b.double()
    return (a - b).abs().amax(-1) / b.abs().max()


def node_channel_error(a, b):
    """[..., C]: |a - b| per node and channel, each channel scaled by its own largest |b| over the case."""
    a, b = a.double(), b.double()
    return (a - b).abs() / b.abs().reshape(-1, b.shape[-1]).amax(0).clamp_min(1e-300)


# ------------------------------------------------------------------------------------------------------------------
# the per-edge comparison of a device's h_E0 rows (test_hip_parity.py::test_features_prepass_edge_by_edge)
# ------------------------------------------------------------------------------------------------------------------
WELL_FACTOR = 4.0     # "as good as the reference's fp32": the project's precedent (test_ic_decode_and_xyz)
WELL_FLOOR = 5e-7     # of the tensor's maximum: two units of the 22-bit hi + lo form h_E0 is stored in
ILL_BOUND = 3e-4      # of the tensor's maximum: what test_features_prepass holds the whole tensor to


def admissible_quaternions(r, s, tr1):
    """The quaternions of ONE edge (r [3], s [3], tr1 scalar, float64) that an evaluation in other arithmetic may
    arrive at by taking one of the reference's discontinuities the other way, and only where the rule above says the
    deciding quantity is rounding noise:
      sign(s_k) with 0 < |s_k| < S_MIN: either sign;
      relu(1 + trace R) with |1 + trace R| < R_MIN: w = 0 or w = sqrt|1 + trace R| / 2 (when the other three components
      vanish, F.normalize turns any w > 0 into 1 and w = 0 into the zero quaternion).
    -> [n, 4], the float64 value first."""
    mag = 0.5 * r.abs().sqrt()
    signs = [[torch.sign(s[k])] if not (0 < abs(float(s[k])) < S_MIN) else [torch.sign(s[k]), -torch.sign(s[k])]
             for k in range(3)]
    ws = [torch.relu(tr1).sqrt() / 2.0]
    if abs(float(tr1)) < R_MIN:
        ws.append(tr1.abs().sqrt() / 2.0 if float(tr1) <= 0 else torch.zeros_like(tr1))
    out = []
    for w in ws:
        for s0 in signs[0]:
            for s1 in signs[1]:
                for s2 in signs[2]:
                    out.append(F.normalize(torch.stack([s0 * mag[0], s1 * mag[1], s2 * mag[2], w]), dim=-1))
    return torch.stack(out)


def check_edge_rows(sd, cg_xyz, mask, got, got_idx, label, expected_other_way=()):
    """Every edge row of a device's h_E0 (`got` [N,L,K,128], neighbours `got_idx` [N,L,K]) against the float64 oracle's
    row of the same neighbour:
      well-conditioned edges   within WELL_FACTOR x max(e_ref, WELL_FLOOR), e_ref = the fp32 oracle's largest error on
                               such edges of this case;
      ill-conditioned edges    within max(ILL_BOUND, WELL_FACTOR x the fp32 oracle's own error on that edge), or - then
                               listed in `expected_other_way` as (structure, node, neighbour) - equal, within the
                               well-conditioned bound, to the float64 row recomputed with an `admissible_quaternions`.
    -> dict of the figures (for the assertion messages and DESIGN.md)."""
    sd64 = to_dtype(sd, torch.float64)
    taps = {}
    E64, _ = oden.ca_features(sd64, cg_xyz.double(), mask.int(), E_idx=got_idx, taps=taps)
    h64 = oden._lin(sd64, "W_e", E64)
    h32, _ = edge_state(sd, cg_xyz, mask, E_idx=got_idx)
    ill = edge_conditioning(cg_xyz, got_idx)
    share = float(ill.double().mean())
    assert share <= MAX_ILL_SHARE, f"{label}: {share:.1%} of the edges are ill-conditioned"
    e32, err = edge_row_error(h32, h64), edge_row_error(got, h64)
    e_ref = float(e32[~ill].max())
    well_bound = WELL_FACTOR * max(e_ref, WELL_FLOOR)
    worst_well = float(err[~ill].max())
    figures = dict(ill_share=share, n_ill=int(ill.sum()), e_ref=e_ref, well_ratio=worst_well / e_ref,
                   worst_ill=float(err[ill].max()))
    head = (f"{label}: {figures['n_ill']} ill-conditioned edges ({share:.1%}); worst well-conditioned edge "
            f"{worst_well:.2e} = {figures['well_ratio']:.2f} x e_ref ({e_ref:.2e})")
    k = int(err.masked_fill(ill, 0).argmax())
    assert worst_well <= well_bound, f"{head}: edge {tuple(int(v) for v in torch.unravel_index(torch.tensor(k), err.shape))}"
    over = ill & (err > torch.maximum(torch.tensor(ILL_BOUND, dtype=torch.float64), WELL_FACTOR * e32))
    q = edge_quantities(cg_xyz, got_idx)
    scale = h64.abs().max()
    other_way = []
    for e in (tuple(v) for v in over.nonzero().tolist()):
        quats = admissible_quaternions(q["r"][e], q["s"][e], q["tr1"][e])
        raw = taps["E_raw"][e].repeat(len(quats), 1)
        raw[:, -4:] = quats
        rows = oden._lin(sd64, "W_e", oden.embed_edges(sd64, raw))
        d = (rows - got[e].double()).abs().amax(-1) / scale
        what = (f"{head}: ill-conditioned edge {e} -> neighbour {int(got_idx[e])} is {float(err[e]):.2e} from float64 (fp32 "
                f"oracle: {float(e32[e]):.2e}); r_k {q['r'][e].tolist()}, s_k {q['s'][e].tolist()}, 1 + trace R "
                f"{float(q['tr1'][e]):.3e}; admissible quaternions {quats.tolist()} give rows {d.tolist()} from the device's")
        assert float(d[1:].min() if len(d) > 1 else d.min()) <= well_bound, what
        other_way.append((e[0], e[1], int(got_idx[e])))
    # (one-sided: on which side the CPU's fp32 oracle lands, and with it the second term of the ill-conditioned bound,
    # may differ between CPUs' vector maths; an edge that needs this path must be written down)
    assert set(other_way) <= set(tuple(v) for v in expected_other_way), \
        f"{head}: edges that match float64 only with a discontinuity taken the other way: {other_way}, written down: " \
        f"{list(expected_other_way)}"
    figures["other_way"] = other_way
    figures["message"] = head
    return figures
