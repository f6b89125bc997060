"""De-normalise -> VQ lookup -> IC decoder -> internal coordinates to Cartesian, on CPU
(TEST INFRASTRUCTURE, see oracle/__init__.py).

Follows reference utils/dataset_module.py:230-256 (get_norm_feature, norm_in=False),
utils/vq_module.py:56-71 (nearest code), models/vae_model.py:830-838, :759-764 (latent_decode,
decoder), :375-412 / :467-503 (IC_Decoder_angle / IC_Decoder), models/gcn_nn.py:54-70, :222-271,
:316-338, :372-380 (make_directed, preprocess_r, radial basis, envelope, message) and
utils/utils_ic.py:197-268 (rotation_matrix, add_atom_to_xyz, ic_to_xyz).
"""
import math

import torch
import torch.nn.functional as F


def denormalise(x, mean, std):
    """dataset_module.py:253: x * std + mean."""
    return x * std + mean


def vq_lookup(z, codebook):
    """vq_module.py:61-71: argmin of |z|^2 + |e|^2 - 2 z.e, first index on ties."""
    zf = z.reshape(-1, codebook.shape[1])
    d = (torch.sum(zf ** 2, dim=1, keepdim=True) + torch.sum(codebook ** 2, dim=1)
         - 2.0 * torch.einsum("bd,nd->bn", zf, codebook))
    idx = torch.argmin(d, dim=1)
    return F.embedding(idx, codebook).view(z.shape), idx


def codebook_of(sd):
    if "quantize.embeddings" in sd:
        return sd["quantize.embeddings"]
    return sd["quantize._codebook.embed"][0]


def _lin(sd, name, x):
    return F.linear(x, sd[name + ".weight"], sd[name + ".bias"])


def _swish(x):
    return x * torch.sigmoid(x)


def _seq(sd, p, x):
    """nn.Sequential(swish, Linear(.1), swish, Linear(.3))."""
    return _lin(sd, f"{p}.3", _swish(_lin(sd, f"{p}.1", _swish(x))))


def directed(nbr):
    """make_directed (gcn_nn.py:54-64): a list that already holds rows with i > j and rows with j > i is the directed
    graph as given (receiver in column 0, sender in column 1); anything else is mirrored."""
    gtr_ij = bool((nbr[:, 0] > nbr[:, 1]).any())
    gtr_ji = bool((nbr[:, 1] > nbr[:, 0]).any())
    if not (gtr_ij and gtr_ji):
        nbr = torch.cat([nbr, nbr.flip(1)], dim=0)
    return nbr


def edge_geometry(cg_xyz, nbr, dtype=None):
    """-> (directed pairs [E,2], dist [E], rbf [E,15], env [E]) in `dtype` (default: that of cg_xyz).
    The radial-basis coefficients n pi / 21 are the model's float32 buffer (gcn_nn.py:231-240 registers
    `torch.arange(1, 16).float() * pi / cutoff`), cast up as the weights are - not recomputed in float64."""
    dtype = cg_xyz.dtype if dtype is None else dtype
    cg_xyz = cg_xyz.to(dtype)
    nb = directed(nbr)
    r_ij = cg_xyz[nb[:, 1]] - cg_xyz[nb[:, 0]]
    dist = ((r_ij ** 2 + 1e-8).sum(-1)) ** 0.5                           # gcn_nn.py:66-70
    n = torch.arange(1, 16).float()
    coef = (n * math.pi / 21.0).to(dtype)
    one, zero = torch.ones((), dtype=dtype), torch.zeros((), dtype=dtype)
    sd_ = dist.unsqueeze(-1)
    num = torch.where(sd_ == 0, coef, torch.sin(coef * sd_))
    den = torch.where(sd_ == 0, one, sd_)
    rbf = torch.where(sd_ >= 21.0, zero, num / den)                     # gcn_nn.py:231-255
    env = 0.5 * (torch.cos(math.pi * dist / 21.0) + 1)
    env = torch.where(dist >= 21.0, torch.zeros_like(env), env)         # gcn_nn.py:265-271
    return nb, dist, rbf, env


def block_phi(sd, blk, S, p="equivaraintconv"):
    """inv_dense of message block `blk` on the raw state: phi [M,40], one row per sending residue."""
    mp = f"{p}.message_blocks.{blk}"
    return _lin(sd, f"{mp}.inv_dense.1", _swish(_lin(sd, f"{mp}.inv_dense.0", S)))


def message_sum(sd, blk, phi, cg_xyz, nbr, p="equivaraintconv", geometry=None):
    """The message sum of block `blk` alone: v[n] = sum over incoming edges (j -> n), in list order, of
    phi[j] * (dist_embed(rbf(d)) * envelope(d)), in the dtype of `sd` (phi and cg_xyz are cast to it).  `phi` may be a
    device's own rows: the sum is then held to a reference that shares its input."""
    dtype = sd[f"{p}.message_blocks.{blk}.dist_embed.block.1.weight"].dtype
    nb, _dist, rbf, env = edge_geometry(cg_xyz, nbr, dtype) if geometry is None else geometry
    phi = phi.to(dtype)
    w_s = _lin(sd, f"{p}.message_blocks.{blk}.dist_embed.block.1", rbf) * env.reshape(-1, 1)
    return torch.zeros_like(phi).index_add_(0, nb[:, 0], phi[nb[:, 1]] * w_s)     # scatter_add


def dense_update(sd, blk, S, v, p="equivaraintconv"):
    return S + _seq(sd, f"{p}.dense_blocks.{blk}", v)


def heads(sd, S, cg_z, angle=False, p="equivaraintconv"):
    """The output heads on the final state S [M,40] -> ic [M,13,3]; bond lengths (and, for the non-angle model, the
    side-chain angles) are table rows."""
    bb_dist = F.embedding(cg_z, sd[f"{p}.backbone_dist.weight"]).unsqueeze(-1)
    sc_dist = F.embedding(cg_z, sd[f"{p}.sidechain_dist.weight"]).unsqueeze(-1)
    bb_angle = _seq(sd, f"{p}.backbone_angle", S)
    bb_tors = _seq(sd, f"{p}.backbone_torsion", torch.cat([S, bb_angle], dim=-1))
    if angle:                                                           # vae_model.py:403-407
        sc_angle = _seq(sd, f"{p}.sidechain_angle", S)
        T = torch.cat([S, sc_angle], dim=-1)
    else:                                                               # vae_model.py:475,496-498
        sc_angle = F.embedding(cg_z, sd[f"{p}.sidechain_angle.weight"])
        T = S
    for i in range(4):
        T = T + _seq(sd, f"{p}.sidechain_torsion_blocks.{i}", T)
    sc_tors = _seq(sd, f"{p}.final_torsion", T)
    ic_bb = torch.cat([bb_dist, bb_angle.unsqueeze(-1), bb_tors.unsqueeze(-1)], dim=-1)
    ic_sc = torch.cat([sc_dist, sc_angle.unsqueeze(-1), sc_tors.unsqueeze(-1)], dim=-1)
    return torch.cat([ic_bb, ic_sc], dim=-2)


def ic_decode(sd, z_q_flat, cg_z, cg_xyz, nbr_undirected, angle=False, p="equivaraintconv", latent_is_state=False,
              taps=None, phi_sub=None):
    """z_q_flat [M,3] (restore_shape'd), cg_z [M], cg_xyz [M,3], nbr [E,2] j>i -> ic [M,13,3].
    latent_is_state: the C2 model (GenZProt.decoder, vae_model.py:556-561) hands its 36-wide latent to the IC decoder
    as it is - no map_out.
    Runs in the dtype of `sd`: z_q_flat and cg_xyz are cast to it, so a float64 state dict (tests/conditioning.py
    to_dtype) gives a float64 evaluation throughout.  One thing stays float32 then, as it does in the model: the
    radial-basis coefficients n pi / 21 are a float32 buffer, cast up like the weights (edge_geometry).
    taps: a dict that receives "S0" (the state after map_out and res_embed) and per message block i "phi{i}" [M,40],
    "v{i}" (the message sum) and "S{i+1}" (the state after the block); heads(sd, taps["S4"], ...) is the result.
    phi_sub: {block: phi [M,40]} used in place of the block's own phi (a device's rows, cast to the dtype)."""
    dtype = sd[f"{p}.res_embed.weight"].dtype
    z_q_flat = z_q_flat.to(dtype)
    S = z_q_flat if latent_is_state else _lin(sd, "map_out", z_q_flat)  # vae_model.py:762
    S = torch.cat([S, F.embedding(cg_z, sd[f"{p}.res_embed.weight"])], dim=-1)
    geometry = edge_geometry(cg_xyz, nbr_undirected, dtype)
    if taps is not None:
        taps["S0"] = S
    for i in range(4):
        phi = block_phi(sd, i, S, p)
        if phi_sub is not None and i in phi_sub:
            phi = phi_sub[i].to(dtype)
        v = message_sum(sd, i, phi, cg_xyz, nbr_undirected, p, geometry=geometry)
        S = dense_update(sd, i, S, v, p)
        if taps is not None:
            taps[f"phi{i}"], taps[f"v{i}"], taps[f"S{i + 1}"] = phi, v, S
    return heads(sd, S, cg_z, angle, p)


def latent_decode(sd, latent, batch, angle=False):
    """vae_model.py:830-838: latent [B,L,3] (already de-normalised) -> (idx, ic [B*L,13,3])."""
    z_q, idx = vq_lookup(latent, codebook_of(sd))
    num = batch["num_CGs"].tolist()
    flat = torch.cat([z_q[b, :n] for b, n in enumerate(num)], dim=0)    # gcn_nn.py:45-52
    ic = ic_decode(sd, flat, batch["CG_nxyz"][:, 0].long(), batch["CG_nxyz"][:, 1:],
                   batch["CG_nbr_list"], angle=angle)
    return idx, ic


# ----------------------------------------------------------------------------------------------
def _rotation(axis, angle):
    """utils_ic.py:197-210 (Euler-Rodrigues)."""
    axis = axis / torch.sqrt((axis * axis).sum(-1)).unsqueeze(-1)
    a = torch.cos(angle / 2).squeeze(-1)
    res = -axis * torch.sin(angle / 2)
    b, c, d = res[..., 0], res[..., 1], res[..., 2]
    rx = torch.stack((a * a + b * b - c * c - d * d, 2 * (b * c - a * d), 2 * (b * d + a * c)), -1)
    ry = torch.stack((2 * (b * c + a * d), a * a + c * c - b * b - d * d, 2 * (c * d - a * b)), -1)
    rz = torch.stack((2 * (b * d - a * c), 2 * (c * d + a * b), a * a + d * d - b * b - c * c), -1)
    return torch.stack((rx, ry, rz), -2)


def _place(ic, atom1, atom2, atom3):
    """utils_ic.py:213-239."""
    dist, ang, dih = ic[..., 0:1], ic[..., 1:2], ic[..., 2:3]
    a = atom2 - atom1
    b = atom2 - atom3
    a = torch.where(a == 0.0, a + 1e-8, a)
    b = torch.where(b == 0.0, b + 1e-8, b)
    d = torch.absolute(dist) * a / torch.sqrt((a * a).sum(-1)).unsqueeze(-1)
    normal = torch.cross(a, b, dim=-1)
    d = torch.matmul(_rotation(normal, ang), d.unsqueeze(-1))
    d = torch.matmul(_rotation(a, dih), d).squeeze(-1)
    return atom1 + d


def ic_to_xyz(og_cg_nxyz, ic, info):
    """utils_ic.py:242-268.  og_cg_nxyz [B,L+2,4], ic [B,L,13,3] -> [B,n_atoms,3].
    (Restated without the reference's .squeeze(), which only changes shapes at B=1 or L=1.)"""
    permute, atom_idx, orders = info
    ca = og_cg_nxyz[:, :, 1:]
    mid, prv, nxt = ca[:, 1:-1], ca[:, :-2], ca[:, 2:]
    N = _place(ic[:, :, 0], mid, prv, nxt)
    C = _place(ic[:, :, 1], mid, nxt, prv)
    O = _place(ic[:, :, 2], C, mid, N)
    atoms = torch.stack((O, N, C, mid), dim=2)
    B = ca.shape[0]
    for i in range(10):
        def pick(col):
            ix = orders[i, :, col].reshape(1, -1, 1, 1).repeat(B, 1, 1, 3)
            return torch.gather(atoms, 2, ix)[:, :, 0]
        new = _place(ic[:, :, 3 + i], pick(2), pick(1), pick(0))
        atoms = torch.cat([atoms, new.unsqueeze(2)], dim=2)
    return atoms.reshape(B, -1, 3)[:, atom_idx, :][:, permute, :]
