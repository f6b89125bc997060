"""the e3nn encoder / CG prior.

e3nn is absent (not installed, not vendored by the reference), so the restated tensor product (oracle/e3nn_lite.py) is
"parity unpinned" against e3nn itself.  What reference-held DATA does pin (fixture tests/golden/c2_prior_e3nn.npz, made
by tools/gen_golden.py g14 from the shipped C2 checkpoint and datasets/miu_and_sigma):
  * the non-trivial Wigner 3j symbols, against the buffers e3nn itself saved in the checkpoint;
  * the instruction set, through the checkpoint's fc.3 widths (weight_numel 192 / 288 / 384) and output masks;
  * the whole prior - harmonics, path coefficients, weight order, mean aggregation - statistically: the TRAINED prior
    evaluated by the restatement on protein-shaped inputs reproduces the per-channel mean and spread of its latent over the
    PED set as the reference recorded them, and wrong conventions visibly do not.
CPU tests hold the oracle to that; GPU tests hold the HIP kernels to the oracle.
"""
import math

import numpy as np
import pytest
import torch

from codlad_amd import synth
from oracle import e3nn_lite as e3
from tests import cases

FIX = np.load(cases.npz_path("c2_prior_e3nn"))


def _prior_sd():
    return {k[len("prior_net."):]: torch.from_numpy(FIX[k]) for k in FIX.files if k.startswith("prior_net.")}


def _rot(seed):
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(4, generator=g, dtype=torch.float64)
    a, b, c, d = (q / q.norm()).tolist()
    return torch.tensor([[a * a + b * b - c * c - d * d, 2 * (b * c - a * d), 2 * (b * d + a * c)],
                         [2 * (b * c + a * d), a * a - b * b + c * c - d * d, 2 * (c * d - a * b)],
                         [2 * (b * d - a * c), 2 * (c * d + a * b), a * a - b * b - c * c + d * d]], dtype=torch.float64)


# ------------------------------------------------------------------------------------------------ CPU: the oracle's pins
def test_wigner_symbols_equal_the_buffers_e3nn_left_in_the_shipped_checkpoint():
    assert float((e3.wigner_3j(1, 1, 1) - torch.from_numpy(FIX["w3j_1_1_1"]).double()).abs().max()) < 1e-7
    assert float((e3.wigner_3j(1, 2, 1) - torch.from_numpy(FIX["w3j_1_2_1"]).double()).abs().max()) < 1e-7
    # the trivial ones in closed form
    assert torch.allclose(e3.wigner_3j(1, 1, 0)[:, :, 0], torch.eye(3, dtype=torch.float64) / math.sqrt(3))
    assert torch.allclose(e3.wigner_3j(0, 1, 1)[0], torch.eye(3, dtype=torch.float64) / math.sqrt(3))
    assert torch.allclose(e3.wigner_3j(1, 0, 1)[:, 0], torch.eye(3, dtype=torch.float64) / math.sqrt(3))


def test_instruction_set_matches_the_checkpoint_widths():
    tps = e3.layer_tps()
    for l, tp in enumerate(tps):
        assert tp.weight_numel == int(FIX[f"weight_numel_{l}"]) == synth.TP_WEIGHT_NUMEL[l]
        assert e3.irreps_dim(tp.out) == FIX[f"output_mask_{l}"].shape[0] and bool(FIX[f"output_mask_{l}"].all())
    assert [len(tp.instr) for tp in tps] == [2, 6, 10]


def test_harmonics_and_symbols_are_consistent_intertwiners():
    """Y_l(R x) = D_l(R) Y_l(x) defines D_l; every 3j symbol must commute with (D_l1, D_l2, D_l3) - which ties the l = 2
    harmonics (order, signs) to the l = 1 ones through the pinned w3j(1, 2, 1)."""
    R = _rot(3)
    x = torch.randn(300, 3, dtype=torch.float64, generator=torch.Generator().manual_seed(1))
    Y, YR = e3.spherical_harmonics(2, x), e3.spherical_harmonics(2, x @ R.T)
    D, off = {}, {0: 0, 1: 1, 2: 4}
    for l in (0, 1, 2):
        A, B = Y[:, off[l]:off[l] + 2 * l + 1], YR[:, off[l]:off[l] + 2 * l + 1]
        D[l] = torch.linalg.lstsq(A, B).solution.T
        assert float((A @ D[l].T - B).abs().max()) < 1e-12
        assert float((D[l] @ D[l].T - torch.eye(2 * l + 1, dtype=torch.float64)).abs().max()) < 1e-12
        assert abs(float(Y[:, off[l]:off[l] + 2 * l + 1].pow(2).sum(-1).mean()) - (2 * l + 1)) < 1e-9   # 'component'
    assert float((D[1] - R).abs().max()) < 1e-12
    for ls in [(1, 1, 0), (1, 1, 1), (1, 2, 1), (0, 1, 1), (1, 0, 1)]:
        C = e3.wigner_3j(*ls)
        Cr = torch.einsum("ijk,ai,bj,ck->abc", C, D[ls[0]], D[ls[1]], D[ls[2]])
        assert float((Cr - C).abs().max()) < 1e-12, ls
    # the l = 2 harmonics ARE the pinned symbol contracted with two copies of the direction (up to a positive factor)
    u = torch.nn.functional.normalize(x, dim=-1)
    y2 = torch.einsum("imk,ni,nk->nm", e3.wigner_3j(1, 2, 1), u, u)
    ratio = (Y[:, 4:] * y2).sum() / (y2 * y2).sum()
    assert float(ratio) > 0 and float((Y[:, 4:] - ratio * y2).abs().max()) < 1e-9


@pytest.mark.parametrize("depth", [0, 1, 2])
def test_conv_layer_is_equivariant(depth):
    """Rotating and inverting the geometry and the vector features rotates / flips the layer's output blocks:
    0e invariant, 1o a vector, 1e a pseudo-vector, 0o a pseudo-scalar."""
    sd = {k: v.double() for k, v in synth.prior_state_dict(5).items()}
    tp = e3.layer_tps()[depth]
    g = torch.Generator().manual_seed(depth)
    n = 40
    xyz = torch.randn(n, 3, generator=g, dtype=torch.float64) * 6
    h = torch.randn(n, 12 * (depth + 1), generator=g, dtype=torch.float64)
    pairs = torch.nonzero(torch.triu(torch.cdist(xyz, xyz) < 9.0, diagonal=1))
    nb = e3.make_directed(pairs)

    def run(xyz_, h_):
        r = xyz_[nb[:, 1]] - xyz_[nb[:, 0]]
        sh = e3.spherical_harmonics(2, r)
        ea = torch.cat([torch.randn(nb.shape[0], 12, generator=torch.Generator().manual_seed(9), dtype=torch.float64),
                        h_[nb[:, 0], :12], h_[nb[:, 1], :12]], -1)
        return e3.tp_conv_layer(sd, f"cg_conv_layers.{depth}", tp, h_, (nb[:, 0], nb[:, 1]), ea, sh)

    def act(feat, R, parity):
        out = feat.clone()
        if feat.shape[1] >= 24:
            out[:, 12:24] = (feat[:, 12:24].reshape(-1, 4, 3) @ R.T).reshape(-1, 12) * parity          # 1o
        if feat.shape[1] >= 36:
            out[:, 24:36] = (feat[:, 24:36].reshape(-1, 4, 3) @ R.T).reshape(-1, 12)                   # 1e
        if feat.shape[1] >= 48:
            out[:, 36:48] = feat[:, 36:48] * parity                                                    # 0o
        return out

    base = run(xyz, h)
    for R, parity in ((_rot(11), 1.0), (torch.eye(3, dtype=torch.float64), -1.0), (_rot(12), -1.0)):
        got = run((xyz @ R.T) * parity, act(h, R, parity))
        assert float((got - act(base, R, parity)).abs().max()) < 1e-10


def _prior_stats(mutate=None):
    sd = _prior_sd()
    mus, sig = [], []
    for L, seed in ((87, 1), (129, 2), (46, 3)):
        batch = synth.make_batch(synth.make_protein(L, seed, n_frames=2))
        mu, sg = e3.prior_forward(sd, batch["CG_nxyz"][:, 0].long(), batch["CG_nxyz"][:, 1:], batch["CG_nbr_list"])
        mus.append(mu); sig.append(sg)
    mu, sg = torch.cat(mus), torch.cat(sig)
    ym, ys = torch.from_numpy(FIX["PED_C2_y_mean"]), torch.from_numpy(FIX["PED_C2_y_std"])
    total = (mu.std(0) ** 2 + sg.mean(0) ** 2).sqrt()          # spread of y = mu + sigma eps
    return float(((mu.mean(0) - ym) / ys).abs().max()), float((total / ys).min()), float((total / ys).max())


def test_trained_prior_reproduces_the_recorded_latent_statistics():
    """The reference recorded, per channel, the mean and std of the C2 prior's latent over the PED set
    (datasets/miu_and_sigma/PED_C2_y_{mean,std}.pt).  The trained prior run through the restatement on synthetic
    protein-shaped CA traces lands on them: every channel's mean within half a recorded std, every channel's spread
    within 0.8 .. 1.25 of the recorded one.  Getting a convention wrong does not: without the path coefficients or with
    a sum instead of the mean the spread is off by 10^4, with the instructions ordered by output 4.5 x, with
    'norm'-normalised harmonics 0.63 x (checked below for two of them)."""
    dmean, lo, hi = _prior_stats()
    assert dmean < 0.6 and 0.8 < lo and hi < 1.25, (dmean, lo, hi)
    init = e3.TensorProduct.__init__
    try:
        def by_output(self, *a):
            init(self, *a)
            z = sorted(zip(self.instr, self.coeff), key=lambda t: (t[0][2], t[0][0], t[0][1]))
            self.instr, self.coeff = [i for i, _ in z], [c for _, c in z]
        e3.TensorProduct.__init__ = by_output
        assert _prior_stats()[2] > 3.0

        def no_coeff(self, *a):
            init(self, *a)
            self.coeff = [1.0] * len(self.coeff)
        e3.TensorProduct.__init__ = no_coeff
        assert _prior_stats()[2] > 100.0
    finally:
        e3.TensorProduct.__init__ = init


def test_module_mirrors_keep_the_checkpoint_layout():
    """`get_vae_model("C2")`'s structure: every tensor of the shipped checkpoint's prior has its namesake, same shape, in
    the mirror; the full models load a state dict that also carries e3nn's own `.tp.` buffers (skipped) strictly."""
    from codlad_amd.utils.model_module import build_vae, load_decoder_state
    c2 = build_vae("C2")
    own = c2.state_dict()
    for k in FIX.files:
        if k.startswith("prior_net."):
            assert k in own and tuple(own[k].shape) == FIX[k].shape, k
    # 175 keys = the shipped checkpoint's key set without e3nn's own `.tp.` buffers and the legacy dist_filter (checked against the file)
    assert len(own) == 175 and sum(1 for k in own if k.startswith("encoder.")) == 69 and sum(1 for k in own if k.startswith("prior_net.")) == 26
    sd = {k: v.clone() for k, v in own.items()}
    sd["prior_net.cg_conv_layers.1.tp.output_mask"] = torch.ones(36)
    sd["prior_net.cg_conv_layers.1.tp._compiled_main_left_right._w3j_1_1_1"] = torch.zeros(3, 3, 3)
    sd["equivaraintconv.message_blocks.0.dist_filter.weight"] = torch.zeros(1)
    load_decoder_state(c2, sd)
    with pytest.raises(RuntimeError):
        load_decoder_state(c2, {k: v for k, v in sd.items() if k != "prior_net.mu.0.weight"})
    n6 = build_vae("N6", with_encoder=True)
    assert "encoder.dense.2.bias" in n6.state_dict() and "map_in.weight" in n6.state_dict()
    n6_dec = build_vae("N6")
    load_decoder_state(n6_dec, n6.state_dict())              # a decoder-only model skips the encoder side of a full one


def _old_gaussian_smearing(dist, start, stop, n):
    """oracle/e3nn_lite.py's gaussian_smearing before it followed its input's dtype."""
    offset = torch.linspace(start, stop, n)
    coeff = -0.5 / (offset[1] - offset[0]).item() ** 2
    return torch.exp(coeff * (dist.view(-1, 1) - offset.view(1, -1)) ** 2)


def _old_graph(z, xyz, nbr_list, max_radius, n_embed, sh_lmax, in_edge_features=4):
    """oracle/e3nn_lite.py's _graph before it followed its input's dtype."""
    nb = e3.make_directed(nbr_list)
    edge_attr = torch.cat([z[nb[:, 0]].unsqueeze(-1).float(), z[nb[:, 1]].unsqueeze(-1).float(),
                           torch.zeros(nb.shape[0], in_edge_features)], -1)
    r = xyz[nb[:, 1]] - xyz[nb[:, 0]]
    edge_attr = torch.cat([edge_attr, _old_gaussian_smearing(r.norm(dim=-1), 0.0, max_radius, n_embed)], -1)
    return (nb[:, 0], nb[:, 1]), edge_attr, e3.spherical_harmonics(sh_lmax, r)


def _g15_encoder_inputs(name):
    L, frames, wseed = cases.E3NN_ENCODER_CASES[name]
    prot = synth.make_protein(L, 50 + L, n_frames=frames)
    batch, atoms = synth.make_batch(prot), synth.make_atoms(prot, seed=L)
    return synth.encoder_state_dict(wseed), (atoms["nxyz"][:, 0], atoms["nxyz"][:, 1:], batch["CG_nxyz"][:, 0].long(),
                                             batch["CG_nxyz"][:, 1:], atoms["CG_mapping"], atoms["nbr_list"], batch["CG_nbr_list"])


def _g15_prior_inputs(name):
    L, frames, wseed, weights = cases.E3NN_PRIOR_CASES[name]
    batch = synth.make_batch(synth.make_protein(L, 40 + L, n_frames=frames))
    sd = _prior_sd() if weights == "trained_c2" else synth.prior_state_dict(wseed)
    return sd, (batch["CG_nxyz"][:, 0].long(), batch["CG_nxyz"][:, 1:], batch["CG_nbr_list"])


def _up(args):
    return tuple(a.double() if a.is_floating_point() else a for a in args)


def test_oracle_follows_the_input_dtype_and_float32_is_bit_unchanged():
    """prior_forward / encoder_forward in float32 return the bits they returned when _graph and gaussian_smearing were
    hard-coded to float32 (the old expressions are kept above), and with float64 weights and inputs every tensor a conv
    layer sees is float64."""
    psd, pargs = _g15_prior_inputs("seeded_L46x2")
    esd, eargs = _g15_encoder_inputs("L12")
    mu, sg = e3.prior_forward(psd, *pargs)
    lat = e3.encoder_forward(esd, *eargs)
    graph, smear = e3._graph, e3.gaussian_smearing
    e3._graph, e3.gaussian_smearing = _old_graph, _old_gaussian_smearing
    try:
        mu_old, sg_old = e3.prior_forward(psd, *pargs)
        lat_old = e3.encoder_forward(esd, *eargs)
    finally:
        e3._graph, e3.gaussian_smearing = graph, smear
    assert mu.dtype == lat.dtype == torch.float32
    assert torch.equal(mu, mu_old) and torch.equal(sg, sg_old) and torch.equal(lat, lat_old)
    # float64 throughout
    seen, orig = [], e3.tp_conv_layer

    def spy(sd, prefix, tp, node_attr, edge_index, edge_attr, edge_sh, out_nodes=None):
        out = orig(sd, prefix, tp, node_attr, edge_index, edge_attr, edge_sh, out_nodes)
        seen.append({node_attr.dtype, edge_attr.dtype, edge_sh.dtype, out.dtype})
        return out

    e3.tp_conv_layer = spy
    try:
        mu64, sg64 = e3.prior_forward({k: v.double() for k, v in psd.items()}, *_up(pargs))
        lat64 = e3.encoder_forward({k: v.double() for k, v in esd.items()}, *_up(eargs))
    finally:
        e3.tp_conv_layer = orig
    assert len(seen) == 13 and all(s == {torch.float64} for s in seen)
    assert mu64.dtype == sg64.dtype == lat64.dtype == torch.float64
    assert rel_err(mu, mu64) < 2e-6 and rel_err(sg, sg64) < 2e-6 and rel_err(lat, lat64) < 2e-6


def test_conv_reference_returns_what_the_references_layers_returned():
    """e3.conv_reference - one `Encoder.conv` call restated from the oracle's parts, the reference the per-launch GPU
    tests compare with - fed the node states the float32 oracle's layers start from, returns the ten per-layer updates the
    reference's own TensorProductConvLayer.forward produced (g15_encoder_L12), in float32 and in float64."""
    from tests import e3nn_parity as ep
    gold = np.load(cases.npz_path("g15_encoder_L12"))
    sd, args = _g15_encoder_inputs("L12")
    G = ep.encoder_graphs(*args)
    states, upd = ep.oracle_layer_states(sd, args)
    done = []
    for l, (ha, hc) in enumerate(states):
        for call in ep.encoder_layer_calls(G, l, ha, hc):
            key = "upd_" + call["layer"].replace(".", "_")
            r32, r64 = ep.reference_of(sd, call, torch.float32), ep.reference_of(sd, call, torch.float64)
            assert r32.dtype == torch.float32 and r64.dtype == torch.float64 and tuple(r32.shape) == gold[key].shape
            assert rel_err(r32, torch.from_numpy(gold[key])) < 2e-6 and rel_err(r64, torch.from_numpy(gold[key])) < 2e-6, key
            assert rel_err(r32, upd[key]) < 2e-6, key
            done.append(key)
    assert sorted(done) == sorted(k for k in gold.files if k.startswith("upd_")) and len(done) == 10


# ------------------------------------------------------------------------------------------------ GPU: HIP vs the oracle
DEV = "cuda:0"


def rel_err(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


@pytest.mark.gpu
@pytest.mark.parametrize("weights", ["trained_c2", "synthetic"])
@pytest.mark.parametrize("L", [5, 46, 129])
def test_hip_prior_matches_oracle(weights, L):
    from codlad_amd.encoder import Prior
    sd = _prior_sd() if weights == "trained_c2" else synth.prior_state_dict(31)
    batch = synth.make_batch(synth.make_protein(L, 40 + L, n_frames=2))
    cg_z, cg_xyz, nbr = batch["CG_nxyz"][:, 0].long(), batch["CG_nxyz"][:, 1:], batch["CG_nbr_list"]
    mu_ref, sg_ref = e3.prior_forward(sd, cg_z, cg_xyz, nbr)
    prior = Prior(sd, DEV)
    mu, sg = prior.forward(cg_z, cg_xyz, nbr)
    assert rel_err(mu, mu_ref) < 1e-5 and rel_err(sg, sg_ref) < 1e-5
    mu2, sg2 = prior.forward(cg_z, cg_xyz, nbr)                    # beads with > 64 neighbours at L = 129: several steps per node
    assert torch.equal(mu, mu2) and torch.equal(sg, sg2)


@pytest.mark.gpu
@pytest.mark.parametrize("L,frames", [(46, 2), (87, 1)])
def test_hip_encoder_matches_oracle(L, frames):
    from codlad_amd.encoder import Encoder
    sd = synth.encoder_state_dict(32)
    prot = synth.make_protein(L, 50 + L, n_frames=frames)
    batch = synth.make_batch(prot)
    atoms = synth.make_atoms(prot, seed=L)
    args = (atoms["nxyz"][:, 0], atoms["nxyz"][:, 1:], batch["CG_nxyz"][:, 0].long(), batch["CG_nxyz"][:, 1:],
            atoms["CG_mapping"], atoms["nbr_list"], batch["CG_nbr_list"])
    ref = e3.encoder_forward(sd, *args)
    got = Encoder(sd, DEV).forward(*args)
    assert got.shape == ref.shape == (L * frames, 36)
    assert rel_err(got, ref) < 1e-5
    # the weights packed once per layer (codlad_tp_conv_pack) or by every workgroup: the same bits
    unpacked = Encoder(sd, DEV)
    unpacked.pack_weights = False
    assert torch.equal(unpacked.forward(*args), got)
    # a frame's latent does not depend on what shares the batch
    if frames == 2:
        one = synth.make_atoms(prot, frame_ids=[1], seed=L)
        b1 = synth.make_batch(prot, frame_ids=[1])
        alone = Encoder(sd, DEV).forward(one["nxyz"][:, 0], one["nxyz"][:, 1:], b1["CG_nxyz"][:, 0].long(),
                                         b1["CG_nxyz"][:, 1:], one["CG_mapping"], one["nbr_list"], b1["CG_nbr_list"])
        assert torch.equal(alone, got[L:])


# The reference's own forward passes (g15, tools/gen_golden.py: e3nnEncoder.forward / e3nnPrior.forward /
# TensorProductConvLayer.forward over the restated primitives) against the device directly, not through the oracle.
@pytest.mark.gpu
@pytest.mark.parametrize("name", list(cases.E3NN_ENCODER_CASES))
def test_hip_encoder_matches_the_references_g15_latent(name):
    from codlad_amd.encoder import Encoder
    sd, args = _g15_encoder_inputs(name)
    gold = torch.from_numpy(np.load(cases.npz_path(f"g15_encoder_{name}"))["latent"])
    got = Encoder(sd, DEV).forward(*args)
    assert tuple(got.shape) == tuple(gold.shape)
    assert rel_err(got, gold) < 1e-5, rel_err(got, gold)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(cases.E3NN_PRIOR_CASES))
def test_hip_prior_matches_the_references_g15_mu_and_sigma(name):
    from codlad_amd.encoder import Prior
    sd, args = _g15_prior_inputs(name)
    gold = np.load(cases.npz_path(f"g15_prior_{name}"))
    mu, sg = Prior(sd, DEV).forward(*args)
    assert tuple(mu.shape) == gold["mu"].shape and tuple(sg.shape) == gold["sigma"].shape
    e_mu, e_sg = rel_err(mu, torch.from_numpy(gold["mu"])), rel_err(sg, torch.from_numpy(gold["sigma"]))
    assert e_mu < 1e-5 and e_sg < 1e-5, (e_mu, e_sg)


@pytest.mark.gpu
def test_hip_conv_layers_match_the_references_g15_updates():
    """The ten per-layer updates the reference's TensorProductConvLayer.forward returned on the small encoder case, each
    against ONE `Encoder.conv` launch (accumulate into zeros) fed the float32 oracle's node states of that layer."""
    from codlad_amd.encoder import Encoder
    from tests import e3nn_parity as ep
    gold = np.load(cases.npz_path("g15_encoder_L12"))
    sd, args = _g15_encoder_inputs("L12")
    G = ep.encoder_graphs(*args)
    states, _upd = ep.oracle_layer_states(sd, args)
    enc = Encoder(sd, DEV)
    done = []
    for l, (ha, hc) in enumerate(states):
        for call in ep.encoder_layer_calls(G, l, ha, hc):
            key = "upd_" + call["layer"].replace(".", "_")
            got = ep.device_conv(enc, call)
            err = rel_err(got, torch.from_numpy(gold[key]))
            print(f"g15 {key}: {err:.2e} of the array's maximum")
            assert tuple(got.shape) == gold[key].shape and err < 1e-5, (key, err)
            done.append(key)
    assert sorted(done) == sorted(k for k in gold.files if k.startswith("upd_")) and len(done) == 10


@pytest.mark.gpu
@pytest.mark.parametrize("depth", [0, 1, 2])
def test_hip_conv_layer_is_equivariant_at_full_size(depth):
    """The size-independent property on the largest graph of BASELINE's PED set (the L = 129 protein's 10 frames: ~10 700
    atoms, ~1.1 M directed edges, too large for the oracle in a test): rotating / inverting the coordinates and the vector
    features rotates / flips the layer's output blocks - 0e invariant, 1o a vector, 1e a pseudo-vector, 0o a pseudo-scalar -
    to fp32 accuracy, on the matrix-pipe kernel."""
    from codlad_amd.encoder import Encoder, directed_csr
    enc = Encoder(synth.encoder_state_dict(36), DEV)
    prot = synth.make_protein(129, 1003, n_frames=10)
    atoms = synth.make_atoms(prot, seed=3)
    xa, ta = atoms["nxyz"][:, 1:].to(DEV).contiguous(), atoms["nxyz"][:, 0].to(DEV).contiguous()
    na = xa.shape[0]
    csr = directed_csr(atoms["nbr_list"].to(DEV), na)
    assert int(csr[0][-1]) > 1_000_000
    g = torch.Generator(device=DEV).manual_seed(depth)
    h = torch.randn(na, 12 * (depth + 1), generator=g, device=DEV)

    def run(xyz_, h_):
        out = torch.empty(na, 12 * (depth + 2), device=DEV)
        enc.conv(f"atom_conv_layers.{depth}", depth, csr, xyz_.contiguous(), xyz_.contiguous(), ta, ta, 1.0, 14.0,
                 "atom_edge_embedding", 14, h_.contiguous(), h_.contiguous(), True, out, False, 64)
        return out

    def act(feat, R, parity):
        out = feat.clone()
        if feat.shape[1] >= 24:
            out[:, 12:24] = (feat[:, 12:24].reshape(-1, 4, 3) @ R.T).reshape(-1, 12) * parity          # 1o
        if feat.shape[1] >= 36:
            out[:, 24:36] = (feat[:, 24:36].reshape(-1, 4, 3) @ R.T).reshape(-1, 12)                   # 1e
        if feat.shape[1] >= 48:
            out[:, 36:48] = feat[:, 36:48] * parity                                                    # 0o
        return out

    base = run(xa, h)
    assert bool(torch.isfinite(base).all())
    scale = float(base.abs().max())
    for R64, parity in ((_rot(21), 1.0), (_rot(22), -1.0)):
        R = R64.float().to(DEV)
        got = run((xa @ R.T) * parity, act(h, R, parity))
        assert float((got - act(base, R, parity)).abs().max()) < 2e-5 * scale


@pytest.mark.gpu
def test_isolated_nodes_and_empty_graphs():
    """Receivers without a single edge (mean over nothing = 0: the node keeps its padded features) and a graph without any
    edge at all, against the oracle."""
    from codlad_amd.encoder import Prior
    sd = synth.prior_state_dict(35)
    batch = synth.make_batch(synth.make_protein(12, 77, n_frames=1))
    cg_z, cg_xyz = batch["CG_nxyz"][:, 0].long(), batch["CG_nxyz"][:, 1:].clone()
    cg_xyz[3] += 500.0                                          # one bead far from all others
    nbr = synth.cg_nbr_list(cg_xyz, 21.0)
    assert not ((nbr == 3).any()) and nbr.shape[0] > 10
    for pairs in (nbr, nbr[:0]):
        mu_ref, sg_ref = e3.prior_forward(sd, cg_z, cg_xyz, pairs)
        mu, sg = Prior(sd, DEV).forward(cg_z, cg_xyz, pairs)
        assert bool(torch.isfinite(mu).all()) and rel_err(mu, mu_ref) < 1e-5 and rel_err(sg, sg_ref) < 1e-5


@pytest.mark.gpu
def test_receiver_csr_kernel():
    """codlad_receiver_csr against the reference's make_directed + a stable grouping by receiver (gcn_nn.py:54-64)."""
    from codlad_amd.encoder import receiver_csr
    g = torch.Generator().manual_seed(4)
    n = 700
    x = torch.randn(n, 3, generator=g) * 6
    und = synth.cg_nbr_list(x, 5.0)                                  # j > i, row-major
    assert und.shape[0] > 2000

    def expect(pairs, both):
        d = torch.cat([pairs, pairs.flip(1)], 0) if both else pairs
        return [sorted(d[d[:, 0] == a, 1].tolist()) for a in range(n)]

    cases_ = [(und, 0, True), (torch.cat([und, und.flip(1)], 0), 0, False), (und.flip(1), 0, True), (und, 1, False),
              (torch.stack([torch.randint(0, 50, (n,), generator=g), torch.arange(n)], 1), 1, False),
              (torch.tensor([[3, 5]]), 0, True)]
    for pairs, mode, both in cases_:
        ptr, snd = receiver_csr(pairs.to(DEV), n, mode)
        ptr, snd = ptr.cpu(), snd.cpu()
        want = expect(pairs, both)
        assert ptr[0] == 0 and int(ptr[-1]) == sum(len(w) for w in want)
        for a in range(n):
            assert snd[ptr[a]:ptr[a + 1]].tolist() == want[a], a
    # a node with more than 64 neighbours, and determinism of the whole thing
    star = torch.stack([torch.zeros(300, dtype=torch.int64), torch.arange(1, 301)], 1)
    p1, s1 = receiver_csr(star.to(DEV), 301, 0)
    p2, s2 = receiver_csr(star.to(DEV), 301, 0)
    assert torch.equal(p1, p2) and torch.equal(s1, s2) and s1[:300].tolist() == list(range(1, 301))


@pytest.mark.gpu
@pytest.mark.parametrize("variant", [0, 1, 2])
@pytest.mark.parametrize("scale", [1.0, 30.0, 1.0 / 30.0])
def test_tp_conv_variants_and_weight_magnitudes(variant, scale):
    """codlad_tp_conv's kernels (CODLAD_OPT_TP_CONV_VARIANT: 0 = all graphs on the matrix-pipe kernel, 1 = all on the
    scalar-operand kernel, 2 = matrix pipe for the intra-level graphs only) against the oracle, also with fc weights thirty
    times larger / smaller than the initialisation's (the matrix-pipe kernel splits weights and activations into fp16
    halves behind fixed power-of-two scales: hidden activations and per-edge weights then span 2^-10 .. 2^10)."""
    from codlad_amd import _lib
    from codlad_amd.encoder import Encoder, Prior
    sd = {k: (v * scale if ".fc." in k and k.endswith("weight") else v) for k, v in synth.encoder_state_dict(33).items()}
    psd = {k: (v * scale if ".fc." in k and k.endswith("weight") else v) for k, v in synth.prior_state_dict(34).items()}
    prot = synth.make_protein(46, 71, n_frames=2)
    batch = synth.make_batch(prot)
    atoms = synth.make_atoms(prot, seed=9)
    args = (atoms["nxyz"][:, 0], atoms["nxyz"][:, 1:], batch["CG_nxyz"][:, 0].long(), batch["CG_nxyz"][:, 1:],
            atoms["CG_mapping"], atoms["nbr_list"], batch["CG_nbr_list"])
    ref = e3.encoder_forward(sd, *args)
    mu_ref, sg_ref = e3.prior_forward(psd, args[2], args[3], args[6])
    _lib.set_option(_lib.OPT_TP_CONV_VARIANT, variant)
    try:
        got = Encoder(sd, DEV).forward(*args)
        mu, sg = Prior(psd, DEV).forward(args[2], args[3], args[6])
    finally:
        _lib.set_option(_lib.OPT_TP_CONV_VARIANT, 0)
    assert rel_err(got, ref) < 1e-5, rel_err(got, ref)
    assert rel_err(mu, mu_ref) < 1e-5 and rel_err(sg, sg_ref) < 1e-5


@pytest.mark.gpu
def test_genzprot_and_recon_models_run_end_to_end():
    """The module mirrors on the device: C2 (`get_latent_cg` -> `latent_decode` on the 36-wide latent, with the shipped
    prior's trained weights) and an N6 VQ-VAE with its encoder (`get_latent_wovq` -> `latent_decode`) against the oracle."""
    from codlad_amd.utils.model_module import build_vae, load_decoder_state
    from oracle import vae_decode as odec
    prot = synth.make_protein(46, 61, n_frames=2)
    batch = synth.make_batch(prot)
    batch.update(synth.make_atoms(prot, seed=3))
    dbatch = {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in batch.items()}
    # C2: trained prior, synthetic decoder
    c2 = build_vae("C2")
    sd = dict(c2.state_dict())
    sd.update({k: torch.from_numpy(FIX[k]) for k in FIX.files if k.startswith("prior_net.")})
    dsd = synth.decoder_state_dict(4322, angle=False)
    sd.update(dsd)
    load_decoder_state(c2, sd)
    c2 = c2.to(DEV).eval()
    g = torch.Generator(device=DEV).manual_seed(5)
    y, _, _, mask, num, mu, sigma = c2.get_latent_cg(dbatch, generator=g)
    mu_ref, sg_ref = e3.prior_forward(_prior_sd(), batch["CG_nxyz"][:, 0].long(), batch["CG_nxyz"][:, 1:],
                                      batch["CG_nbr_list"])
    assert rel_err(mu, mu_ref) < 1e-5 and rel_err(sigma, sg_ref) < 1e-5 and y.shape == (2, 46, 36) and bool(mask.all())
    _ic, ic_recon = c2.latent_decode(y, mask, dbatch)
    ic_ref = odec.ic_decode(dsd, y.reshape(-1, 36).cpu(), batch["CG_nxyz"][:, 0].long(), batch["CG_nxyz"][:, 1:],
                            batch["CG_nbr_list"], angle=False, latent_is_state=True)
    assert rel_err(ic_recon, ic_ref) < 2e-5
    # N6 with encoder: recon
    n6 = build_vae("N6", with_encoder=True)
    vsd = synth.vqvae_state_dict("N6", "PED", 4321)
    esd = synth.encoder_state_dict(778)
    full = dict(n6.state_dict())
    full.update(vsd)
    full.update({"encoder." + k: v for k, v in esd.items()})
    load_decoder_state(n6, full)
    n6 = n6.to(DEV).eval()
    lat, _, _, mask, _num, _, _ = n6.get_latent_wovq(dbatch)
    h_ref = e3.encoder_forward(esd, batch["nxyz"][:, 0], batch["nxyz"][:, 1:], batch["CG_nxyz"][:, 0].long(),
                               batch["CG_nxyz"][:, 1:], batch["CG_mapping"], batch["nbr_list"], batch["CG_nbr_list"])
    lat_ref = torch.nn.functional.linear(h_ref, vsd["map_in.weight"], vsd["map_in.bias"]).reshape(2, 46, 3)
    assert rel_err(lat, lat_ref) < 1e-5
    _ic, ic_recon = n6.latent_decode(lat, mask, dbatch)
    assert ic_recon.shape == (92, 13, 3) and bool(torch.isfinite(ic_recon).all())


@pytest.mark.gpu
def test_batch_lengths_are_read_once_and_never_stale():
    """models.vae_model.batch_lengths keeps a host copy of a batch's `num_CGs` per tensor.  A freed tensor's address is
    handed out again by the caching allocator - the next batch's lengths land where the last batch's were - so an entry
    keeps its tensor alive (the first version of the cache did not, and test.py decoded the L = 92 batch with L = 87's
    lengths)."""
    from codlad_amd.models.vae_model import batch_lengths
    for L in (87, 92, 46, 129, 87):
        t = torch.tensor([L, L], dtype=torch.int64, device=DEV)
        assert batch_lengths(t) == [L, L]
        assert batch_lengths(t) == [L, L]
        t[1] = 5                                    # in-place change: another version, another entry
        assert batch_lengths(t) == [L, 5]
        del t
    assert batch_lengths(torch.tensor([3, 4])) == [3, 4]          # host tensors are read directly
