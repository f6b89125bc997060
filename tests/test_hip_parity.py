"""GPU parity: every HIP entry point of libcodlad_hip.so against the CPU oracle (and the
reference-generated goldens) on the same seeded inputs.  Run with `-m gpu` on an MI355X."""
import ctypes as C

import numpy as np
import pytest
import torch

from codlad_amd import _lib, engine, synth
from codlad_amd.diffusion_and_flow.schedule import Tables, named_betas, space_timesteps
from codlad_amd.engine import Decoder, Denoiser
from codlad_amd.weights import pack_block
from oracle import denoiser as oden
from oracle import sampler as osam
from oracle import vae_decode as odec
from tests import cases
from tests import conditioning as cond
from tests import ddim_cases

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EDGE_WIDE_DEFAULT = 22 * 256      # CODLAD_OPT_EDGE_WIDE_MAX_TILES as shipped (22 x the CU count)
NODE_QUAD_DEFAULT = 2 * 256      # CODLAD_OPT_NODE_QUAD_MAX_TILES as shipped (twice the CU count)
EDGE_UPD_DEFAULT = 0      # the library's default CODLAD_OPT_EDGE_UPD_VARIANT


def rel_err(a, b):
    a = torch.as_tensor(a).detach().cpu().double()
    b = torch.as_tensor(b).detach().cpu().double()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


@pytest.fixture(scope="module")
def sd():
    return synth.denoiser_state_dict(cases.WEIGHT_SEED)


@pytest.fixture(scope="module", params=["f16x3", "f16x4", "f32"])
def den(sd, request):
    """All contraction modes of the library: f16x3 (default) and f16x4 (fp16 hi/lo split operands on
    the f16 matrix pipe, 3 or 4 cross products, fp32 accumulate) and f32 (v_mfma_f32_32x32x2_f32)."""
    return Denoiser(sd, DEV, precision=request.param)


def tables(T):
    return Tables(named_betas("linear", 1000), space_timesteps(1000, str(T)))


def structures_of(den, prot):
    frames = torch.from_numpy(prot["xyz_full"])[:, 1:-1]
    z = torch.from_numpy(prot["z_full"])[1:-1]
    return den.prepare_structures([f for f in frames], [z for _ in frames])


# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("act", [0, 1])
def test_mfma_chain_primitive(act):
    """Packing order + C-layout chain: Y = act(W X + b) against fp64."""
    g = torch.Generator().manual_seed(5)
    W = torch.randn(128, 128, generator=g) / 11.0
    W[3, 7] = 2.5  # asymmetric marker
    b = torch.randn(128, generator=g)
    X = torch.randn(77, 128, generator=g)  # ragged tail: 77 = 2*32 + 13
    Y = torch.empty(77, 128, device=DEV)
    rc = _lib.lib().codlad_selftest_gemm128(_lib.ptr(pack_block(W).to(DEV)), _lib.ptr(b.to(DEV)),
                                            _lib.ptr(X.to(DEV)), 77, act, _lib.ptr(Y), None)
    _lib.check(rc, "selftest")
    torch.cuda.synchronize()
    ref = X.double() @ W.double().t() + b.double()
    if act:
        ref = torch.nn.functional.gelu(ref)
    assert rel_err(Y, ref) < 2e-6


@pytest.mark.parametrize("terms", [3, 4])
def test_split_f16_chain_primitive_is_exact_on_integers(terms):
    """Operand lane maps of v_mfma_f32_32x32x16_f16 + the hi/lo packing, checked with small integers
    (exact in fp16, so any mapping error shows as a wrong integer, not as rounding)."""
    from codlad_amd.weights import pack_block_h
    g = torch.Generator().manual_seed(6)
    W = torch.randint(-8, 9, (128, 128), generator=g).float()
    W[3, 7] = 100.0  # asymmetric marker
    b = torch.randint(-50, 50, (128,), generator=g).float()
    X = torch.randint(-16, 17, (77, 128), generator=g).float()
    Y = torch.empty(77, 128, device=DEV)
    Wh, bd, Xd = pack_block_h(W).to(DEV), b.to(DEV), X.to(DEV)
    rc = _lib.lib().codlad_selftest_gemm128_h(_lib.ptr(Wh), _lib.ptr(bd), _lib.ptr(Xd), 77, 0, terms, _lib.ptr(Y), None)
    _lib.check(rc, "selftest_h")
    torch.cuda.synchronize()
    assert torch.equal(Y.cpu(), X @ W.t() + b)
    # non-representable operands: hi/lo split keeps fp32-level accuracy; GELU fused into the input side
    W2 = torch.randn(128, 128, generator=g) / 11.0
    X2 = torch.randn(77, 128, generator=g) * 3.0
    W2h, X2d = pack_block_h(W2).to(DEV), X2.to(DEV)
    for act in (0, 1):
        rc = _lib.lib().codlad_selftest_gemm128_h(_lib.ptr(W2h), _lib.ptr(bd), _lib.ptr(X2d), 77, act, terms, _lib.ptr(Y), None)
        _lib.check(rc, "selftest_h")
        torch.cuda.synchronize()
        xin = torch.nn.functional.gelu(X2.double()) if act else X2.double()
        assert rel_err(Y, xin @ W2.double().t() + b.double()) < 2e-6


@pytest.mark.parametrize("name", list(cases.DENOISER_CASES))
def test_features_prepass(den, sd, name):
    L, B, seed = cases.DENOISER_CASES[name]
    prot, batch, x, t, mask = cases.denoiser_inputs(L, B, seed)
    st = structures_of(den, prot)
    torch.cuda.synchronize()
    cg_z, cg_xyz, m = oden.batch_to_dense(batch)
    E, E_idx = oden.ca_features(sd, cg_xyz, m.int())
    hE0 = torch.nn.functional.linear(E, sd["W_e.weight"], sd["W_e.bias"])
    K = min(64, L)
    got_idx = st.E_idx.cpu().view(B, L, 64)[:, :, :K].long()
    gold_idx = torch.from_numpy(np.load(cases.npz_path(f"g2_forward_{name}"))["E_idx"])
    # Neighbour lists must be identical up to the order of EXACTLY tied distances (the synthetic
    # traces have a fixed 3.8 A step, so d(i,i-1) == d(i,i+1) bit for bit is common, and
    # torch.topk leaves the order of equal keys unspecified): same neighbour set per residue and
    # the same, bitwise equal, ascending distance sequence.
    dX = cg_xyz[:, None, :, :] - cg_xyz[:, :, None, :]
    D = torch.sqrt(torch.sum(dX ** 2, 3) + 1e-6)
    # ... and up to 1 ulp: ATen's vectorised CPU sqrt is not correctly rounded (0.6 % of the
    # distances come out 1 ulp low), the kernel's is, so neighbours 1 ulp apart may swap places.
    for ref_idx in (E_idx, gold_idx):
        torch.testing.assert_close(torch.gather(D, 2, got_idx), torch.gather(D, 2, ref_idx),
                                   rtol=2.5e-7, atol=0)
        assert torch.equal(got_idx.sort(-1).values, ref_idx.sort(-1).values)
    assert bool((got_idx[:, :, 0] == torch.arange(L)[None]).all())         # self comes first
    # compare edge features edge by edge: bring the oracle's rows into this kernel's neighbour order
    perm = (got_idx[..., :, None] == E_idx[..., None, :]).float().argmax(-1)   # [B,L,K]
    hE0 = torch.gather(hE0, 2, perm[..., None].expand(-1, -1, -1, 128))
    got = engine.edge_rows(st.h_E0, split=den.split_edge_state).cpu().view(B, L, 64, 128)[:, :, :K]
    # The quaternion features are ill-conditioned by construction in the reference: for the self
    # edge (and any neighbour with a parallel frame) R = O_i^T O_j ~ I and the magnitudes
    # 0.5*sqrt(|1 + Rxx - Ryy - Rzz|) are the square root of rounding noise (~1e-4) with a noise
    # sign (protein_mpnn_utils.py:379-390).  They dominate the difference here; everything else
    # agrees to ~1e-6 and the denoiser output (test_denoiser_forward) to 1e-5.
    assert rel_err(got, hE0) < 3e-4
    err = (got - hE0).abs().amax(-1)                    # per edge
    assert float(err[:, :, 1:].median()) < 2e-6         # typical edge: fp32 rounding only


@pytest.mark.parametrize("name", list(cond.feature_geometries()))
def test_features_prepass_edge_by_edge(den, sd, name):
    """Every edge row of the device's h_E0 against the FLOAT64 oracle's row of the same neighbour - the maximum over
    edges, not the median - on the four DENOISER_CASES and the geometries of the two DDIM cases with a wider trajectory
    bound.  Which edges are ill-conditioned is decided from the reference's own formulas (tests/conditioning.py, at most
    10 % of a case); the bounds and the one admitted exception are those of cond.check_edge_rows."""
    L, B, seed = cond.feature_geometries()[name]
    prot, batch, x, t, mask = cases.denoiser_inputs(L, B, seed)
    st = structures_of(den, prot)
    torch.cuda.synchronize()
    cg_z, cg_xyz, m = oden.batch_to_dense(batch)
    K = min(64, L)
    got_idx = st.E_idx.cpu().view(B, L, 64)[:, :, :K].long()
    assert torch.equal(got_idx.sort(-1).values, oden.knn(cg_xyz, m.float())[1].sort(-1).values)     # same neighbour sets
    got = engine.edge_rows(st.h_E0, split=den.split_edge_state).cpu().view(B, L, 64, 128)[:, :, :K]
    fig = cond.check_edge_rows(sd, cg_xyz, m, got, got_idx, f"{name} {den.weights.precision}",
                               ddim_cases.FEATURE_DISCONTINUITY_EDGES.get(name, ()))
    print(fig["message"], "; worst ill-conditioned edge %.2e" % fig["worst_ill"], "; other way:", fig["other_way"])


def test_step_mods(den, sd):
    tv = [999, 500, 10, 0]
    mods = den.step_mods(tv).cpu()
    c = oden.t_embed(sd, torch.tensor(tv))
    sc = torch.nn.functional.silu(c)
    heads = [f"encoder_layers.{l}" for l in range(3)] + [f"decoder_layers.{l}" for l in range(3)] + ["W_out"]
    ref = torch.cat([torch.nn.functional.linear(sc, sd[f"{h}.adaLN_modulation.1.weight"],
                                                sd[f"{h}.adaLN_modulation.1.bias"]) for h in heads], dim=1)
    assert ref.shape == mods.shape
    assert rel_err(mods, ref) < 5e-6


@pytest.mark.parametrize("name", list(cases.DENOISER_CASES))
def test_denoiser_forward(den, sd, name):
    L, B, seed = cases.DENOISER_CASES[name]
    prot, batch, x, t, mask = cases.denoiser_inputs(L, B, seed)
    st = structures_of(den, prot)
    job = den.make_job(st, list(range(B)))
    out = den.forward(job, x.reshape(-1, 3).to(DEV), int(t[0])).cpu().view(B, L, 6)
    cg_z, cg_xyz, m = oden.batch_to_dense(batch)
    ref = oden.forward(sd, x, t, cg_xyz, cg_z, mask)
    assert rel_err(out, ref) < 1e-5
    gold = np.load(cases.npz_path(f"g2_forward_{name}"))
    assert rel_err(out, gold["out"]) < 1e-5
    if "enc0_hV" in gold.files:  # intermediate left in the workspace: last decoder h_V
        assert rel_err(job.hV.cpu().view(B, L, 128), gold["dec2_hV"]) < 1e-5


@pytest.mark.parametrize("L", [5, 31, 32, 33, 63, 64, 65, 200, 505, 2048])
def test_denoiser_forward_edge_lengths(den, sd, L):
    """Tile boundaries of the kernels: K = L < 32 (one partly filled column tile), 32/33 (second tile
    empty / one column), 63/64/65 (K saturates at 64), the longest Atlas test protein (505), and a chain four times
    that (the k-NN selection walks a 2 048-entry distance row per node)."""
    if L > 1000 and den.weights.precision != "f16x3":
        pytest.skip("the long chain runs in the default mode only (its oracle pass takes 20 s)")
    prot = synth.make_protein(L, 70 + L, n_frames=1)
    batch = synth.make_batch(prot)
    x = synth.gaussian((1, L, 3), 5)
    t = torch.tensor([777])
    st = structures_of(den, prot)
    job = den.make_job(st, [0])
    out = den.forward(job, x.reshape(-1, 3).to(DEV), 777).cpu().view(1, L, 6)
    cg_z, cg_xyz, m = oden.batch_to_dense(batch)
    ref = oden.forward(sd, x, t, cg_xyz, cg_z, m)
    assert bool(torch.isfinite(out).all())
    assert rel_err(out, ref) < 1e-5


def test_chain_longer_than_the_lds_distance_row_is_refused(den):
    """The k-NN selection keeps a node's distances to its whole chain in LDS; a chain that does not fit (beyond
    ~21 k residues) is an error code from the C ABI, not a wrong neighbour list."""
    L = 30000
    xyz = synth.gaussian((L, 3), 5) * 60.0
    with pytest.raises(RuntimeError, match="too long"):
        den.prepare_structures([xyz], [torch.zeros(L, dtype=torch.long)])


def test_edge_launch_probe_counts_the_launches_of_a_forward(den):
    """bench.py's measurement aid: with the probe on, one forward records 6 message and 3 edge-update launches (the
    layer-0 pair as the hoisted kind when the step-invariant terms are given), each with a positive duration."""
    import ctypes as C
    from codlad_amd import _lib
    lib = _lib.lib()
    prot = synth.make_protein(70, 9, n_frames=2)
    st = structures_of(den, prot)
    job = den.make_job(st, [0, 1, 1])
    x = synth.gaussian((job.n_nodes, 3), 2).to(DEV)
    lib.codlad_probe_edge_launches(1)
    den.forward(job, x, 10)
    lib.codlad_probe_edge_launches(0)
    den.forward(job, x, 10)                      # not recorded
    got = {}
    for kind in range(4):
        total = C.c_double(0.0)
        got[kind] = (lib.codlad_probe_read(kind, C.byref(total)), total.value)
    hoisted = st.E1 is not None
    assert [got[k][0] for k in range(4)] == ([5, 2, 1, 1] if hoisted else [6, 3, 0, 0])
    assert all(ms > 0 for n, ms in got.values() if n)


def test_ensemble_members_share_structure(den, sd):
    """Two samples on ONE structure == the same two samples on two copies of it."""
    L, B, seed = cases.DENOISER_CASES["L46_B2"]
    prot, batch, x, t, mask = cases.denoiser_inputs(L, B, seed)
    frames = torch.from_numpy(prot["xyz_full"])[:, 1:-1]
    z = torch.from_numpy(prot["z_full"])[1:-1]
    st1 = den.prepare_structures([frames[0]], [z])
    st2 = den.prepare_structures([frames[0], frames[0]], [z, z])
    xx = x.reshape(-1, 3).to(DEV)
    o1 = den.forward(den.make_job(st1, [0, 0]), xx, 321)
    o2 = den.forward(den.make_job(st2, [0, 1]), xx, 321)
    assert torch.equal(o1, o2)


def test_hoisted_layer0_edge_terms(den, sd):
    """The per-structure precomputation of encoder layer 0's edge contractions (E1) holds
    W1[:,128:256] @ h_E0 / W11[:,128:256] @ h_E0, and using it changes the forward only by rounding
    (fp32 summation order: P + Q + E1 instead of accumulating onto P + Q)."""
    pa = synth.make_protein(40, 5, n_frames=1)    # K = 40: one full and one partial column half
    pb = synth.make_protein(87, 6, n_frames=1)
    za, zb = torch.from_numpy(pa["z_full"])[1:-1], torch.from_numpy(pb["z_full"])[1:-1]
    xa, xb = torch.from_numpy(pa["xyz_full"])[0, 1:-1], torch.from_numpy(pb["xyz_full"])[0, 1:-1]
    st = den.prepare_structures([xa, xb], [za, zb])
    assert st.E1 is not None and tuple(engine.edge_rows(st.E1).shape) == (2, 127, 64, 128)
    K = torch.tensor([40] * 40 + [64] * 87, device=DEV)
    valid = (torch.arange(64, device=DEV)[None, :] < K[:, None])
    hE = engine.edge_rows(st.h_E0, split=den.split_edge_state).double()
    ex = den.weights.exponents["enc0"]
    for which, name in enumerate(["W1", "W11"]):
        W = sd[f"encoder_layers.0.{name}.weight"][:, 128:256].to(DEV).double()
        want = hE @ W.T
        # in the split-fp16 modes E1 carries the layer's block exponent (include/codlad_hip.h)
        scale = 1.0 if den.weights.precision == "f32" else 2.0 ** -ex["e1" if which == 0 else "e11"]
        got = engine.edge_rows(st.E1[which]).double() * scale
        # columns beyond K are never written, in h_E0 and in E1 alike: whatever the allocation held, possibly NaN, so they
        # are cut out (a product with 0 would keep a NaN)
        zero = torch.zeros((), dtype=torch.float64, device=DEV)
        err = torch.where(valid[..., None], (got - want).abs(), zero).max() / torch.where(valid[..., None], want.abs(), zero).max()
        assert float(err) < 2e-6, (name, float(err))
    plain = den.prepare_structures([xa, xb], [za, zb], hoist_layer0=False)
    assert plain.E1 is None
    x = synth.gaussian((40 + 87 + 87, 3), 99).to(DEV)
    o_h = den.forward(den.make_job(st, [0, 1, 1]), x, 700)
    o_p = den.forward(den.make_job(plain, [0, 1, 1]), x, 700)
    assert rel_err(o_h, o_p) < 2e-6


def test_ragged_job_matches_separate_jobs(den, sd):
    """Mixed lengths in one launch (no padding) == each length on its own."""
    pa = synth.make_protein(46, 12, n_frames=1)
    pb = synth.make_protein(87, 13, n_frames=1)
    za, zb = torch.from_numpy(pa["z_full"])[1:-1], torch.from_numpy(pb["z_full"])[1:-1]
    xa, xb = torch.from_numpy(pa["xyz_full"])[0, 1:-1], torch.from_numpy(pb["xyz_full"])[0, 1:-1]
    st = den.prepare_structures([xa, xb], [za, zb])
    job = den.make_job(st, [0, 1, 1])
    x = synth.gaussian((46 + 87 + 87, 3), 99).to(DEV)
    out = den.forward(job, x, 700)
    sa = den.prepare_structures([xa], [za])
    sb = den.prepare_structures([xb], [zb])
    oa = den.forward(den.make_job(sa, [0]), x[:46], 700)
    ob = den.forward(den.make_job(sb, [0, 0]), x[46:], 700)
    assert torch.equal(out, torch.cat([oa, ob]))


@pytest.mark.parametrize("name", list(cases.LOOP_CASES))
def test_sample_loop(den, sd, name):
    L, B, seed, T = cases.LOOP_CASES[name]
    prot, batch, _x, _t, mask = cases.denoiser_inputs(L, B, seed)
    z, eps = cases.loop_noise(T, B, L, seed)
    st = structures_of(den, prot)
    job = den.make_job(st, list(range(B)))
    x0 = den.sample(job, z.reshape(-1, 3).to(DEV), eps.reshape(T, -1, 3).to(DEV), tables(T))
    gold = np.load(cases.npz_path(f"g3_loop_{name}"))
    assert rel_err(x0.cpu().view(B, L, 3), gold["sample"]) < (1e-4 if T > 10 else 2e-5)
    if T <= 10:
        cg_z, cg_xyz, _ = oden.batch_to_dense(batch)
        ref = osam.p_sample_loop(sd, T, z, eps, cg_xyz, cg_z, mask, hoist_features=True)
        assert rel_err(x0.cpu().view(B, L, 3), ref) < 2e-5


def test_stepwise_equals_fused_loop(den, sd):
    """codlad_denoiser_forward + codlad_ddpm_update per step == codlad_sample_loop."""
    L, B, seed, T = cases.LOOP_CASES["L46_B2_T10"]
    prot, batch, _x, _t, mask = cases.denoiser_inputs(L, B, seed)
    z, eps = cases.loop_noise(T, B, L, seed)
    st = structures_of(den, prot)
    job = den.make_job(st, list(range(B)))
    tb = tables(T)
    x = z.reshape(-1, 3).to(DEV)
    for k, i in enumerate(range(T - 1, -1, -1)):
        out = den.forward(job, x, tb.timestep_map[i])
        x = den.ddpm_update(x, out, eps[k].reshape(-1, 3).to(DEV), tb, i)
    fused = den.sample(job, z.reshape(-1, 3).to(DEV), eps.reshape(T, -1, 3).to(DEV), tb)
    assert torch.equal(x, fused)


def test_jobs_on_separate_streams_equal_jobs_one_by_one(den):
    """Denoiser.sample_many: independent jobs enqueued on their own HIP streams (so that one job's kernels fill the CUs
    another's leave idle) give, job by job, the bits of `sample` - every job has its own workspace and status word."""
    T = 10
    tb = tables(T)
    jobs, xs, ns = [], [], []
    for k, name in enumerate(("L46_B2_T10", "L87_B2_T10") if "L87_B2_T10" in cases.LOOP_CASES else ("L46_B2_T10", "L46_B2_T10")):
        L, B, seed, _T = cases.LOOP_CASES[name]
        prot, _batch, _x, _t, _mask = cases.denoiser_inputs(L, B, seed + k)
        z, eps = cases.loop_noise(T, B, L, seed + k)
        jobs.append(den.make_job(structures_of(den, prot), list(range(B))))
        xs.append(z.reshape(-1, 3).to(DEV))
        ns.append(eps.reshape(T, -1, 3).to(DEV))
    one_by_one = [den.sample(j, x, n, tb) for j, x, n in zip(jobs, xs, ns)]
    together = den.sample_many(jobs, xs, ns, tb)
    torch.cuda.synchronize()
    for a, b in zip(one_by_one, together):
        assert torch.equal(a, b)


def test_split_f16_agrees_with_f32_mfma_and_survives_large_latents(sd):
    """The contraction modes agree to fp32 rounding level, also when the latent is far outside
    the trained range (|x| ~ 3000, as late steps of an untrained sampler produce): the only
    un-normalised operand, the neighbour sum S, is contracted with a power-of-two pre-scale so its
    fp16 halves do not overflow."""
    L, B, seed = cases.DENOISER_CASES["L87_B2"]
    prot, batch, x, t, mask = cases.denoiser_inputs(L, B, seed)
    outs = {}
    for prec in ("f32", "f16x4", "f16x3"):
        d = Denoiser(sd, DEV, precision=prec)
        st = structures_of(d, prot)
        job = d.make_job(st, list(range(B)))
        outs[prec] = [d.forward(job, (x * s).reshape(-1, 3).to(DEV), 500).cpu() for s in (1.0, 30.0, 3000.0)]
    for prec in ("f16x4", "f16x3"):
        for a, b in zip(outs["f32"], outs[prec]):
            assert bool(torch.isfinite(b).all())
            assert rel_err(b, a) < 5e-6


def test_deterministic_replay(den, sd):
    L, B, seed, T = cases.LOOP_CASES["L87_B2_T10"]
    prot, batch, _x, _t, mask = cases.denoiser_inputs(L, B, seed)
    z, eps = cases.loop_noise(T, B, L, seed)
    st = structures_of(den, prot)
    job = den.make_job(st, list(range(B)))
    a = den.sample(job, z.reshape(-1, 3).to(DEV), eps.reshape(T, -1, 3).to(DEV), tables(T))
    b = den.sample(job, z.reshape(-1, 3).to(DEV), eps.reshape(T, -1, 3).to(DEV), tables(T))
    assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------
def _vae_sd(vae_type, dataname, real_c2=False):
    vsd = synth.vqvae_state_dict(vae_type, dataname, cases.VAE_SEED, c2_like_map_out=real_c2)
    if real_c2:
        w = np.load(cases.npz_path("c2_decoder_weights"))
        for k in w.files:
            vsd[k] = torch.from_numpy(w[k])
    return vsd


@pytest.mark.parametrize("vae_type,dataname", [("N6", "PED"), ("K3", "PDB"), ("K4", "Atlas")])
def test_vq_lookup_bit_exact(vae_type, dataname):
    gold = np.load(cases.npz_path(f"g4_vq_{vae_type}"))
    mean, std = synth.norm_stats(dataname, vae_type)
    dec = Decoder(synth.vqvae_state_dict(vae_type, dataname, cases.VAE_SEED), DEV, mean, std)
    x = synth.gaussian((4, 77, 3), 123 + len(dataname))
    idx, zq, lat = dec.vq(x.to(DEV))
    assert torch.equal(lat.cpu(), torch.from_numpy(gold["latent"]))
    assert torch.equal(idx.cpu(), torch.from_numpy(gold["idx"]))
    assert torch.equal(zq.cpu(), torch.from_numpy(gold["z_q"]))


def test_vq_lookup_large_random_vs_oracle():
    """200k latents incl. exact ties (duplicated codes): first index wins, indices bit-exact."""
    vsd = synth.vqvae_state_dict("N6", "PED", cases.VAE_SEED)
    cb = odec.codebook_of(vsd).clone()
    cb[100] = cb[7]; cb[4095] = cb[7]
    vsd["quantize._codebook.embed"] = cb[None]
    dec = Decoder(vsd, DEV)
    lat = synth.gaussian((200000, 3), 77) * 5.0
    lat[:64] = cb[7]
    idx, zq, _ = dec.vq(lat.to(DEV), normalised=False)
    ridx = odec.vq_lookup(lat, cb)[1]
    assert torch.equal(idx.cpu(), ridx)
    assert int(idx[0]) == 7


@pytest.mark.parametrize("name", list(cases.DECODER_CASES) + ["realC2_L87_B2"])
def test_ic_decode_and_xyz(name):
    real = name.startswith("realC2")
    L, B, seed, vae_type = cases.DECODER_CASES["N6_L87_B2" if real else name]
    prot, batch, latent, dataname = cases.decoder_inputs(L, B, seed, vae_type)
    vsd = _vae_sd(vae_type, dataname, real)
    dec = Decoder(vsd, DEV)
    idx, zq, _ = dec.vq(latent.to(DEV), normalised=False)
    gold = np.load(cases.npz_path(f"g5_decode_{name}"))
    if "idx" in gold.files:
        assert torch.equal(idx.cpu(), torch.from_numpy(gold["idx"]))
    ic = dec.ic_decode(zq.reshape(-1, 3), batch["CG_nxyz"][:, 0].long(), batch["CG_nxyz"][:, 1:],
                       batch["CG_nbr_list"])
    assert rel_err(ic, gold["ic_recon"]) < 2e-5
    if not real:
        og = batch["OG_CG_nxyz"].reshape(-1, L + 2, 4)[:, :, 1:]
        gold_ic = torch.from_numpy(gold["ic_recon"]).reshape(B, L, 13, 3)
        xyz = dec.ic_to_xyz(og.to(DEV), gold_ic.to(DEV), prot["info"])
        gx = torch.from_numpy(np.load(cases.npz_path(f"g6_xyz_{name}"))["xyz"])
        assert xyz.shape == gx.shape
        d = xyz.cpu() - gx
        assert float((d ** 2).sum(-1).mean().sqrt()) < 1e-4          # RMSD, Angstrom
        # Untrained decoder weights give some near-collinear reference triplets, where a placement
        # is ill-conditioned (the reference's own fp32 result is up to 1e-3 A from an fp64 run of
        # the same algorithm in the K4 case).  Require the kernel to be about as close to the
        # fp64 result as the reference's fp32 result is.
        x64 = odec.ic_to_xyz(batch["OG_CG_nxyz"].reshape(-1, L + 2, 4).double(), gold_ic.double(),
                             prot["info"])
        ref_err = float((gx.double() - x64).abs().max())
        my_err = float((xyz.cpu().double() - x64).abs().max())
        assert my_err < 4 * ref_err + 2e-5, (my_err, ref_err)


@pytest.mark.parametrize("name", list(cases.DECODER_CASES))
def test_ic_decode_message_kernel_variants(name):
    """CODLAD_OPT_DEC_EDGE_VARIANT: the decoder's message sum with the radial basis from one sine / cosine and the
    15 -> 40 filter on the f16 matrix pipe (0, default) and with 15 library sines and fp32 FMAs (1, the round-2 kernel):
    both within the golden's tolerance, and close to each other (not bit-identical: different summation order and a
    22-bit operand split)."""
    L, B, seed, vae_type = cases.DECODER_CASES[name]
    prot, batch, latent, dataname = cases.decoder_inputs(L, B, seed, vae_type)
    dec = Decoder(_vae_sd(vae_type, dataname, False), DEV)
    _idx, zq, _ = dec.vq(latent.to(DEV), normalised=False)
    gold = np.load(cases.npz_path(f"g5_decode_{name}"))
    ics = []
    for variant in (0, 1):
        _lib.set_option(_lib.OPT_DEC_EDGE_VARIANT, variant)
        try:
            ics.append(dec.ic_decode(zq.reshape(-1, 3), batch["CG_nxyz"][:, 0].long(), batch["CG_nxyz"][:, 1:],
                                     batch["CG_nbr_list"]))
        finally:
            _lib.set_option(_lib.OPT_DEC_EDGE_VARIANT, 0)
        assert rel_err(ics[-1], gold["ic_recon"]) < 2e-5, variant
    assert rel_err(ics[0], ics[1]) < 1e-5
    assert torch.equal(ics[0], dec.ic_decode(zq.reshape(-1, 3), batch["CG_nxyz"][:, 0].long(), batch["CG_nxyz"][:, 1:],
                                             batch["CG_nbr_list"]))          # deterministic


def test_ic_to_xyz_groups_equals_one_launch_per_protein():
    """codlad_ic_to_xyz_groups: several proteins (different lengths and atom tables) in one launch give exactly the
    coordinates of one codlad_ic_to_xyz launch per protein."""
    dec = Decoder(synth.vqvae_state_dict("N6", "PED", cases.VAE_SEED), DEV)
    groups, want = [], []
    for L, B, seed in ((46, 3, 1), (129, 1, 2), (5, 2, 3), (87, 4, 4)):
        prot = synth.make_protein(L, 70 + seed, n_frames=B)
        ca = torch.from_numpy(prot["xyz_full"]).float().to(DEV)
        ic = (synth.gaussian((B, L, 13, 3), 80 + seed) * torch.tensor([0.1, 0.5, 1.0]) + torch.tensor([1.5, 1.9, 0.0])).to(DEV)
        groups.append((ca, ic, prot["info"]))
        want.append(dec.ic_to_xyz(ca, ic, prot["info"]))
    for reuse in (False, True, True):
        got = dec.ic_to_xyz_groups(groups, reuse=reuse)
        assert len(got) == len(want) and all(torch.equal(g, w) for g, w in zip(got, want))


def test_cg_graph_on_device_equals_reference_neighbour_list():
    """codlad_cg_graph == get_neighbor_list + make_directed + receiver-sorted scatter order."""
    dec = Decoder(synth.vqvae_state_dict("N6", "PED", cases.VAE_SEED), DEV)
    lens, xyzs, pairs, off = [], [], [], 0
    for L, seed in ((5, 1), (46, 2), (129, 3), (300, 4)):
        xyz = torch.from_numpy(synth.make_protein(L, seed)["xyz_full"][0, 1:-1])
        lens.append(L); xyzs.append(xyz)
        pairs.append(synth.cg_nbr_list(xyz) + off)
        off += L
    ptr, src = dec.build_csr(torch.cat(xyzs), lens)
    rptr, rsrc = Decoder.csr_from_pairs(torch.cat(pairs), off)
    assert torch.equal(ptr.cpu(), rptr) and torch.equal(src.cpu(), rsrc)
    # a tighter cutoff exercises the distance test itself
    p8 = synth.cg_nbr_list(xyzs[2], cutoff=8.0)
    ptr8, src8 = dec.build_csr(xyzs[2], [129], cutoff=8.0)
    r8 = Decoder.csr_from_pairs(p8, 129)
    assert torch.equal(ptr8.cpu(), r8[0]) and torch.equal(src8.cpu(), r8[1])


def allowed_code_flips(lat_mine, lat_ref, codebook):
    """Residues whose VQ code MAY legitimately differ between two runs whose latents differ by delta.
    d_k(z) = |z - e_k|^2, so moving z by delta moves the margin d_2 - d_1 by exactly 2 delta.(e_1 - e_2):
    a flip needs margin <= 2 |delta| |e_1 - e_2| (+ the fp32 rounding of the distance formula itself,
    a few ulp of |z|^2 + |e|^2).  A factor 2 of slack on the first term; nothing else is tolerated.
    Returns (allowed [n] bool, ref idx [n], margin [n])."""
    z = lat_ref.reshape(-1, 3).double()
    e = codebook.double()
    d = (z ** 2).sum(1, keepdim=True) + (e ** 2).sum(1) - 2.0 * z @ e.t()
    top = torch.topk(d, 2, dim=1, largest=False)
    margin = top.values[:, 1] - top.values[:, 0]
    e1, e2 = e[top.indices[:, 0]], e[top.indices[:, 1]]
    delta = (lat_mine.reshape(-1, 3).double() - z).norm(dim=1)
    bound = 2.0 * 2.0 * delta * (e1 - e2).norm(dim=1) + 8 * 2.0 ** -24 * ((z ** 2).sum(1) + (e1 ** 2).sum(1))
    return margin <= bound, top.indices[:, 0], margin


@pytest.mark.parametrize("name", list(cases.E2E_CASES))
def test_end_to_end(den, sd, name):
    """noise -> xyz on the GPU vs the reference CPU path (N6 and the two angle decoders).  A VQ code may differ from
    the reference's only where the OBSERVED latent deviation of that residue can bridge the reference's own top-2 margin
    (allowed_code_flips) AND the case lists that near-tie by name (cases.E2E_EXPECTED_FLIPS: none on the committed
    goldens); then EVERY frame's internal coordinates and Cartesian coordinates are compared."""
    L, B, seed, T, vae_type, dataname = cases.E2E_CASES[name]
    gold = np.load(cases.npz_path(f"g7_e2e_{name}"))
    prot, batch, _x, _t, mask = cases.denoiser_inputs(L, B, seed, phospho=vae_type != "N6")
    z, eps = cases.loop_noise(T, B, L, seed)
    st = structures_of(den, prot)
    job = den.make_job(st, list(range(B)))
    x0 = den.sample(job, z.reshape(-1, 3).to(DEV), eps.reshape(T, -1, 3).to(DEV), tables(T))
    assert rel_err(x0.cpu().view(B, L, 3), gold["samples"]) < 1e-4
    mean, std = synth.norm_stats(dataname, vae_type)
    vsd = synth.vqvae_state_dict(vae_type, dataname, cases.VAE_SEED)
    dec = Decoder(vsd, DEV, mean, std)
    idx, zq, lat = dec.vq(x0)
    lat_ref = torch.from_numpy(gold["samples"]) * std + mean                 # get_norm_feature(norm_in=False)
    allowed, ref_idx, margin = allowed_code_flips(lat.cpu(), lat_ref, odec.codebook_of(vsd))
    assert torch.equal(ref_idx, torch.from_numpy(gold["idx"]).reshape(-1))   # the golden's own codes, recomputed
    differ = idx.cpu() != ref_idx
    assert not bool((differ & ~allowed).any()), \
        f"{int((differ & ~allowed).sum())} VQ codes differ where the latent deviation cannot explain it " \
        f"(smallest such margin {float(margin[differ & ~allowed].min()):.3e})"
    expected = sorted(cases.E2E_EXPECTED_FLIPS.get((name, den.weights.precision), []))
    assert differ.nonzero().flatten().tolist() == expected, \
        f"VQ codes of residues {differ.nonzero().flatten().tolist()} differ from the reference's (margins " \
        f"{margin[differ].tolist()}); expected {expected}"
    # with no unexpected flip every frame decodes from the reference's own codes: all of them are compared
    ic = dec.ic_decode(zq, batch["CG_nxyz"][:, 0].long(), batch["CG_nxyz"][:, 1:], batch["CG_nbr_list"])
    clean = ~differ.view(B, L).any(dim=1)
    assert int(clean.sum()) == B - len({r // L for r in expected})
    ic_ref = torch.from_numpy(gold["ic_recon"]).reshape(B, L, 13, 3)
    assert rel_err(ic.view(B, L, 13, 3).cpu()[clean], ic_ref[clean]) < 2e-5
    og = batch["OG_CG_nxyz"].reshape(-1, L + 2, 4)
    xyz = dec.ic_to_xyz(og[:, :, 1:].to(DEV), ic.view(B, L, 13, 3), prot["info"])
    gx = torch.from_numpy(gold["xyz"])
    rmsd = ((xyz.cpu() - gx) ** 2).sum(-1)[clean].mean().sqrt()
    # N6: RMSD <= 1e-4 A (north_star).  The angle decoders with untrained weights place some atoms from near-collinear
    # triplets, where ic -> xyz is ill-conditioned (the reference's own fp32 coordinates are up to ~1e-3 A from an fp64
    # run of the same placements): there the coordinates must be about as close to the fp64 placement of the REFERENCE's
    # internal coordinates as the reference's own fp32 result is - the criterion of test_ic_decode_and_xyz.
    if vae_type == "N6":
        assert float(rmsd) < 1e-4, float(rmsd)
    else:
        x64 = odec.ic_to_xyz(og.double(), ic_ref.double(), prot["info"])
        ref_err = float((gx.double() - x64)[clean].abs().max())
        my_err = float((xyz.cpu().double() - x64)[clean].abs().max())
        assert my_err < 4 * ref_err + 1e-4, (my_err, ref_err)
    print(f"{name}: no code flips, {int(clean.sum())}/{B} frames compared, RMSD {float(rmsd):.2e} A")


def test_random_ragged_jobs_against_oracle_and_between_modes(sd):
    """Randomised shapes: tiny and odd lengths, repeated / unused structures, uneven ensemble sizes.
    Each job: f16x3 against the f32-MFMA mode, two samples against the CPU oracle, and one sample
    bit-for-bit against the same sample run alone."""
    rng = np.random.Generator(np.random.PCG64(2024))
    d3, d32 = Denoiser(sd, DEV, precision="f16x3"), Denoiser(sd, DEV, precision="f32")
    for trial in range(6):
        n_struct = int(rng.integers(2, 7))
        lens = [int(x) for x in rng.choice([4, 5, 7, 16, 31, 32, 33, 40, 63, 64, 65, 97, 130, 201], n_struct)]
        prots = [synth.make_protein(L, 500 + 10 * trial + i, n_frames=1) for i, L in enumerate(lens)]
        xyz = [torch.from_numpy(p["xyz_full"])[0, 1:-1] for p in prots]
        zz = [torch.from_numpy(p["z_full"])[1:-1] for p in prots]
        sample_struct = [int(s) for s in rng.integers(0, n_struct, int(rng.integers(1, 9)))]
        n_nodes = sum(lens[s] for s in sample_struct)
        x = synth.gaussian((n_nodes, 3), 900 + trial).to(DEV)
        t = int(rng.integers(0, 1000))
        outs = {}
        for name, den in (("f16x3", d3), ("f32", d32)):
            st = den.prepare_structures(xyz, zz)
            outs[name] = den.forward(den.make_job(st, sample_struct), x, t)
        assert bool(torch.isfinite(outs["f16x3"]).all())
        assert rel_err(outs["f16x3"], outs["f32"]) < 5e-6, (trial, lens, sample_struct)
        off = np.concatenate([[0], np.cumsum([lens[s] for s in sample_struct])])
        for k in sorted({0, len(sample_struct) - 1}):
            s = sample_struct[k]
            a, b = int(off[k]), int(off[k + 1])
            batch = synth.make_batch(prots[s])
            cg_z, cg_xyz, m = oden.batch_to_dense(batch)
            ref = oden.forward(sd, x[a:b].cpu()[None], torch.tensor([t]), cg_xyz, cg_z, m)
            assert rel_err(outs["f16x3"][a:b], ref[0]) < 1e-5, (trial, k, lens[s])
            alone = d3.forward(d3.make_job(d3.prepare_structures([xyz[s]], [zz[s]]), [0]), x[a:b], t)
            assert torch.equal(alone, outs["f16x3"][a:b])


def test_small_job_node_kernel_is_bit_identical_to_the_streaming_one(sd):
    """The wide node kernel (small jobs: one 32-node tile per 8-wave workgroup, contractions cut by output block,
    operands exchanged as split fragments through LDS) computes exactly what the streaming kernel does: same
    per-element code, same accumulation order."""
    outs = []
    # streaming kernel | eight waves per tile (node_kernel_w) | four waves per tile with a ring of weight quarters (node_kernel_q)
    for max_tiles, quad_tiles in ((0, 0), (1 << 20, 0), (1 << 20, 1 << 20)):
        _lib.set_option(_lib.OPT_NODEQ_MAX_TILES, max_tiles)
        _lib.set_option(_lib.OPT_NODE_QUAD_MAX_TILES, quad_tiles)
        try:
            for precision in ("f16x3", "f16x4"):
                d = Denoiser(sd, DEV, precision=precision)
                pa, pb = synth.make_protein(40, 5, n_frames=1), synth.make_protein(87, 6, n_frames=1)
                st = d.prepare_structures([torch.from_numpy(p["xyz_full"])[0, 1:-1] for p in (pa, pb)],
                                          [torch.from_numpy(p["z_full"])[1:-1] for p in (pa, pb)])
                job = d.make_job(st, [0, 1, 1])
                x = synth.gaussian((40 + 87 + 87, 3), 99).to(DEV)
                T = 5
                eps = synth.gaussian((T, 214, 3), 98).to(DEV)
                outs.append((d.forward(job, x, 700), d.sample(job, x, eps, tables(T))))
        finally:
            _lib.set_option(_lib.OPT_NODEQ_MAX_TILES, 256)
            _lib.set_option(_lib.OPT_NODE_QUAD_MAX_TILES, NODE_QUAD_DEFAULT)
    for v in (1, 2):
        for k in range(2):
            assert bool(torch.isfinite(outs[k][0]).all())
            assert torch.equal(outs[k][0], outs[2 * v + k][0]) and torch.equal(outs[k][1], outs[2 * v + k][1]), (v, k)


def test_small_job_tilewise_edge_kernels_agree_with_per_node_order(sd):
    """Small jobs deal the edge kernels' work out per non-empty 32-edge tile (two waves per node with K > 32; the
    message sum is kept per half and lane half and added up by the node kernel in the per-node kernel's order):
    bit-identical to the per-node order, on lengths that give empty, partial and full second halves, in both node
    kernels, and equal to the oracle."""
    lens = [5, 31, 32, 33, 47, 64, 87]
    prots = [synth.make_protein(L, 300 + i, n_frames=1) for i, L in enumerate(lens)]
    xyz = [torch.from_numpy(p["xyz_full"])[0, 1:-1] for p in prots]
    zz = [torch.from_numpy(p["z_full"])[1:-1] for p in prots]
    x = synth.gaussian((sum(lens), 3), 17).to(DEV)
    T = 4
    eps = synth.gaussian((T, sum(lens), 3), 18).to(DEV)
    outs = []
    for max_nodes, wide_tiles in ((0, 256), (1 << 20, 256), (1 << 20, 0)):
        _lib.set_option(_lib.OPT_EDGE_TILE_MAX_NODES, max_nodes)
        _lib.set_option(_lib.OPT_NODEQ_MAX_TILES, wide_tiles)
        _lib.set_option(_lib.OPT_EDGE_WIDE_MAX_TILES, 0)      # the one-wave tile kernels (the four-wave ones: next test)
        _lib.set_option(_lib.OPT_NODE_QUAD_MAX_TILES, 0)      # node update: streaming or eight-wave kernel as NODEQ says
        try:
            d = Denoiser(sd, DEV, precision="f16x3")
            job = d.make_job(d.prepare_structures(xyz, zz), list(range(len(lens))))
            if max_nodes:
                tl = job.tile_list.cpu()
                want = [(n, hf) for n in range(sum(lens)) for hf in range(2 if int(job.node_info[n, 2]) > 32 else 1)]
                assert [tuple(r) for r in tl.tolist()] == want
            outs.append((d.forward(job, x, 600), d.sample(job, x, eps, tables(T))))
        finally:
            _lib.set_option(_lib.OPT_EDGE_TILE_MAX_NODES, 1 << 30)
            _lib.set_option(_lib.OPT_NODEQ_MAX_TILES, 256)
            _lib.set_option(_lib.OPT_EDGE_WIDE_MAX_TILES, EDGE_WIDE_DEFAULT)
            _lib.set_option(_lib.OPT_NODE_QUAD_MAX_TILES, NODE_QUAD_DEFAULT)
    for o in outs[1:]:
        assert torch.equal(o[0], outs[0][0]) and torch.equal(o[1], outs[0][1])
    off = np.concatenate([[0], np.cumsum(lens)])
    for k in (0, 3, 6):
        batch = synth.make_batch(prots[k])
        cg_z, cg_xyz, m = oden.batch_to_dense(batch)
        a, b = int(off[k]), int(off[k + 1])
        ref = oden.forward(sd, x[a:b].cpu()[None], torch.tensor([600]), cg_xyz, cg_z, m)
        assert rel_err(outs[1][0][a:b], ref[0]) < 1e-5


@pytest.mark.parametrize("precision", ["f16x3", "f16x4"])
def test_small_job_wide_edge_kernels_are_bit_identical(sd, precision):
    """msg_wide_kernel / upd_wide_kernel (edge_wide_kernels.hip: four waves per 32-edge tile, one output block each, weight
    quarters in registers, the LayerNorm's moments streamed from LDS in the one-wave order) against the one-wave tile
    kernels and the per-node kernels: bit-identical, with and without the hoisted layer-0 terms, on lengths that give
    empty, partial and full second halves; also with fewer workgroups than tiles (a workgroup walks several tiles)."""
    lens = [5, 31, 32, 33, 47, 64, 87, 120]
    prots = [synth.make_protein(L, 500 + i, n_frames=1) for i, L in enumerate(lens)]
    xyz = [torch.from_numpy(p["xyz_full"])[0, 1:-1] for p in prots]
    zz = [torch.from_numpy(p["z_full"])[1:-1] for p in prots]
    members = list(range(len(lens))) + [7, 6, 0] + [7] * 2
    n = sum(lens[m] for m in members)
    x = synth.gaussian((n, 3), 37).to(DEV)
    T = 3
    eps = synth.gaussian((T, n, 3), 38).to(DEV)
    outs = []
    try:
        # per-node kernels | one-wave tile kernels | wide kernels
        for max_nodes, wide in ((0, 0), (1 << 20, 0), (1 << 20, 1 << 20)):
            _lib.set_option(_lib.OPT_EDGE_TILE_MAX_NODES, max_nodes)
            _lib.set_option(_lib.OPT_EDGE_WIDE_MAX_TILES, wide)
            d = Denoiser(sd, DEV, precision=precision)
            for hoist in (True, False):
                job = d.make_job(d.prepare_structures(xyz, zz, hoist_layer0=hoist), members)
                if wide:
                    assert 2 * 256 < job.ws.n_tiles <= 8 * 256      # more tiles than the wide kernels' grid: workgroups loop
                outs.append((d.forward(job, x, 600), d.sample(job, x, eps, tables(T))))
    finally:
        _lib.set_option(_lib.OPT_EDGE_TILE_MAX_NODES, 1 << 30)
        _lib.set_option(_lib.OPT_EDGE_WIDE_MAX_TILES, EDGE_WIDE_DEFAULT)
    for k in range(2):
        assert bool(torch.isfinite(outs[k][0]).all())
        for v in (1, 2):
            assert torch.equal(outs[k][0], outs[2 * v + k][0]) and torch.equal(outs[k][1], outs[2 * v + k][1]), (precision, k, v)


@pytest.mark.parametrize("precision", ["f16x3", "f16x4"])
def test_edge_update_one_wave_per_simd_is_bit_identical(sd, precision):
    """upd1_kernel_h (round 4: one wave per SIMD, five k-steps of W11e resident in registers, the next tile's rows and
    Q rows prefetched) runs the arithmetic of upd_kernel_h in the same order: bit-identical, with and without the
    hoisted layer-0 terms, on lengths that give empty, partial and full second halves and one-tile nodes in a row."""
    lens = [5, 31, 32, 33, 47, 64, 87, 120]
    prots = [synth.make_protein(L, 400 + i, n_frames=1) for i, L in enumerate(lens)]
    xyz = [torch.from_numpy(p["xyz_full"])[0, 1:-1] for p in prots]
    zz = [torch.from_numpy(p["z_full"])[1:-1] for p in prots]
    members = list(range(len(lens))) + [7, 6, 0]
    n = sum(lens[m] for m in members)
    x = synth.gaussian((n, 3), 27).to(DEV)
    T = 3
    eps = synth.gaussian((T, n, 3), 28).to(DEV)
    outs = []
    _lib.set_option(_lib.OPT_EDGE_TILE_MAX_NODES, 0)      # the per-node kernels, whatever the job size
    try:
        for variant in (0, 2):         # 2: upd1_kernel_h whatever the job (1 leaves jobs with many one-tile nodes to upd_kernel_h)
            _lib.set_option(_lib.OPT_EDGE_UPD_VARIANT, variant)
            d = Denoiser(sd, DEV, precision=precision)
            for hoist in (True, False):
                job = d.make_job(d.prepare_structures(xyz, zz, hoist_layer0=hoist), members)
                outs.append((d.forward(job, x, 600), d.sample(job, x, eps, tables(T))))
    finally:
        _lib.set_option(_lib.OPT_EDGE_TILE_MAX_NODES, 1 << 30)
        _lib.set_option(_lib.OPT_EDGE_UPD_VARIANT, EDGE_UPD_DEFAULT)
    for k in range(2):
        assert bool(torch.isfinite(outs[k][0]).all())
        assert torch.equal(outs[k][0], outs[2 + k][0]) and torch.equal(outs[k][1], outs[2 + k][1]), (precision, k)
