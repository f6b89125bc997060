"""The float64 path through the CPU oracle and the classifier of ill-conditioned edges (tests/conditioning.py): what
the per-edge and per-node GPU tests (test_hip_parity.py::test_features_prepass, test_fp64_parity.py) stand on.  No GPU.

Errors here are per node and per output channel, each channel scaled by its own largest value over the case - not one
number per tensor (the six output channels have maxima between 0.26 and 2.4)."""
import numpy as np
import pytest
import torch

from codlad_amd import synth
from oracle import denoiser as oden
from tests import cases
from tests import conditioning as cond

# fp32 forward against the float64 one, everything but the timestep embedding: the bound the suite holds every fp32
# evaluation of these cases to (test_denoiser_forward: 1e-5 of the tensor's maximum), here per channel.
FP32_FORWARD = 1e-5


def embedding_term(t_max):
    """What the fp32 timestep embedding adds: cos / sin of t * f with the frequency f rounded to fp32 (2^-24 relative) and
    the product rounded again (2^-24), so the argument is off by up to t * 2^-23 at f ~ 1; cos and sin have slope <= 1 and
    the embedding enters the adaLN vectors, which scale and shift O(1) activations, with a gain of order one."""
    return float(t_max) * 2.0 ** -23


def g(name):
    return np.load(cases.npz_path(name))


@pytest.fixture(scope="module")
def sd():
    return synth.denoiser_state_dict(cases.WEIGHT_SEED)


def forward64(sd, x, t, cg_xyz, cg_z, mask, **kw):
    kw = {k: (v.double() if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in kw.items()}
    return oden.forward(cond.to_dtype(sd, torch.float64), x.double(), t, cg_xyz.double(), cg_z, mask, **kw)


def check_against_golden(sd, gold_out, x, t, cg_xyz, cg_z, mask, what, **kw):
    """float64 forward against a golden output of the reference's fp32 forward, per node and channel: with the fp32
    adaLN vectors substituted (everything but the timestep embedding) and whole."""
    gold_out = torch.from_numpy(gold_out)
    valid = mask[..., None].expand_as(gold_out)
    out = forward64(sd, x, t, cg_xyz, cg_z, mask, **kw)
    assert out.dtype == torch.float64
    e_all = float(cond.node_channel_error(gold_out, out)[valid].max())
    part = forward64(sd, x, t, cg_xyz, cg_z, mask, mods=oden.step_mods(sd, t), **kw)
    e_part = float(cond.node_channel_error(gold_out, part)[valid].max())
    print(f"{what}: fp32 golden vs float64, per node and channel: {e_all:.2e} whole, {e_part:.2e} with the fp32 adaLN vectors")
    assert e_part < FP32_FORWARD, (what, e_part)
    assert e_all < FP32_FORWARD + embedding_term(float(t.max())), (what, e_all)


@pytest.mark.parametrize("name", list(cases.DENOISER_CASES) + [cases.PADDED_CASE[0]])
def test_float64_forward_against_g2(sd, name):
    gold = g(f"g2_forward_{name}")
    if name == cases.PADDED_CASE[0]:
        batch, x, t, mask = cases.padded_inputs(*cases.PADDED_CASE[1:])
    else:
        prot, batch, x, t, mask = cases.denoiser_inputs(*cases.DENOISER_CASES[name])
    cg_z, cg_xyz, m = oden.batch_to_dense(batch)
    check_against_golden(sd, gold["out"], x, t, cg_xyz, cg_z, mask, name)


@pytest.mark.parametrize("name", list(cases.SELF_COND_CASES))
def test_float64_forward_against_g9_selfcond(name):
    L, B, seed, _T = cases.SELF_COND_CASES[name]
    gold = g(f"g9_selfcond_{name}")
    sd_sc = synth.denoiser_state_dict(cases.WEIGHT_SEED, self_condition=True)
    prot, batch, x, t, mask = cases.denoiser_inputs(L, B, seed)
    cg_z, cg_xyz, m = oden.batch_to_dense(batch)
    xsc = synth.gaussian((B, L, 3), 6000 + seed)
    check_against_golden(sd_sc, gold["out_none"], x, t, cg_xyz, cg_z, m, name + " no x_self_cond")
    check_against_golden(sd_sc, gold["out_sc"], x, t, cg_xyz, cg_z, m, name + " x_self_cond", x_self_cond=xsc)


@pytest.mark.parametrize("name", list(cases.FLOW_CASES))
def test_float64_forward_against_g12_flow(name):
    L, B, seed, times, _n = cases.FLOW_CASES[name]
    gold = g(f"g12_flow_{name}")
    fsd = synth.denoiser_state_dict(cases.WEIGHT_SEED, flow=True)
    prot, batch, x, _t, mask = cases.denoiser_inputs(L, B, seed)
    cg_z, cg_xyz, m = oden.batch_to_dense(batch)
    for k, tv in enumerate(times):
        t = torch.full((B,), tv, dtype=torch.float32)          # the fp32 time the reference's model was given
        check_against_golden(fsd, gold[f"v_t{k}"], x, t, cg_xyz, cg_z, mask, f"{name} t={tv}")


@pytest.mark.parametrize("name", ["L20_B2", "L87_B2"])
def test_substitution_hooks_are_bit_neutral(sd, name):
    """forward(h_E0=, mods=) fed with the forward's own intermediate values is the plain forward to the bit (fp32), each
    hook alone and both together; ca_features(E_idx=) with the selection's own list likewise."""
    prot, batch, x, t, mask = cases.denoiser_inputs(*cases.DENOISER_CASES[name])
    cg_z, cg_xyz, m = oden.batch_to_dense(batch)
    taps = {}
    plain = oden.forward(sd, x, t, cg_xyz, cg_z, mask, taps=taps)
    hE0, mods = (taps["h_E0"], taps["E_idx"]), oden.step_mods(sd, t)
    assert mods.shape == (x.shape[0], 6016)
    for kw in (dict(h_E0=hE0), dict(mods=mods), dict(h_E0=hE0, mods=mods), dict(h_E0=hE0, mods=mods[0])):
        taps2 = {}
        assert torch.equal(oden.forward(sd, x, t, cg_xyz, cg_z, mask, taps=taps2, **kw), plain), list(kw)
        assert all(torch.equal(taps[k], taps2[k]) for k in taps)
    E, E_idx = oden.ca_features(sd, cg_xyz, m.int())
    E2, E_idx2 = oden.ca_features(sd, cg_xyz, m.int(), E_idx=E_idx)
    assert torch.equal(E, E2) and E_idx2 is E_idx
    # a permuted list permutes the rows
    perm = torch.randperm(E_idx.shape[-1], generator=torch.Generator().manual_seed(3))
    E3, _ = oden.ca_features(sd, cg_xyz, m.int(), E_idx=E_idx[..., perm])
    assert torch.equal(E3, E[:, :, perm])


def test_float64_forward_is_float64_throughout(sd):
    """Every tap of a float64 forward is float64 (nothing on the way pins fp32), and the timestep embedding follows the
    weights' dtype."""
    prot, batch, x, t, mask = cases.denoiser_inputs(*cases.DENOISER_CASES["L20_B2"])
    cg_z, cg_xyz, m = oden.batch_to_dense(batch)
    taps = {}
    forward64(sd, x, t, cg_xyz, cg_z, mask, taps=taps)
    assert all(v.dtype == torch.float64 for k, v in taps.items() if k != "E_idx")
    e32, e64 = oden.timestep_embedding(t), oden.timestep_embedding(t, dtype=torch.float64)
    assert e32.dtype == torch.float32 and e64.dtype == torch.float64
    assert float((e32.double() - e64).abs().max()) < embedding_term(float(t.max()))


# ---------------------------------------------------------------------------------------------------------------------
# the classifier
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(cond.feature_geometries()))
def test_edge_conditioning_rule(sd, name):
    """What validates the rule of tests/conditioning.py, on every geometry the per-edge GPU test uses: it calls at most
    10 % of the edges ill-conditioned, and on the others the reference's own fp32 agrees with float64 within 2e-6 of the
    tensor's maximum (measured 8.0e-7 - 9.2e-7; the factor 2 is for other CPUs' vector maths)."""
    L, B, seed = cond.feature_geometries()[name]
    prot, batch, x, t, mask = cases.denoiser_inputs(L, B, seed)
    cg_z, cg_xyz, m = oden.batch_to_dense(batch)
    h32, E_idx = cond.edge_state(sd, cg_xyz, m)
    h64, _ = cond.edge_state(cond.to_dtype(sd, torch.float64), cg_xyz, m, E_idx=E_idx)
    ill = cond.edge_conditioning(cg_xyz, E_idx)
    assert ill.shape == E_idx.shape and ill.dtype == torch.bool
    share = float(ill.double().mean())
    err = cond.edge_row_error(h32, h64)
    print(f"{name}: {share:.1%} ill-conditioned; fp32 vs float64 {float(err[~ill].max()):.2e} on the rest, "
          f"{float(err[ill].max()):.2e} on them")
    assert share <= cond.MAX_ILL_SHARE, (name, share)
    assert float(err[~ill].max()) < 2e-6, (name, float(err[~ill].max()))
    # a self edge between whole frames has R = I up to rounding: every radicand is noise (the chain's ends and residues
    # next to a step outside the 3.6-4.0 A window have zeroed frames, R = 0, and nothing ill-conditioned about them)
    whole = cond.edge_quantities(cg_xyz, E_idx)["tr1"][:, :, 0] > 3.9
    assert bool(whole.any()) and bool(ill[:, :, 0][whole].all())


def test_edge_quantities_are_the_oracles(sd):
    """The restated radicands / sign arguments give the float64 oracle's quaternion back exactly, so the classifier
    cannot drift from the formulas it speaks about."""
    prot, batch, x, t, mask = cases.denoiser_inputs(*cases.DENOISER_CASES["L46_B2"])
    cg_z, cg_xyz, m = oden.batch_to_dense(batch)
    _, E_idx = oden.knn(cg_xyz, m.float())
    q = cond.edge_quantities(cg_xyz, E_idx)
    quat = torch.nn.functional.normalize(torch.cat((torch.sign(q["s"]) * 0.5 * q["r"].abs().sqrt(),
                                                    torch.relu(q["tr1"]).sqrt()[..., None] / 2.0), -1), dim=-1)
    assert torch.equal(quat, oden.orientation_features(cg_xyz.double(), E_idx)[..., 3:])
    assert torch.equal(quat, oden._quaternions(q["R"]))
