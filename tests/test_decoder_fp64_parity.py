"""GPU: the IC decoder (csrc/ic_decoder_kernels.hip) residue by residue and channel by channel against a float64 reference.

The decoder's counterpart of test_fp64_parity.py (denoiser) and test_e3nn_fp64_parity.py (encoder).  Per residue and per
channel, each channel scaled by its own largest float64 value over the case (tests/conditioning.py::node_channel_error):

    err_hip[residue, ch] <= c x max(e_ref[ch], FLOOR)

e_ref[ch]: the fp32 oracle's largest per-residue error against float64 in that channel on the same inputs, computed here.
FLOOR = 1e-6 of the channel's maximum.  c = 4 where the arithmetic keeps fp32 operands and the reference's order
(dec_init / dec_dense / dec_heads, and the message sum with CODLAD_OPT_DEC_EDGE_VARIANT = 1), c = 16 with the default
variant 0, whose filter operands are split into 22 of 24 significand bits (the two bits f16x3 is granted).  No residue and
no channel is left out.  Table channels (bond lengths; the side-chain angles of the non-angle model) are bit-equal to the
fp32 table entry.

Three things are held:
  (a) ic    the 39 outputs against the float64 oracle run end to end from the same z_q;
  (b) S     the final state (40 channels, the heads' input) read back from the scratch against the oracle's - the heads
            are then out of the picture;
  (c) V     the block-3 message sum read back from the scratch against a float64 message sum GIVEN THE DEVICE'S OWN
            block-3 phi (cast up), e_ref from the fp32 message sum of the same phi: dec_edge_kernel /
            dec_edge_exact_kernel alone, edge by edge on the in-degree-1 rows of the cutoff sweep.

Cases: tests/decoder_cases.py (held to what they claim by tests/test_decoder_cases_host.py).
Measured ratios per tap, variant and case: DESIGN.md section 2.
"""
import pytest
import torch

from codlad_amd import _lib
from codlad_amd.engine import Decoder
from tests import decoder_cases as dc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
VARIANTS = (0, 1)

_decoders = {}


def decoder_of(weights):
    if weights not in _decoders:
        _decoders[weights] = Decoder(dc.state_dict_of(weights), DEV)
    return _decoders[weights]


def device_run(case, variant):
    """One decode on the device -> CPU tensors: ic [M,39] and the taps of Decoder.read_taps."""
    dec = decoder_of(case["weights"])
    M = case["cg_xyz"].shape[0]
    scratch = torch.full((M, Decoder.SCRATCH_WIDTH), float("nan"), device=DEV)      # nothing read below may be left over
    _lib.set_option(_lib.OPT_DEC_EDGE_VARIANT, variant)
    try:
        ic = dec.ic_decode(case["z_q"].to(DEV), case["cg_z"], case["cg_xyz"], case["pairs"], scratch=scratch)
        torch.cuda.synchronize()
    finally:
        _lib.set_option(_lib.OPT_DEC_EDGE_VARIANT, 0)
    taps = {k: v.cpu() for k, v in Decoder.read_taps(scratch).items()}
    assert ic.shape == (M, 13, 3) and bool(torch.isfinite(ic).all()) and all(bool(torch.isfinite(t).all()) for t in taps.values())
    return ic.cpu().reshape(M, 39), taps


def hold(label, variant, what, got, r32, r64, c=None):
    """Print the worst ratio of one tap and assert the rule on every residue and channel."""
    c = dc.C_VARIANT[variant] if c is None else c
    r, n, ch, err, e_ref = dc.worst_ratio(got, r32, r64)
    msg = (f"fp64 parity decoder {label} variant {variant} {what}: err/max(e_ref, FLOOR) {r:.2f} at residue {n} channel {ch} "
           f"(err {err:.2e}, e_ref {e_ref:.2e})")
    print(msg)
    assert r <= c, msg
    return r


def check_ic_and_state(case, variant, got=None):
    """(a) and (b), and the table channels bit for bit."""
    ic, taps = device_run(case, variant) if got is None else got
    ref = dc.references(case)
    table = dc.table_channels(dc.is_angle(case))
    assert torch.equal(ic[:, table], ref["ic"][0][:, table]), f"{case['name']}: table channels differ from the fp32 table"
    hold(case["name"], variant, "ic", ic, *ref["ic"])
    hold(case["name"], variant, "S", taps["S"], *ref["S"])
    return ic, taps


def check_message_sum(case, variant, taps):
    """(c): the device's block-3 V against the message sum of the device's own block-3 phi."""
    v32, v64 = dc.message_references(case, taps["phi3"])
    assert v64.dtype == torch.float64
    hold(case["name"], variant, "V", taps["V"], v32, v64)
    return v64


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("vae_type", ["N6", "K4"])
def test_indegree(vae_type, variant):
    """In-degrees 0, 1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 200 and true neighbourhoods of up to four chunks, a
    coincident pair, all 25 residue types; dec_heads_kernel<false> (N6) and <true> (K4)."""
    case = dc.indegree_case(vae_type)
    _ic, taps = check_ic_and_state(case, variant)
    v64 = check_message_sum(case, variant, taps)
    assert bool((taps["V"][0] == 0).all()) and bool((v64[0] == 0).all())              # in-degree 0


@pytest.mark.parametrize("variant", VARIANTS)
def test_cutoff_sweep(variant):
    """One edge per row of V from the coincident floor to beyond the cutoff: radial basis (one sincos and the recurrence
    in variant 0, 15 library sines in variant 1), envelope and the >= branch, edge by edge."""
    case = dc.cutoff_sweep_case()
    _ic, taps = check_ic_and_state(case, variant)
    check_message_sum(case, variant, taps)
    rows, d, nominal = dc.sweep_rows(case)
    beyond = rows[d >= dc.CUTOFF]
    assert beyond.numel() == 4 and 21.0 in d.tolist()
    assert bool((taps["V"][beyond] == 0).all()), "a row at d >= 21 is not exactly zero"
    inside = rows[d < 20.0]
    assert bool((taps["V"][inside].abs().amax(1) > 0).all())


@pytest.mark.parametrize("M", dc.ROWS_M)
def test_rows(M):
    """M = 2, 63, 64, 65, 129: the last workgroup of the lane-per-residue kernels with 2, 63, 64, 1 and 1 live lanes."""
    check_ic_and_state(dc.rows_case(M), 0)


@pytest.mark.parametrize("builder", ["pairs", "build_csr"])
@pytest.mark.parametrize("M", [1, 5])
def test_graph_without_edges_decodes_with_zero_messages(M, builder):
    """A graph without edges (a single residue; an empty pair list) decodes, from either CSR builder: every V is zero,
    the result is the oracle's for the empty list."""
    case = dc.no_edges_case(M)
    dec = decoder_of(case["weights"])
    if builder == "pairs":
        csr = Decoder.csr_from_pairs(case["pairs"].to(DEV), M)
    else:
        csr = dec.build_csr(case["cg_xyz"], [1] * M)                    # M samples of one residue: no pair shares a sample
    assert csr[0].tolist() == [0] * (M + 1) and csr[1].numel() == 0
    scratch = torch.full((M, Decoder.SCRATCH_WIDTH), float("nan"), device=DEV)
    ic = dec.ic_decode(case["z_q"].to(DEV), case["cg_z"], case["cg_xyz"], csr=csr, scratch=scratch)
    taps = {k: v.cpu() for k, v in Decoder.read_taps(scratch).items()}
    assert bool((taps["V"] == 0).all())
    check_ic_and_state(case, 0, got=(ic.cpu().reshape(M, 39), taps))


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("name", dc.EXISTING)
def test_existing_geometries(name, variant):
    """The shipped decoder cases under the per-residue, per-channel rule (test_ic_decode_and_xyz holds them to one
    global norm at 2e-5)."""
    check_ic_and_state(dc.existing_case(name), variant)


def test_scratch_argument_is_checked_and_optional():
    case = dc.rows_case(65)
    dec = decoder_of(case["weights"])
    args = (case["z_q"].to(DEV), case["cg_z"], case["cg_xyz"], case["pairs"])
    scratch = torch.empty(65, Decoder.SCRATCH_WIDTH, device=DEV)
    assert torch.equal(dec.ic_decode(*args), dec.ic_decode(*args, scratch=scratch))
    with pytest.raises(ValueError):
        dec.ic_decode(*args, scratch=torch.empty(64, Decoder.SCRATCH_WIDTH, device=DEV))
    with pytest.raises(ValueError):
        dec.ic_decode(*args, scratch=torch.empty(65, Decoder.SCRATCH_WIDTH, device=DEV, dtype=torch.float64))


@pytest.mark.parametrize("variant", VARIANTS)
def test_persistent_loop_second_trip(variant):
    """M = 4 222 > 16 x CUs: dec_edge_kernel's persistent loop (variant 0) takes a second trip for the residues past
    the grid - reused jsh, re-zeroed sums.  The first, a middle, the last 87-residue copy (which straddles the grid) and
    the 46-residue sample beyond it are bit-identical to launches of their own, and hold (a).  Variant 1 (one workgroup
    per residue, no loop) once, for the same claim of its header."""
    job, offs = dc.persistent_case()
    M = job["cg_xyz"].shape[0]
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    if M <= 16 * cus:
        pytest.skip(f"{cus} CUs: the edge kernel's grid of {16 * cus} covers all {M} residues, no second loop trip")
    assert M > 16 * cus
    ic, taps = device_run(job, variant)
    parts = dc.persistent_parts()
    for k in (0, dc.PERSISTENT_COPIES // 2, dc.PERSISTENT_COPIES - 1, dc.PERSISTENT_COPIES):
        a, b = offs[k], offs[k + 1]
        if k >= dc.PERSISTENT_COPIES - 1:
            assert b > 16 * cus                                          # residues of a second loop trip
        one_ic, one_taps = device_run(parts[k], variant)
        assert torch.equal(ic[a:b], one_ic), f"sample {k}: ic depends on what shares the launch"
        for tap in ("S", "V", "phi3"):
            assert torch.equal(taps[tap][a:b], one_taps[tap]), f"sample {k}: {tap} depends on what shares the launch"
        check_ic_and_state(parts[k], variant, got=(ic[a:b], {t: v[a:b] for t, v in taps.items()}))
