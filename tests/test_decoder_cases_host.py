"""CPU: the cases of tests/decoder_cases.py are what they claim to be, and the oracle's taps are its own computation.

The GPU test (test_decoder_fp64_parity.py) only means something if the crafted pair lists really produce the aimed-at
in-degrees and distances, if the float64 oracle really runs in float64, and if the rule's e_ref is not vacuous."""
import numpy as np
import pytest
import torch

from codlad_amd.engine import Decoder
from oracle import vae_decode as odec
from tests import conditioning as cond
from tests import decoder_cases as dc


def _all_small_cases():
    return ([dc.indegree_case("N6"), dc.indegree_case("K4"), dc.cutoff_sweep_case()] + [dc.rows_case(M) for M in dc.ROWS_M]
            + [dc.existing_case(n) for n in dc.EXISTING])


def _csr_degrees(case):
    M = case["cg_xyz"].shape[0]
    ptr, src = Decoder.csr_from_pairs(case["pairs"], M)
    assert ptr.dtype == torch.int32 and src.dtype == torch.int32 and int(ptr[0]) == 0 and int(ptr[-1]) == src.numel()
    return ptr, src


@pytest.mark.parametrize("vae_type", ["N6", "K4"])
def test_indegree_case_has_the_listed_in_degrees(vae_type):
    c = dc.indegree_case(vae_type)
    M = c["cg_xyz"].shape[0]
    assert M == 260 and dc.is_angle(c) == (vae_type == "K4")
    ptr, src = _csr_degrees(c)
    deg = (ptr[1:] - ptr[:-1]).long()
    assert deg[:len(dc.INDEGREES)].tolist() == list(dc.INDEGREES) == [0, 1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 200]
    assert torch.equal(deg, dc.in_degrees(c))                      # the oracle's reading of the list is the engine's
    # every other residue: its true cutoff neighbourhood, up to a fourth 64-edge chunk
    true_deg = torch.bincount(dc._cutoff_pairs(c["cg_xyz"])[:, 0], minlength=M)
    assert torch.equal(deg[len(dc.INDEGREES):], true_deg[len(dc.INDEGREES):]) and int(deg.max()) > 192
    # the crafted receivers' senders are distinct, never the receiver itself, and arrive in list order
    for n, k in enumerate(dc.INDEGREES):
        s = src[int(ptr[n]):int(ptr[n + 1])].long()
        assert s.numel() == k and torch.unique(s).numel() == k and n not in s.tolist()
        assert torch.equal(s, c["pairs"][c["pairs"][:, 0] == n, 1])
    d = dc.kernel_distance(c["cg_xyz"], odec.directed(c["pairs"]))
    assert bool((d >= dc.CUTOFF).any()) and bool((d < dc.CUTOFF).any())            # crafted receivers reach past the cutoff
    a, b = c["coincident"]
    both = c["pairs"][(c["pairs"][:, 0] == a) & (c["pairs"][:, 1] == b)]
    assert both.shape[0] == 1 and float(dc.kernel_distance(c["cg_xyz"], both)) == pytest.approx(3e-8 ** 0.5, rel=1e-6)
    assert sorted(set(c["cg_z"].tolist())) == list(range(25))


def test_cutoff_sweep_case_has_every_distance_class():
    c = dc.cutoff_sweep_case()
    M = c["cg_xyz"].shape[0]
    assert 125 <= M <= 135
    ptr, _src = _csr_degrees(c)
    deg = (ptr[1:] - ptr[:-1]).long()
    rows, d, nominal = dc.sweep_rows(c)
    assert rows.numel() >= 64 and torch.unique(rows).numel() == rows.numel() and bool((deg[rows] == 1).all())
    assert len(set(map(str, nominal))) == 41
    below = float(np.nextafter(np.float32(21.0), np.float32(0.0)))
    for k, nom in enumerate(nominal):
        got = float(d[k])
        if nom == dc.SWEEP_FLOOR:
            assert got == pytest.approx(3e-8 ** 0.5, rel=1e-6) and got >= 1.7e-4       # refined_rcp's stated range
        elif nom == dc.SWEEP_BELOW:
            assert got == below and got < 21.0
        elif nom in (21.0, 21.5):
            assert got == nom                                     # exactly, as the kernel's formula computes it
        else:
            assert got == pytest.approx(nom, rel=2e-6) and got < 21.0
    assert int((d >= 21.0).sum()) == 4 and int((d == 21.0).sum()) == 2 and int((d < 21.0).sum()) == rows.numel() - 4
    # float64 sees the same sides of the cutoff at 21.0 and 21.5 (r = (d, 0, 0) exactly), so V is zero in every reference
    _nb, d64, rbf, env = odec.edge_geometry(c["cg_xyz"].double(), c["pairs"])
    first = d64[:len(dc.SWEEP_DISTANCES)]
    assert first.dtype == torch.float64
    assert bool(((first >= 21.0) == (d[:len(dc.SWEEP_DISTANCES)] >= 21.0)).all())
    out = first >= 21.0
    assert bool((env[:len(out)][out] == 0).all()) and bool((rbf[:len(out)][out] == 0).all())


@pytest.mark.parametrize("M", dc.ROWS_M)
def test_rows_cases(M):
    c = dc.rows_case(M)
    assert c["cg_xyz"].shape == (M, 3) and bool((c["pairs"][:, 1] > c["pairs"][:, 0]).all())          # undirected j > i
    ptr, _src = _csr_degrees(c)
    assert int(ptr[-1]) == 2 * c["pairs"].shape[0] and int((ptr[1:] - ptr[:-1]).min()) >= 1
    assert torch.equal(c["cg_xyz"], dc.rows_case(129)["cg_xyz"][:M])


def test_persistent_case_is_larger_than_the_grid_of_a_256_cu_part():
    job, offs = dc.persistent_case()
    M = job["cg_xyz"].shape[0]
    assert M == 48 * 87 + 46 == 4222 > 16 * 256 and offs[-1] == M and len(offs) == 50
    parts = dc.persistent_parts()
    assert not torch.equal(parts[0]["z_q"], parts[1]["z_q"]) and torch.equal(parts[0]["cg_xyz"], parts[47]["cg_xyz"])
    ptr, _src = _csr_degrees(job)
    for k in (0, 24, 47, 48):
        p, _ = _csr_degrees(parts[k])
        assert torch.equal((ptr[1:] - ptr[:-1])[offs[k]:offs[k + 1]], p[1:] - p[:-1])
    assert offs[47] < 16 * 256 < offs[48]            # the last 87-copy straddles the grid, the 46-residue part is beyond it


def test_a_graph_without_edges():
    for M in (1, 5):
        c = dc.no_edges_case(M)
        ptr, src = Decoder.csr_from_pairs(c["pairs"], M)
        assert ptr.tolist() == [0] * (M + 1) and src.numel() == 0 and src.dtype == torch.int32
        _ic, taps = dc.oracle_run(c, torch.float64)
        assert all(bool((taps[f"v{i}"] == 0).all()) for i in range(4))


@pytest.mark.parametrize("case", _all_small_cases(), ids=lambda c: c["name"])
def test_references_are_float64_and_the_rule_is_not_vacuous(case):
    """The float64 oracle returns float64 (dc.oracle_run asserts it for every tap); the fp32 oracle has a non-zero error
    against it in every computed channel; the channels where it has none, so that FLOOR alone sets the bound, are exactly
    the table channels, where fp32 and float64 hold the same table entry."""
    ref = dc.references(case)
    ic32, ic64 = ref["ic"]
    assert ic64.dtype == torch.float64 and ic32.dtype == torch.float32
    e_ic, e_S = dc.e_ref_of(ic32, ic64), dc.e_ref_of(*ref["S"])
    table = dc.table_channels(dc.is_angle(case))
    assert (e_ic == 0).nonzero().flatten().tolist() == table and len(table) == (13 if dc.is_angle(case) else 23)
    assert bool((e_S > 0).all())
    assert torch.equal(ic32[:, table].double(), ic64[:, table])
    computed = [ch for ch in range(39) if ch not in table]
    assert float(e_ic[computed].max()) < 1e-4 and float(e_S.max()) < 1e-4          # and fp32 is still fp32
    # the fp32 oracle obeys the rule against itself
    for got, (r32, r64) in ((ic32, ref["ic"]), (ref["S"][0], ref["S"])):
        assert dc.worst_ratio(got, r32, r64)[0] <= 1.0


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("case", [dc.indegree_case("K4"), dc.cutoff_sweep_case(), dc.existing_case("realC2_state_L87_B2")],
                         ids=lambda c: c["name"])
def test_oracle_taps_reassemble_into_its_output(case, dtype):
    sd = cond.to_dtype(dc.state_dict_of(case["weights"]), dtype)
    ic, taps = dc.oracle_run(case, dtype)
    assert sorted(taps) == sorted(["S0"] + [f"{k}{i}" for i in range(4) for k in ("phi", "v")] + [f"S{i}" for i in range(1, 5)])
    if not case["latent_is_state"]:
        assert torch.equal(taps["S0"][:, :36], torch.nn.functional.linear(case["z_q"].to(dtype), sd["map_out.weight"],
                                                                          sd["map_out.bias"]))
    else:
        assert torch.equal(taps["S0"][:, :36], case["z_q"].to(dtype))
    for i in range(4):
        assert torch.equal(taps[f"phi{i}"], odec.block_phi(sd, i, taps[f"S{i}"]))
        assert torch.equal(taps[f"v{i}"], odec.message_sum(sd, i, taps[f"phi{i}"], case["cg_xyz"], case["pairs"]))
        assert torch.equal(taps[f"S{i + 1}"], odec.dense_update(sd, i, taps[f"S{i}"], taps[f"v{i}"]))
    assert torch.equal(ic, odec.heads(sd, taps["S4"], case["cg_z"], dc.is_angle(case)))
    # a substituted phi is used: the block's own gives the same bits, another one changes the sum and what follows
    same, _ = dc.oracle_run(case, dtype, phi_sub={3: taps["phi3"]})
    assert torch.equal(same, ic)
    other, t2 = dc.oracle_run(case, dtype, phi_sub={3: torch.zeros_like(taps["phi3"])})
    assert bool((t2["v3"] == 0).all()) and torch.equal(t2["S3"], taps["S3"]) and not torch.equal(other, ic)
    # a float32 phi handed to the float64 sum is cast up, not the sum down
    v = odec.message_sum(sd, 3, taps["phi3"].float(), case["cg_xyz"], case["pairs"])
    assert v.dtype == dtype


def test_in_degree_one_rows_are_one_filter_times_one_phi_row():
    c = dc.cutoff_sweep_case()
    sd = cond.to_dtype(dc.state_dict_of(c["weights"]), torch.float64)
    _ic, taps = dc.oracle_run(c, torch.float64)
    rows, d, _nominal = dc.sweep_rows(c)
    n = len(dc.SWEEP_DISTANCES)
    senders = torch.cat([rows[n:], rows[:n]])
    nb, _d, rbf, env = odec.edge_geometry(c["cg_xyz"].double(), c["pairs"])
    assert torch.equal(nb[:2 * n, 0], rows) and torch.equal(nb[:2 * n, 1], senders)
    filt = odec._lin(sd, "equivaraintconv.message_blocks.3.dist_embed.block.1", rbf[:2 * n]) * env[:2 * n, None]
    assert torch.equal(taps["v3"][rows], taps["phi3"][senders] * filt)
    assert bool((taps["v3"][rows][d >= 21.0] == 0).all()) and bool((taps["v3"][rows][d < 20.0].abs().amax(1) > 0).all())


def test_read_taps_follows_the_documented_scratch_layout():
    """S^T [40][M] | V [M][40] | phi_a [M][40] | phi_b [M][40] (csrc/ic_decoder_kernels.hip); block 3 reads plane 1."""
    M = 7
    S, V, pa, pb = (torch.randn(M, 40, generator=torch.Generator().manual_seed(s)) for s in range(4))
    scratch = torch.cat([S.t().reshape(-1), V.reshape(-1), pa.reshape(-1), pb.reshape(-1), torch.zeros(40 * M)]).reshape(M, 200)
    taps = Decoder.read_taps(scratch)
    assert torch.equal(taps["S"], S) and torch.equal(taps["V"], V) and torch.equal(taps["phi2"], pa) and torch.equal(taps["phi3"], pb)
    scratch.zero_()
    assert torch.equal(taps["S"], S)                                       # copies, not views
