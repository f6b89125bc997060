"""GPU: everything after the IC decoder against float64 - per atom, per quad and per decision.

The tail's counterpart of test_decoder_fp64_parity.py, through the Python entry points (Decoder.ic_to_xyz,
Decoder.ic_to_xyz_groups, Decoder.vq, Decoder.build_csr, dataset_builder.xyz_to_ic, metrics.bond_graph_counts,
metrics.clash_result).  Cases and rules: tests/tail_cases.py (held to what they claim by tests/test_tail_cases_host.py).

  ic -> xyz   err_hip[atom] x s[atom] <= 4 x max(E_ref, 2^-23 x max|x64|), s the chain sine: no atom is left out;
  xyz -> ic   per quad: distance within 4 x 2^-23 max|x|, bond angle within 4 max(u, 2^-23), dihedral within that over the
              smaller sine of its two bond angles, u = 2^-23 max|x| / the quad's shortest bond;
  decisions   the float64 decision wherever its margin exceeds the rounding bound, the fp32 oracle's below it, planted
              ties by the first-index / <= / < rule itself.

Measured ratios and below-margin counts: DESIGN.md section 2, "The decoder tail against float64".
"""
import numpy as np
import pytest
import torch

from codlad_amd import metrics as gm
from codlad_amd import synth
from codlad_amd.engine import Decoder
from codlad_amd.utils import dataset_builder as db
from tests import cases
from tests import tail_cases as tc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

_dec = {}


def decoder():
    if "d" not in _dec:
        _dec["d"] = Decoder(synth.vqvae_state_dict("N6", "PED", cases.VAE_SEED), DEV)
    return _dec["d"]


# ---------------------------------------------------------------------------------------------------------------------
# 1. ic -> xyz
# ---------------------------------------------------------------------------------------------------------------------
def device_xyz(case):
    out = decoder().ic_to_xyz(case["og"][:, :, 1:].to(DEV), case["ic"].to(DEV), case["info"])
    torch.cuda.synchronize()
    return out.cpu()


def hold_atoms(label, xyz, x64, s, scale):
    ratio, f, a, err, sa = tc.worst_atom(xyz, x64, s, scale)
    msg = (f"fp64 parity tail ic->xyz {label}: err x s / max(E_ref, floor) {ratio:.2f} at frame {f} atom {a} (err {err:.2e} A, "
           f"s {sa:.2e}, scale {scale:.2e} A)")
    print(msg)
    assert xyz.shape == x64.shape and bool(torch.isfinite(xyz).all()), label
    assert ratio <= tc.C, msg
    return ratio


@pytest.mark.parametrize("name", tc.XYZ_CASES)
def test_ic_to_xyz_per_atom(name):
    """The golden geometries with the internal coordinates an untrained decoder emitted, synthetic ic, angles far outside
    (-pi, pi] and at the multiples of pi / 2, negative and 1e-3 A bonds, CA differences with exactly zero components, a
    frame 1 500 A from the origin, B x L around the 128-thread block, and every residue table."""
    case = tc.xyz_case(name)
    ref = tc.xyz_reference(case)
    xyz = device_xyz(case)
    hold_atoms(name, xyz, ref["x64"], ref["s"], ref["scale"])
    if name == "far":                                  # the translation costs what the floor says and nothing else
        near = tc.xyz_reference(tc.xyz_case(case["near"]))
        back = xyz.double() - torch.tensor(tc.SHIFT, dtype=torch.float64)
        hold_atoms("far - shift against the untranslated float64", back, near["x64"], near["s"], ref["scale"])


def _device_groups(group_cases):
    return [(c["og"][:, :, 1:].to(DEV), c["ic"].to(DEV), c["info"]) for c in group_cases]


@pytest.mark.parametrize("name", tc.GROUP_LISTS)
def test_ic_to_xyz_groups_per_atom(name):
    """1, 2, 3 and 17 groups in one launch (1-row groups, group boundaries all over a block, exactly 128 rows, one protein
    twice with different ic): bit-equal to one launch per group, and every atom within the bound.  reuse=True after a
    call with another group list builds a fresh table."""
    dec = decoder()
    group_cases = tc.group_list(name)
    groups = _device_groups(group_cases)
    want = [dec.ic_to_xyz(*g) for g in groups]
    got = dec.ic_to_xyz_groups(groups)
    assert len(got) == len(want) and all(torch.equal(g, w) for g, w in zip(got, want))
    other = _device_groups(tc.group_list("three_total_128" if name != "three_total_128" else "seventeen"))
    dec.ic_to_xyz_groups(other, reuse=True)
    for _ in range(2):                                 # the second call replays the cached table into the same outputs
        again = dec.ic_to_xyz_groups(groups, reuse=True)
        assert all(torch.equal(g, w) for g, w in zip(again, want))
    worst = 0.0
    for c, g in zip(group_cases, got):
        ref = tc.xyz_reference(c)
        worst = max(worst, tc.worst_atom(g.cpu(), ref["x64"], ref["s"], ref["scale"])[0])
        hold = tc.worst_atom(g.cpu(), ref["x64"], ref["s"], ref["scale"])
        assert hold[0] <= tc.C, (c["name"], hold)
    print(f"fp64 parity tail ic->xyz groups {name}: worst err x s / max(E_ref, floor) {worst:.2f} over {len(got)} groups")


# ---------------------------------------------------------------------------------------------------------------------
# 2. xyz -> ic
# ---------------------------------------------------------------------------------------------------------------------
def device_ic(xyz, quads):
    out = db.xyz_to_ic(torch.as_tensor(xyz).to(DEV), quads)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def test_xyz_to_ic_designed_quads():
    """Bond angles of exactly 0 and pi (atan2 must hold them; the dihedral is undefined there), of 1e-4 and pi - 1e-4,
    dihedrals at 0+, 0-, 0, +-pi and +-pi/2, a negative index between valid ones, and all of it again 1 500 A away."""
    d = tc.designed_quads()
    got = device_ic(d["xyz"], d["quads"])
    worst = tc.hold_ic("designed quads", got, d["xyz"], d["quads"], d["label"])
    k = d["label"].index
    assert got[0, k("angle_0"), 1] == 0.0 and abs(float(got[0, k("angle_pi"), 1]) - np.pi) <= tc.C * tc.FLOOR_ULP
    assert (got[0, k("negative_index")] == 0).all() and (got[0, k("negative_index_far")] == 0).all()
    assert (got[..., 1] >= 0).all() and (got[..., 1] <= np.float32(np.pi)).all()
    assert (got[..., 2] >= 0).all() and (got[..., 2] <= np.float32(2 * np.pi)).all()
    print(f"fp64 parity tail xyz->ic designed quads: worst err / tol distance {worst[0]:.2f}, angle {worst[1]:.2f}, dihedral "
          f"{worst[2]:.2f}")


@pytest.mark.parametrize("name", list(cases.DECODER_CASES))
def test_xyz_to_ic_per_quad_and_round_trip_per_atom(name):
    """The golden frames per quad, and xyz -> ic -> xyz on the device per atom against the original coordinates, E_ref from
    the fp32 oracle's own round trip."""
    rt = tc.round_trip_reference(name)
    got = device_ic(rt["full"], rt["quads"])
    worst = tc.hold_ic(name, got, rt["full"], rt["quads"])
    print(f"fp64 parity tail xyz->ic {name}: worst err / tol distance {worst[0]:.2f}, angle {worst[1]:.2f}, dihedral {worst[2]:.2f}")
    B, L = rt["og"].shape[0], rt["og"].shape[1] - 2
    back = decoder().ic_to_xyz(rt["og"][:, :, 1:].to(DEV), torch.from_numpy(got).to(DEV).reshape(B, L, 13, 3), rt["info"]).cpu()
    hold_atoms(f"{name} round trip", back, rt["x0"], rt["s"], rt["scale"])


@pytest.mark.parametrize("F,Q", tc.THREAD_COUNTS)
def test_xyz_to_ic_thread_counts(F, Q):
    """n_frames x n_quads = 255, 256 and 257 around the 256-thread block."""
    rt = tc.round_trip_reference("N6_L46_B3")
    xyz, quads = rt["full"][:F], rt["quads"][:Q]
    got = device_ic(xyz, quads)
    assert got.shape == (F, Q, 3)
    tc.hold_ic(f"{F} x {Q}", got, xyz, quads)
    whole = device_ic(rt["full"], rt["quads"])
    assert np.array_equal(got, whole[:F, :Q])


# ---------------------------------------------------------------------------------------------------------------------
# 3. decisions
# ---------------------------------------------------------------------------------------------------------------------
def vq_decoder(codebook):
    return Decoder(tc.vq_state_dict(codebook), DEV, torch.tensor(tc.VQ_MEAN), torch.tensor(tc.VQ_STD))


def device_vq(dec, x, codebook):
    idx, zq, lat = dec.vq(x.to(DEV))
    torch.cuda.synchronize()
    idx, zq, lat = idx.cpu(), zq.cpu(), lat.cpu()
    assert torch.equal(lat, tc.vq_denormalise(x)), "latent_out is not the separately rounded x * std + mean"
    assert int(idx.min()) >= 0 and int(idx.max()) < codebook.shape[0] and torch.equal(zq, codebook[idx])
    return idx, lat


@pytest.mark.parametrize("size", tc.VQ_SIZES)
def test_vq_lookup_against_float64_by_margin(size):
    """Codebooks of 1 .. 9000 codes (empty and short wave ranges; 9000 above the 64 KB attribute switch), n = 1, 63, 64, 65
    and 1000, latents at scales 1, 5 and 50, with a real de-normalisation in front."""
    cb = tc.vq_codebook(size)
    dec = vq_decoder(cb)
    below = total = 0
    for n in tc.VQ_N:
        for k, scale in enumerate(tc.VQ_SCALES):
            idx, lat = device_vq(dec, tc.vq_inputs(n, scale, 9100 + 10 * n + k), cb)
            idx64, flagged, idx32 = tc.vq_reference(lat, cb)           # from the device's own latent_out
            want = tc.mixed(flagged, idx32, idx64)
            bad = (idx != want).nonzero().flatten().tolist()
            assert not bad, (f"{size} codes, n {n}, scale {scale}: lookups {bad[:8]} differ from float64 outside the margin "
                             f"(or from the fp32 oracle inside it)")
            below += int(flagged.sum())
            total += n
    print(f"fp64 parity tail VQ {size} codes: {total} lookups equal float64, {below} below the margin bound equal the fp32 oracle")
    assert below <= tc.MAX_BELOW_SHARE * total


@pytest.mark.parametrize("size,i,j,aim", tc.VQ_TIES)
def test_vq_lookup_planted_ties_take_the_first_index(size, i, j, aim):
    cb = tc.vq_tie_codebook(size, i, j)
    idx, _lat = device_vq(vq_decoder(cb), tc.vq_tie_inputs(cb, i, j), cb)
    assert bool((idx == min(i, j)).all()), f"a duplicated code {aim}: {sorted(set(idx.tolist()))} instead of {min(i, j)}"


@pytest.mark.parametrize("cutoff", tc.CG_CUTOFFS)
def test_cg_graph_against_float64_by_margin(cutoff):
    """Samples of 1, 2, 63, 64, 65, 128, 129 and 300 nodes in one job of 925 (no multiple of 4), one trace as two samples,
    planted pairs at exactly the cutoff (in) and at the float32 numbers on either side."""
    job = tc.cg_job()
    want, _flagged, st = tc.cg_reference(job, cutoff)
    ptr, src = decoder().build_csr(job["xyz"], job["lens"], cutoff=cutoff)
    torch.cuda.synchronize()
    ptr, src = ptr.cpu(), src.cpu()
    M = job["xyz"].shape[0]
    assert ptr.numel() == M + 1 and int(ptr[0]) == 0 and int(ptr[-1]) == src.numel()
    assert int(src.min()) >= 0 and int(src.max()) < M
    got = tc.cg_adjacency(ptr, src)
    p0 = job["planted"][cutoff]
    assert [bool(got[p0, p0 + k]) for k in (1, 2, 3)] == [True, False, True], "planted pairs: <= at the cutoff itself"
    assert [bool(got[p0 + k, p0]) for k in (1, 2, 3)] == [True, False, True]
    diff = (got != want).nonzero().tolist()
    assert not diff, f"cutoff {cutoff}: pairs {diff[:8]} differ from float64 outside the margin"
    assert tc.cg_order_ok(ptr, src), "senders are not j > i ascending, then j < i ascending"
    wptr, wsrc = tc.cg_expected_csr(want)
    assert torch.equal(ptr, wptr) and torch.equal(src, wsrc)
    print(f"fp64 parity tail CG graph cutoff {cutoff}: {st['pairs']} pairs equal float64, {st['below']} below the margin bound, "
          f"{st['planted']} planted")


def test_bond_graph_counts_against_float64_by_margin():
    """Structures of 1, 2, 3, 255, 256, 257, 700 and 4200 atoms and a planted one in ONE call (max_atoms 4200: the row cap
    of 512 is reached and rows loop), elements H, C, N, O, S, P; twice, for the integer atomics."""
    job, ref = tc.bond_job(), tc.bond_reference()
    args = (job["xyz"].to(DEV), job["xyz_recon"].to(DEV), job["num_atoms"], job["atomic_nums"])
    first = gm.bond_graph_counts(*args, scale=tc.BOND_SCALE).cpu()
    second = gm.bond_graph_counts(*args, scale=tc.BOND_SCALE).cpu()
    assert torch.equal(first, second)
    assert first[-1].tolist() == job["planted_counts"], "planted pairs: < at the threshold itself"
    for s, (n, r) in enumerate(zip(job["num_atoms"], ref)):
        assert first[s].tolist() == r["want"], f"structure {s} ({n} atoms): {first[s].tolist()} instead of {r['want']}"
    print(f"fp64 parity tail bond graph: {sum(r['pairs'] for r in ref)} pair decisions equal float64, "
          f"{sum(r['below'] for r in ref[:-1])} below the margin bound, 4 planted")


def test_clash_count_against_float64_by_margin():
    """The 1.2 A count of sqrt(d^2 + 1e-7) on 2000 near pairs and two planted pairs at neighbouring float32 separations on
    either side of the threshold: the COUNT, recovered from the ratio (the list has 2002 rows, a float32 ratio resolves
    1 / 2002 easily)."""
    job = tc.clash_job()
    ref = tc.clash_reference(job)
    xyz = job["xyz"].to(DEV)
    nbr, none = job["pairs"].to(DEV), torch.zeros(0, 2, dtype=torch.int64, device=DEV)
    assert torch.equal(gm.clash_list(none, nbr).cpu(), job["pairs"])
    n = job["pairs"].shape[0]
    ratio = float(gm.clash_result(none, nbr, xyz, none))
    count = round(ratio * n)
    assert abs(ratio * n - count) < 1e-3 and count == ref["want"], (ratio * n, ref)
    for row, inside in job["planted"].items():           # each planted pair alone: 1 or 0
        one = float(gm.clash_result(none, nbr[row:row + 1].clone(), xyz, none))
        assert one == (1.0 if inside else 0.0), (row, one)
    print(f"fp64 parity tail clash: count {count} of {n} equals float64, {ref['below']} below the margin bound, 2 planted")
