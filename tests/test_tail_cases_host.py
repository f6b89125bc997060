"""CPU: the cases and rules of tests/tail_cases.py are what they claim to be, with the fp32 oracle standing in for the device.

The GPU test (test_tail_fp64_parity.py) only means something if the chain sine really belongs to the float64 coordinates
of the oracle, if no designed placement is degenerate, if the fp32 restatement of each kernel's formula keeps the stated
tolerances itself, and if the margins flag few decisions and the fp32 oracle satisfies the margin rule alone.  Prints, per
case: E_ref and the floor, the below-margin shares, and the arccos / atan2 comparison (run with -s to see them)."""
import numpy as np
import pytest
import torch

from codlad_amd import synth
from codlad_amd.utils import dataset_builder as db
from oracle import vae_decode as odec
from tests import cases
from tests import tail_cases as tc


# ---------------------------------------------------------------------------------------------------------------------
# 1. ic -> xyz
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", tc.XYZ_CASES)
def test_chain_sine_rule_on_the_fp32_oracle(name):
    case = tc.xyz_case(name)
    ref = tc.xyz_reference(case)
    x64 = odec.ic_to_xyz(case["og"].double(), case["ic"].double(), case["info"])
    assert x64.dtype == torch.float64 and torch.equal(ref["x64"], x64)          # the sine's coordinates are the oracle's
    s = ref["s"]
    assert s.shape == x64.shape[:2] and bool(torch.isfinite(x64).all()) and bool(torch.isfinite(s).all())
    assert float(s.max()) <= 1.0 + 1e-12 and float(s.min()) > 0.0
    ratio, f, a, err, sa = tc.worst_atom(ref["x32"], ref["x64"], s, ref["scale"])
    print(f"tail ic->xyz {name}: E_ref {ref['e_ref']:.2e} A, floor {ref['floor']:.2e} A, smallest s {float(s.min()):.2e}, "
          f"fp32 oracle worst err {float((ref['x32'].double() - x64).norm(dim=-1).max()):.2e} A, worst err x s / scale "
          f"{ratio:.2f} (frame {f} atom {a}: err {err:.2e}, s {sa:.2e})")
    assert ratio <= 1.0 + 1e-12                                                  # trivially: E_ref is this maximum
    if case["designed"]:
        assert float(s.min()) >= tc.S_MIN, f"{name}: a placement with s = {float(s.min()):.2e}: choose another seed"
    # the rule's flatness: E_ref stays a small multiple of one rounding of the largest coordinate (a chain is at most 7
    # placements deep, each adding about one such rounding), whatever the plain error does - so the bound is not vacuous
    assert 0.0 < ref["e_ref"] <= 8 * ref["floor"]


def test_chain_sine_is_one_on_ca_and_carried_along_the_chain():
    case = tc.xyz_case("trp_arg")
    ref = tc.xyz_reference(case)
    names = [synth.IDX2THR[int(z)] for z in case["z"]]
    atoms = [a for nm in names for a in synth.PDB_ATOM_ORDER[nm]]
    s = ref["s"][0]
    assert all(float(s[k]) == 1.0 for k, a in enumerate(atoms) if a == "CA")
    first = 0
    for nm in names:                                 # along TRP's and ARG's chains s never grows: CB >= CG >= CD ...
        at = synth.PDB_ATOM_ORDER[nm]
        chain = ["CB", "CG", "CD", "NE", "CZ", "NH1"] if nm == "ARG" else ["CB", "CG", "CD1", "NE1"]
        v = [float(s[first + at.index(a)]) for a in chain]
        assert v == sorted(v, reverse=True), (nm, v)
        first += len(at)


def test_designed_ic_cases_hold_what_they_aim_at():
    c = tc.xyz_case("angles")
    ic, leaf = c["ic"], torch.from_numpy(tc.leaf_slots(c["z"]))[None].expand(2, -1, -1)
    f32 = lambda v: float(np.float32(v))                                         # noqa: E731
    for v in tc.ANGLE_SPECIALS:                                                  # every special value in the torsions
        assert int((ic[..., 2] == f32(v)).sum()) > 0, v
    for v in (tc.PI / 2, -tc.PI / 2, 50.0, -50.0):
        assert int((ic[..., 1] == f32(v)).sum()) > 0, v
    multiple = torch.zeros_like(leaf)
    for v in (0.0, tc.PI, 2 * tc.PI, -3 * tc.PI, 7 * tc.PI, -7 * tc.PI):
        hit = ic[..., 1] == f32(v)
        assert int(hit.sum()) > 0, v
        multiple |= hit
    assert bool((multiple <= leaf).all())
    for ch in (1, 2):
        assert int(((ic[..., ch].abs() < 0.05) & (ic[..., ch] != 0)).sum()) > 5
        assert int((((ic[..., ch] - tc.PI).abs() < 0.05) & (ic[..., ch] != f32(tc.PI))).sum()) > 5
    assert int((ic[..., 0] < 0).sum()) > 100 and int((ic[..., 0] == f32(1e-3)).sum()) > 10
    assert bool(((ic[..., 0] == f32(1e-3)) <= leaf).all())
    assert float(ic[..., 1:].abs().max()) == 50.0

    z = tc.xyz_case("zero_component")
    ca = z["og"][:, :, 1:]
    d = ca[:, 1:] - ca[:, :-1]
    assert bool((d[0, :, 2] == 0).all()) and bool((ca[0, :, 2] == 5.0).all())        # the plane z = 5
    assert bool(((d[1] == 0).sum(-1) == 2).all())                                    # axis-parallel steps
    assert bool((d[2, 0::2, 0] == 0).all()) and bool((d[2, 1::2, 0] != 0).all())     # x shared in pairs
    far, near = tc.xyz_case("far"), tc.xyz_case("synth_L46x3")
    assert torch.equal(far["ic"], near["ic"])
    assert float((far["og"][:, :, 1:] - near["og"][:, :, 1:] - torch.tensor(tc.SHIFT)).abs().max()) < 1e-4
    rf, rn = tc.xyz_reference(far), tc.xyz_reference(near)
    assert rf["floor"] > 1e-4 and rf["scale"] >= rf["floor"]                         # the floor carries the far bound
    # the second assertion of the far test, on the fp32 oracle: x_far - shift against the untranslated float64 result
    back = rf["x32"].double() - torch.tensor(tc.SHIFT, dtype=torch.float64)
    assert tc.worst_atom(back, rn["x64"], rn["s"], rf["scale"])[0] <= tc.C
    assert sorted(B * L for B, L in tc.ROWS) == [1, 2, 127, 128, 129, 129] and (3, 43) in tc.ROWS
    names = {synth.IDX2THR[int(k)] for k in tc.xyz_case("all_types")["z"]}
    assert names == set(synth.IDX2THR) and {"TPO", "SEP"} <= names
    assert {synth.IDX2THR[int(k)] for k in tc.xyz_case("gly")["z"]} == {"GLY"}
    assert tc.xyz_reference(tc.xyz_case("gly"))["x64"].shape[1] == 12 * 4
    assert {synth.IDX2THR[int(k)] for k in tc.xyz_case("trp_arg")["z"]} == {"TRP", "ARG"}


def test_group_lists_have_the_listed_shapes():
    rows = {n: [c["ic"].shape[0] * c["ic"].shape[1] for c in tc.group_list(n)] for n in tc.GROUP_LISTS}
    assert [len(rows[n]) for n in tc.GROUP_LISTS] == [1, 2, 3, 17]
    assert rows["one_row"] == [1] and rows["three_total_128"][0] == 1 and sum(rows["three_total_128"]) == 128
    a, b = tc.group_list("same_protein_twice")
    assert a["info"] is b["info"] and torch.equal(a["og"], b["og"]) and not torch.equal(a["ic"], b["ic"])
    r17 = rows["seventeen"]
    assert r17.count(1) == 6 and sum(r17) > 256                                     # 1-row groups between blocks
    starts = np.cumsum([0] + r17)[:-1] % 128
    assert len(set(starts.tolist())) >= 15                                           # boundaries all over a block
    for n in tc.GROUP_LISTS:
        for c in tc.group_list(n):
            assert float(tc.xyz_reference(c)["s"].min()) >= tc.S_MIN, c["name"]


# ---------------------------------------------------------------------------------------------------------------------
# 2. xyz -> ic
# ---------------------------------------------------------------------------------------------------------------------
def _hold_ic(label, got, xyz, quads, labels=None):
    return tc.hold_ic(label, got, xyz, quads, labels)


def test_designed_quads_atan2_restatement_keeps_the_tolerances_and_arccos_does_not():
    d = tc.designed_quads()
    ic64, tol, ok, collinear = tc.ic_reference(d["xyz"], d["quads"])
    lab = d["label"]
    n = d["first_far"]
    k = lab.index
    assert ic64[0, k("angle_0"), 1] == 0.0 and ic64[0, k("angle_pi"), 1] == np.pi
    assert collinear[0, k("angle_0")] and collinear[0, k("angle_pi")] and collinear[0, :n].sum() == 2
    assert abs(ic64[0, k("angle_1e-4"), 1] - 1e-4) < 1e-7 and abs(ic64[0, k("angle_pi-1e-4"), 1] - (np.pi - 1e-4)) < 1e-7
    assert 0 < ic64[0, k("dihedral_0+"), 2] < 2e-6 and 0 < 2 * np.pi - ic64[0, k("dihedral_0-"), 2] < 2e-6
    assert ic64[0, k("dihedral_0"), 2] == 0.0 and abs(ic64[0, k("dihedral_+pi"), 2] - np.pi) < 1e-12
    assert 0 < np.pi - ic64[0, k("dihedral_pi-"), 2] < 2e-6 and 0 < ic64[0, k("dihedral_pi+"), 2] - np.pi < 2e-6
    assert sorted(np.round(ic64[0, [k("dihedral_+pi/2"), k("dihedral_-pi/2")], 2] / np.pi, 6)) == [0.5, 1.5]
    assert not ok[k("negative_index")] and ok.sum() == len(lab) - 2
    assert np.abs(d["xyz"][0, 4 * n:] - d["xyz"][0, :4 * n] - np.array(tc.SHIFT, dtype=np.float32)).max() < 1e-3
    worst = _hold_ic("designed, atan2 form", tc.ic_fp32(d["xyz"], d["quads"]), d["xyz"], d["quads"], lab)
    print(f"tail xyz->ic designed quads, fp32 atan2 restatement: worst err / tol distance {worst[0]:.2f}, angle {worst[1]:.2f}, "
          f"dihedral {worst[2]:.2f}")
    acos = tc.ic_fp32(d["xyz"], d["quads"], form="arccos")
    err = tc.ic_error(acos, ic64)[0, :, 1] / tol[0, :, 1]
    for q in (k("angle_0"), k("angle_pi"), k("angle_1e-4"), k("angle_pi-1e-4")):
        print(f"tail xyz->ic {lab[q]}: arccos form off by {err[q] * tol[0, q, 1]:.2e} rad = {err[q]:.0f} x the tolerance; atan2 "
              f"form {tc.ic_error(tc.ic_fp32(d['xyz'], d['quads']), ic64)[0, q, 1]:.2e} rad")
    assert err[k("angle_1e-4")] > 10 or err[k("angle_pi-1e-4")] > 10, "arccos would do: the atan2 form is not needed"


@pytest.mark.parametrize("name", list(cases.DECODER_CASES))
def test_golden_frames_atan2_restatement_and_round_trip_budget(name):
    rt = tc.round_trip_reference(name)
    worst = _hold_ic(name, tc.ic_fp32(rt["full"], rt["quads"]), rt["full"], rt["quads"])
    print(f"tail xyz->ic {name}: fp32 atan2 restatement worst err / tol distance {worst[0]:.2f}, angle {worst[1]:.2f}, dihedral "
          f"{worst[2]:.2f}; round trip E_ref {rt['e_ref']:.2e} A, floor {rt['floor']:.2e} A, smallest s {float(rt['s'].min()):.2e}")
    assert rt["e_ref"] > 0 and rt["x0"].dtype == torch.float64
    for F, Q in tc.THREAD_COUNTS:
        assert F <= rt["full"].shape[0] or name != "N6_L46_B3"
        assert Q <= rt["quads"].shape[0]
    assert sorted(F * Q for F, Q in tc.THREAD_COUNTS) == [255, 256, 257]


# ---------------------------------------------------------------------------------------------------------------------
# 3. decisions
# ---------------------------------------------------------------------------------------------------------------------
def _share(below, total):
    return below / max(total, 1)


@pytest.mark.parametrize("size", tc.VQ_SIZES)
def test_vq_margin_rule_on_the_fp32_oracle(size):
    cb = tc.vq_codebook(size)
    assert cb.shape == (size, 3) and torch.unique(cb, dim=0).shape[0] == size
    ranges = tc.vq_wave_ranges(size)
    assert ranges[0][0] == 0 and max(b for _a, b in ranges) == size and sum(b - a for a, b in ranges) == size
    if size < 16 or size == 17:
        assert any(a == b for a, b in ranges)                                   # empty wave ranges
    below = total = 0
    for n in tc.VQ_N:
        for k, scale in enumerate(tc.VQ_SCALES):
            lat = tc.vq_denormalise(tc.vq_inputs(n, scale, 9100 + 10 * n + k))
            idx64, flagged, idx32 = tc.vq_reference(lat, cb)
            assert torch.equal(tc.mixed(flagged, idx32, idx64), idx32), (size, n, scale)   # the oracle alone keeps the rule
            below += int(flagged.sum())
            total += n
    print(f"tail VQ {size} codes: {below} of {total} lookups below the margin bound ({100 * _share(below, total):.3f} %)")
    assert _share(below, total) <= tc.MAX_BELOW_SHARE


@pytest.mark.parametrize("size,i,j,aim", tc.VQ_TIES)
def test_vq_planted_ties(size, i, j, aim):
    cb = tc.vq_tie_codebook(size, i, j)
    ranges = tc.vq_wave_ranges(size)
    wave = lambda c: next(w for w, (a, b) in enumerate(ranges) if a <= c < b)        # noqa: E731
    if "inside" in aim:
        assert wave(i) == wave(j)
        if "shorter" in aim:
            a, b = ranges[wave(i)]
            assert wave(i) == 15 and b - a < ranges[0][1] - ranges[0][0] and size % 16 != 0
    else:
        assert wave(i) != wave(j)
    lat = tc.vq_denormalise(tc.vq_tie_inputs(cb, i, j))
    idx64, flagged, idx32 = tc.vq_reference(lat, cb)
    assert bool((idx64 == min(i, j)).all()) and bool((idx32 == min(i, j)).all()) and not bool(flagged.any())


@pytest.mark.parametrize("cutoff", tc.CG_CUTOFFS)
def test_cg_margin_rule_on_the_fp32_oracle(cutoff):
    job = tc.cg_job()
    lens = job["lens"]
    assert lens[:8] == list(tc.CG_SAMPLES) and lens[8] == 65 and lens[9:] == [4, 4] and sum(lens) % 4 != 0
    o65 = sum(lens[:tc.CG_SAMPLES.index(65)])
    assert torch.equal(job["xyz"][o65:o65 + 65], job["xyz"][sum(lens[:8]):sum(lens[:9])])
    want, flagged, st = tc.cg_reference(job, cutoff)
    print(f"tail CG graph cutoff {cutoff}: {st['below']} of {st['pairs']} pairs below the margin bound "
          f"({100 * _share(st['below'], st['pairs']):.4f} %), {st['planted']} planted, {int(want.sum()) // 2} pairs inside; "
          f"fp32 differs from float64 on {st['fp32_differs_from_fp64']}")
    assert st["oracle_ok"] and _share(st["below"], st["pairs"]) <= tc.MAX_BELOW_SHARE
    assert bool((want == want.t()).all()) and int(want.sum()) > 1000
    p0 = job["planted"][cutoff]
    x = job["xyz"][p0:p0 + 4, 0].tolist()
    assert x[0] == 0.0 and x[1] == cutoff and x[2] > cutoff > x[3]
    assert [bool(want[p0, p0 + k]) for k in (1, 2, 3)] == [True, False, True]
    ptr, src = tc.cg_expected_csr(want)
    assert tc.cg_order_ok(ptr, src) and torch.equal(tc.cg_adjacency(ptr, src), want)


def test_bond_margin_rule_on_the_fp32_oracle():
    job = tc.bond_job()
    assert job["num_atoms"][:8] == [1, 2, 3, 255, 256, 257, 700, 4200] and (max(job["num_atoms"]) + 7) // 8 > 512
    assert set(job["atomic_nums"].tolist()) == set(tc.BOND_ELEMENTS)
    ref = tc.bond_reference()
    for n, r in zip(job["num_atoms"], ref):
        print(f"tail bond graph {n} atoms: counts {r['want']}, {r['below']} of {r['pairs']} pair decisions below the margin bound")
        assert r["want"] == r["oracle"]                                         # the oracle alone keeps the rule
        if n != 4:
            assert _share(r["below"], r["pairs"]) <= tc.MAX_BELOW_SHARE
    assert ref[-1]["want"] == job["planted_counts"] and ref[-1]["below"] == 4   # planted: both pairs, both coordinate sets
    big = ref[7]["want"]
    assert big[0] > 3000 and big[2] > 100 and 0 < big[3] < big[0]               # bonds exist, differ, and hydrogens matter
    assert ref[0]["want"] == [0] * 6


def test_clash_margin_rule_on_the_fp32_oracle():
    job = tc.clash_job()
    r = tc.clash_reference(job)
    print(f"tail clash: {r['below']} of {r['n']} pairs below the margin bound ({100 * _share(r['below'], r['n']):.3f} %), count "
          f"{r['want']} (fp32 {r['count32']}, float64 {r['count64']})")
    assert r["want"] == r["count32"] and r["planted_ok"]
    sq = (job["xyz"][job["pairs"][:, 0]] - job["xyz"][job["pairs"][:, 1]]) ** 2
    v = ((sq[:, 0] + sq[:, 1]) + sq[:, 2]) + torch.tensor(tc.CLASH_EPS, dtype=torch.float32)
    print(f"tail clash: torch's float32 sqrt differs from the correctly rounded one on {int((torch.sqrt(v) != tc.sqrt32(v)).sum())} "
          f"of {v.numel()} values on this CPU (why the in-margin oracle uses sqrt32)")
    x = torch.tensor([2.0, 3.0, 1.44, 21.0 ** 2, 2.0934098], dtype=torch.float32)
    assert tc.sqrt32(x).tolist() == [float(np.sqrt(np.float32(t))) for t in x.tolist()]      # numpy's is the IEEE one
    assert 0 < r["below"] and _share(r["below"], r["n"]) <= tc.MAX_BELOW_SHARE
    assert 500 < r["want"] < 1500
    d = tc.clash_dist32(job["xyz"], job["pairs"])
    rows = sorted(job["planted"])
    assert float(d[rows[0]]) < float(np.float32(1.2)) <= float(d[rows[1]])
    dx = (job["xyz"][job["pairs"][rows, 1], 0] - job["xyz"][job["pairs"][rows, 0], 0]).numpy()
    assert np.nextafter(dx[0], np.float32(2)) == dx[1]                          # neighbouring float32 separations
