"""Secondary structure on the device (codlad_amd/csrc/dssp_kernels.hip through codlad_amd.metrics) against tests/dssp_ref.py.

Stage 1 (coordinates to bitmaps): a pair is UNDECIDED when |E64 + 0.5| <= 4 x max |E32 - E64| of the float32 restatement on
the same call's inputs; bends and links likewise.  acc, don and geom equal the float64 reference on every decided pair; the
planted cases have no undecided pair at all (tests/test_dssp_host.py holds their margins and the cap of the noisy copies on
the CPU).  don is the transpose of acc bit for bit.  Stage 2 (bitmaps to states) is integer work and is held exactly: to the
plain-loop reference run on the device's own bitmaps, and on hand-written and random bitmaps.

Measured on an MI355X (printed by every run): e_best deviates from float64 by 1.4e-6 .. 5.2e-5 kcal/mol per call, in every
call exactly the float32 restatement's own deviation; kappa by 5.6e-6 .. 2.4e-2 degrees (the largest at kappa = 0.01 degrees,
where acos is ill-conditioned; at most 3 x the restatement's); 0 undecided of 130 118 eligible pairs."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from codlad_amd import metrics
from tests import dssp_ref as dr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
UNDECIDED_CAP = 1e-4


def dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)                    # a copy: the cached inputs are read-only


def host(out):
    return {k: v.cpu().numpy() for k, v in out.items() if torch.is_tensor(v)}


def words(t):
    """int64 words of the device -> the uint64 bit patterns."""
    return t.view(np.uint64)


@functools.lru_cache(maxsize=None)
def sized_call(R):
    """The inputs of one call at size R: the planted structure and its noisy copies, with the references (computed once)."""
    top, x = dr.sized(R)
    xyz = np.concatenate([x[None], dr.noisy(x, 7 * R)])
    xyz.setflags(write=False)
    return top, xyz, dr.margins(xyz, top)


def check_stage1(out, m, R, planted_rows):
    """out: the device's tensors on the host; m: dr.margins of the same inputs.  -> (undecided, eligible) pair counts."""
    r64 = m["r64"]
    acc, don = dr.unpack_bits(words(out["acc"]), R), dr.unpack_bits(words(out["don"]), R)
    assert np.array_equal(don, acc.transpose(0, 2, 1))                                  # exactly the transpose
    und = m["undecided_e"]
    assert not (acc & ~r64["eligible"]).any()                                           # no bit outside the eligible pairs
    assert np.array_equal(acc[~und], r64["hb"][~und])
    W = (R + 63) // 64
    if R % 64:                                                                          # bits >= R of the last word are 0
        assert not (words(out["acc"])[..., W - 1] >> np.uint64(R % 64)).any()
        assert not (words(out["don"])[..., W - 1] >> np.uint64(R % 64)).any()
    link, bend = (out["geom"] & dr.GEOM_LINK) > 0, (out["geom"] & dr.GEOM_BEND) > 0
    assert not (out["geom"] & ~np.uint8(3)).any()
    assert np.array_equal(link[~m["undecided_d"]], r64["link"][~m["undecided_d"]])
    assert np.array_equal(bend[~m["undecided_k"]], r64["bend"][~m["undecided_k"]])
    for s in planted_rows:
        assert not und[s].any() and not m["undecided_k"][s].any() and not m["undecided_d"][s].any(), s
    # kappa: defined exactly where the reference defines it (away from an undecided link), within 4 x the deviation
    sure = ~np.isnan(r64["kappa"])
    touched = np.zeros_like(sure)
    if m["undecided_d"].any():
        for s, r in zip(*np.nonzero(m["undecided_d"])):
            touched[s, max(r - 2, 0):r + 3] = True
    assert np.array_equal(np.isnan(out["kappa"])[~touched], ~sure[~touched])
    ok = sure & ~np.isnan(out["kappa"])
    dk = float(np.abs(out["kappa"][ok].astype(np.float64) - r64["kappa"][ok]).max()) if ok.any() else 0.0
    assert dk <= 4.0 * m["dev_k"] + 1e-30, (dk, m["dev_k"])
    # the lowest energies and their partners
    assert out["e_best"].dtype == np.float32 and out["partner"].dtype == np.int32
    clear = r64["gap"] > 4.0 * m["dev_e"]
    assert np.array_equal(out["partner"][clear], r64["partner"][clear])
    de = float(np.abs(out["e_best"].astype(np.float64) - r64["e_best"]).max())
    assert de <= 4.0 * m["dev_e"], (de, m["dev_e"])
    assert np.array_equal(out["partner"] < 0, r64["partner"] < 0) and (out["e_best"][out["partner"] < 0] == 0).all()
    assert out["finite"].all()
    print(f"R={R}: device e_best within {de:.2e} kcal/mol and kappa within {dk:.2e} deg of float64; restatement "
          f"{m['dev_e']:.2e} / {m['dev_k']:.2e}; undecided {int(und.sum())} of {int(r64['eligible'].sum())} eligible pairs")
    return int(und.sum()), int(r64["eligible"].sum())


@pytest.mark.gpu
@pytest.mark.parametrize("R", dr.SIZES)
def test_stage1_against_float64_at_every_size(R):
    top, xyz, m = sized_call(R)
    out = host(metrics.hbonds(dev(xyz), top))
    assert out["acc"].shape == (xyz.shape[0], R, (R + 63) // 64) and out["acc"].dtype == np.int64
    undecided, eligible = check_stage1(out, m, R, planted_rows=[0])
    assert undecided <= max(UNDECIDED_CAP * eligible, 0)


@pytest.mark.gpu
def test_stage1_and_the_labels_on_the_planted_cases():
    """Exact bitmaps (no undecided pair) and, end to end, exactly the hand-derived labels."""
    for name, (top, x, want) in dr.planted().items():
        m = dr.margins(x[None], top)
        res = metrics.dssp(dev(x[None]), top)
        out = host(res)
        R = top.n_residues
        undecided, _ = check_stage1(out, m, R, planted_rows=[0])
        assert undecided == 0, name
        assert np.array_equal(dr.unpack_bits(words(out["acc"]), R), m["r64"]["hb"]), name
        assert np.array_equal(out["geom"], m["r64"]["geom"]), name
        assert res["ss_string"] == [want], (name, res["ss_string"])
        assert out["counts"][0].tolist() == [want.count(c) for c in dr.CODES], name
        for c, key in enumerate(metrics.DSSP_NAMES):
            assert out[key].tolist() == [want.count(dr.CODES[c])], (name, key)
    # what the special cases plant shows in the bits
    top, x, _w = dr.planted()["helix_pro"]
    acc = dr.unpack_bits(words(host(metrics.hbonds(dev(x[None]), top))["acc"]), 14)[0]
    assert not acc[3, 7] and acc[2, 6] and acc[4, 8]
    top, x, _w = dr.planted()["sheet_anti"]
    assert host(metrics.dssp(dev(x[None]), top))["bridge"][0, 1:6, 1].tolist() == [12, 11, 10, 9, 8]


def assign_on_device(hb, link, bend, finite=None):
    """The pattern stage of the device on bitmaps given as matrices [S, R, R] / [S, R]."""
    acc, don = dr.pack_bits(hb)
    geom = (dr.GEOM_LINK * link + dr.GEOM_BEND * bend).astype(np.uint8)
    fin = np.ones(hb.shape[0], np.uint8) if finite is None else np.asarray(finite, np.uint8)
    return host(metrics.dssp_assign(dev(acc.view(np.int64)), dev(don.view(np.int64)), dev(geom), dev(fin))), geom, fin


@pytest.mark.gpu
@pytest.mark.parametrize("R", dr.SIZES)
def test_stage2_equals_the_loops_on_the_devices_own_bitmaps(R):
    top, xyz, _m = sized_call(R)
    out = host(metrics.dssp(dev(xyz), top))
    hb = dr.unpack_bits(words(out["acc"]), R)
    ss, bridge, counts = dr.assign_batch(hb, out["geom"], out["finite"])
    assert np.array_equal(out["ss"], ss) and np.array_equal(out["bridge"], bridge) and np.array_equal(out["counts"], counts)
    assert out["ss"].dtype == np.uint8 and out["bridge"].dtype == np.int32 and out["counts"].dtype == np.int32
    assert (out["counts"].sum(1) == R).all()


@pytest.mark.gpu
@pytest.mark.parametrize("R", (130, 200))
def test_stage2_on_hand_written_and_random_bitmaps(R):
    """Ladders whose partners straddle bits 63 / 64 and 127 / 128 (the shifts must carry), a bridge with |i - j| = 2, a
    bridge across a broken link, G next to H, overlapping I, left-over T and S - and random maps, all in one call."""
    maps = [dr.handmade(R)[:3]] + [dr.random_maps(R, seed) for seed in (1, 2, 3, 4, 5)]
    hb, link, bend = (np.stack([m[k] for m in maps]) for k in range(3))
    out, geom, fin = assign_on_device(hb, link, bend)
    ss, bridge, counts = dr.assign_batch(hb, geom, fin)
    assert np.array_equal(out["ss"], ss) and np.array_equal(out["bridge"], bridge) and np.array_equal(out["counts"], counts)
    checks = dr.handmade(R)[3]
    got = dr.labels(out["ss"][0])
    assert {r: got[r] for r in checks} == checks
    # the link bit of the last residue is ignored, and a structure marked not finite gets the defined result
    link2 = link.copy()
    link2[:, R - 1] = True
    out2, _g, _f = assign_on_device(hb, link2, bend, finite=[1, 0, 1, 1, 0, 1])
    keep = np.array([0, 2, 3, 5])
    assert np.array_equal(out2["ss"][keep], ss[keep]) and np.array_equal(out2["bridge"][keep], bridge[keep])
    assert (out2["ss"][[1, 4]] == dr.UNDEFINED).all() and (out2["bridge"][[1, 4]] == -1).all() and (out2["counts"][[1, 4]] == -1).all()


KEYS = ("acc", "don", "geom", "kappa", "e_best", "partner", "finite", "ss", "bridge", "counts")


def same(a, b):
    return all(np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)) for k in KEYS)


@pytest.mark.gpu
def test_a_mixed_call_equals_single_calls_and_repeats_bit_for_bit():
    top, xyz, _m = sized_call(65)
    assert xyz.shape[0] == 5
    x = dev(xyz)
    first, second = host(metrics.dssp(x, top)), host(metrics.dssp(x, top))
    assert same(first, second)
    for s in range(5):
        one = host(metrics.dssp(x[s:s + 1], top))
        assert all(np.array_equal(one[k][0].view(np.uint8), first[k][s].view(np.uint8)) for k in KEYS), s


@pytest.mark.gpu
@pytest.mark.parametrize("bad", ("nan", "+inf", "-inf"))
def test_non_finite_input_has_a_defined_result(bad):
    value = {"nan": float("nan"), "+inf": float("inf"), "-inf": float("-inf")}[bad]
    top, xyz, _m = sized_call(65)
    clean = host(metrics.dssp(dev(xyz), top))
    hit = xyz.copy()
    hit[2, top.atom(30, "O"), 1] = value                       # a backbone atom of structure 2
    out = host(metrics.dssp(dev(hit), top))
    assert out["finite"].tolist() == [True, True, False, True, True]
    assert not out["acc"][2].any() and not out["don"][2].any() and not out["geom"][2].any()
    assert np.isnan(out["kappa"][2]).all() and np.isnan(out["e_best"][2]).all() and (out["partner"][2] == -1).all()
    assert (out["ss"][2] == dr.UNDEFINED).all() and (out["bridge"][2] == -1).all() and (out["counts"][2] == -1).all()
    others = [0, 1, 3, 4]
    assert all(np.array_equal(out[k][others].view(np.uint8), clean[k][others].view(np.uint8)) for k in KEYS)
    res = metrics.dssp(dev(hit), top)
    assert res["ss_string"][2] == "?" * 65 and res["ss_string"][0] == dr.labels(clean["ss"][0])
    prop = metrics.ss_propensity(res["ss"]).cpu().numpy()
    want = np.stack([(clean["ss"][others] == c).sum(0) / 4.0 for c in range(8)], 1)
    assert prop.dtype == np.float64 and prop.shape == (65, 8) and np.array_equal(prop, want)
    # a side-chain atom is never read: the same value there changes nothing
    side = xyz.copy()
    side[2, top.atom(30, "CB"), 1] = value
    assert same(host(metrics.dssp(dev(side), top)), clean)


# ---------------------------------------------------------------------------------------------------------------- CLI
def _cli(cwd, *extra):
    cmd = [sys.executable, os.path.join(ROOT, "test.py"), "--synthetic", "--synthetic_weights", "--num_sampling_steps", "4",
           "--num_ensemble", "2"] + list(extra)
    res = subprocess.run(cmd, env=dict(os.environ, PYTHONPATH=ROOT), cwd=str(cwd), capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-1500:] + res.stderr[-3000:]
    files = {f: os.path.join(dp, f) for dp, _d, fs in os.walk(os.path.join(str(cwd), "logs")) for f in fs}
    return files, res.stdout


@pytest.mark.gpu
def test_cli_dssp_end_to_end(tmp_path):
    from codlad_amd import synth
    from codlad_amd.utils.cg_input import template_topology
    (tmp_path / "on").mkdir()
    (tmp_path / "off").mkdir()
    on, stdout = _cli(tmp_path / "on", "--dssp")
    off, stdout_off = _cli(tmp_path / "off")
    new = {f for f in on if f.endswith(("_dssp.npy", "_dssp_propensity.npy"))}
    assert set(on) - set(off) == new and set(off) <= set(on) and len(new) == 2 * 4        # the four PED-shaped proteins
    for f in off:
        assert open(on[f], "rb").read() == open(off[f], "rb").read(), f                   # nothing else changes
    assert "secondary structure" in stdout and "helix " in stdout and "strand " in stdout and "coil " in stdout
    assert "secondary structure" not in stdout_off
    for i, L in enumerate((46, 87, 92, 129)):
        name = f"synthetic_L{L}"
        xyz = np.load(on[f"{name}_xyz_recon.npy"])
        E, B, n_atoms = xyz.shape[:3]
        prot = synth.make_protein(L, 1000 + i, n_frames=1)
        top = template_topology([synth.IDX2THR[int(z)] for z in prot["z_full"]][1:-1])
        assert top.n_atoms == n_atoms and top.n_residues == L
        ss, prop = np.load(on[f"{name}_dssp.npy"]), np.load(on[f"{name}_dssp_propensity.npy"])
        assert ss.shape == (E * B, L) and ss.dtype == np.uint8 and prop.shape == (L, 8) and prop.dtype == np.float64
        want = metrics.dssp(dev(xyz.reshape(-1, n_atoms, 3)), top)
        assert np.array_equal(ss, want["ss"].cpu().numpy())
        assert np.array_equal(prop, metrics.ss_propensity(want["ss"]).cpu().numpy(), equal_nan=True)
        assert np.allclose(prop.sum(1), 1.0)
