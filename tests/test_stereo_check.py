"""Stereochemistry check on the device (codlad_stereo_check, csrc/stereo_kernels.hip; metrics.stereo_check).

Inputs are chains built by NeRF from planted torsions, inversions and peptide-bond classes (tests/stereo_ref.py), rounded
to fp32, as built and translated by 1000 A; the float64 reference runs on those fp32 coordinates.  Margins asserted on the
CPU for every case: every |omega| at least 0.5 degrees from 30 and 150, every |v| >= 0.1 A^3, every bond angle inside a
torsion within [60, 150] degrees - so no fp32 decision can differ and flags and counts must be EXACTLY the reference's.

Values: |device - float64| <= 4 x ref_dev (+ the atan2f term for torsions), ref_dev = the largest deviation, over all
cases, of the SAME formula evaluated in numpy float32 (one rounding per operation, the kernel's order) from float64.
The torsion's additive term is ATAN2F_ULPS + 1 ulps of 180 degrees (2^-16 degrees each): atan2f of the device library
is ASSUMED accurate to 6 ulp, the OpenCL full-profile limit that library is written to - the ROCm accuracy table was
not available when this was written, so the figure is an assumption, not a citation; the radian -> degree product adds
half an ulp of rounding and half an ulp for the rounded constant.  Sizes: one below / at / one above a wave (64) and a
workgroup (256), three workgroups (600), for 1 and 3 structures, and a two-chain topology.

Figures (printed by every run): ref_dev 2.83e-5 degrees and 5.72e-7 A^3, bounds 2.20e-4 degrees and 2.29e-6 A^3; the device's
largest errors on an MI355X: 2.71e-5 degrees and 5.72e-7 A^3 (the volumes are the float32 evaluation's, bit for bit)."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from codlad_amd import _lib, metrics
from tests import stereo_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ATAN2F_ULPS = 6                    # assumed accuracy of the device library's atan2f (see the module docstring)
ULP_180 = 2.0 ** -16               # spacing of fp32 in [128, 256)
TWO_CHAINS = "two_chains"
KEYS = sr.SIZES + (TWO_CHAINS,)


@functools.lru_cache(maxsize=None)
def case(key):
    """Three structures of one topology, as built and translated, with their references -> dict: top, pl (the planted
    inputs per structure), x [2][3, n_atoms, 3] fp32, ref [2] = (values float64, flags, counts), ref32 [2] = values of the
    float32 evaluation."""
    n, breaks = (90, (41,)) if key == TWO_CHAINS else (key, ())
    pls = [sr.planted(n, 7000 + 10 * n + s, breaks, first=n % 22) for s in range(3)]
    built = [sr.build_chain(**pl) for pl in pls]
    top = built[0][0]
    xyz = np.stack([b[1] for b in built])
    x = [xyz.astype(np.float32), (xyz + sr.SHIFT).astype(np.float32)]
    return dict(top=top, pl=pls, x=x, ref=[sr.reference(v, top) for v in x],
                ref32=[sr.reference(v, top, np.float32)[0].astype(np.float64) for v in x])


@functools.lru_cache(maxsize=None)
def bounds():
    """(torsion bound in degrees, volume bound in A^3, ref_dev of each) over ALL cases."""
    dev_t = dev_v = 0.0
    for key in KEYS:
        c = case(key)
        for (v64, _f, _c), v32 in zip(c["ref"], c["ref32"]):
            dev_t = max(dev_t, float(np.nanmax(sr.angle_diff(v32[..., :7], v64[..., :7]), initial=0.0)))
            dev_v = max(dev_v, float(np.nanmax(np.abs(v32[..., 7:] - v64[..., 7:]), initial=0.0)))
    tol_t, tol_v = 4 * dev_t + (ATAN2F_ULPS + 1) * ULP_180, 4 * dev_v
    print(f"ref_dev torsion {dev_t:.3e} deg volume {dev_v:.3e} A^3; bounds {tol_t:.3e} deg {tol_v:.3e} A^3")
    return tol_t, tol_v, dev_t, dev_v


def run(x, top):
    out = metrics.stereo_check(torch.from_numpy(np.ascontiguousarray(x)).cuda(), top)
    return out, out["values"].cpu().numpy(), out["flags"].cpu().numpy(), out["counts"].cpu().numpy()


def compare(values, flags, counts, ref, what):
    """Device output of some structures against their reference: -> (largest torsion error, largest volume error)."""
    v64, f64, c64 = ref
    tol_t, tol_v, _dt, _dv = bounds()
    assert values.dtype == np.float32 and flags.dtype == np.uint8 and counts.dtype == np.int32
    assert values.shape == v64.shape and flags.shape == f64.shape and counts.shape == c64.shape
    assert np.array_equal(np.isnan(values), np.isnan(v64)), what                        # absent / undefined: the same places
    err_t = float(np.nanmax(sr.angle_diff(values[..., :7], v64[..., :7]), initial=0.0))
    err_v = float(np.nanmax(np.abs(values[..., 7:].astype(np.float64) - v64[..., 7:]), initial=0.0))
    print(f"{what}: torsion error {err_t:.3e} (bound {tol_t:.3e}) volume error {err_v:.3e} (bound {tol_v:.3e}) counts {counts.tolist()}")
    assert np.array_equal(flags, f64), (what, np.argwhere(flags != f64)[:5])
    assert np.array_equal(counts, c64), (what, counts, c64)
    with np.errstate(invalid="ignore"):
        assert (values[..., :7][np.isfinite(values[..., :7])] > -180.0).all() and np.nanmax(values[..., :7], initial=0.0) <= 180.0
    assert err_t <= tol_t and err_v <= tol_v, (what, err_t, tol_t, err_v, tol_v)
    return err_t, err_v


# ------------------------------------------------------------------------------------------------------------------ CPU
def test_inputs_keep_their_margins_and_the_reference_returns_what_was_planted():
    seen = np.zeros(6, dtype=np.int64)
    w_margin, v_min = np.inf, np.inf
    for key in KEYS:
        c = case(key)
        top = c["top"]
        for x, (v64, flags, counts) in zip(c["x"], c["ref"]):
            w = np.abs(v64[..., 2])
            w_margin = min(w_margin, float(np.nanmin(np.minimum(np.abs(w - 30.0), np.abs(w - 150.0)), initial=np.inf)))
            v_min = min(v_min, float(np.nanmin(np.abs(v64[..., 7:]), initial=np.inf)))
            ang = sr.bond_angles(x, top)
            assert np.nanmin(ang, initial=90.0) >= 60.0 and np.nanmax(ang, initial=90.0) <= 150.0, key
            assert counts[:, 5].sum() == 0
            seen += counts.sum(0)
            for s in range(3):                                 # the planted angles and inversions ARE what the reference finds
                tors, want = sr.planted_truth(top, c["pl"][s])
                assert np.array_equal(np.isnan(v64[s, :, :7]), np.isnan(tors)) and flags[s].tolist() == want.tolist(), (key, s)
                # rounding a coordinate of magnitude M to fp32 moves it by <= 2^-24 M; four atoms, three axes and lever arms of
                # about 1 A: an angle moves by a few times that in radians (8 x is generous, and still 1000 x below the margins)
                moved = np.rad2deg(8 * 2.0 ** -24 * float(np.abs(x[s]).max()))
                assert np.nanmax(sr.angle_diff(v64[s, :, :7], tors), initial=0.0) < moved, (key, s)
    print(f"smallest |omega| margin {w_margin:.3f} deg, smallest |v| {v_min:.3f} A^3, totals {seen.tolist()}")
    assert w_margin >= 0.5 and v_min >= 0.1
    assert (seen[:5] > 0).all()                                # every decision occurs, cis on PRO and on non-PRO
    tol_t, tol_v, dev_t, dev_v = bounds()
    assert 0 < dev_t < 1e-4 and 0 < dev_v < 2e-6               # the fp32 formula is well conditioned on these inputs


# ------------------------------------------------------------------------------------------------------------------ GPU
@pytest.mark.gpu
@pytest.mark.parametrize("shifted", [0, 1], ids=["built", "shifted"])
@pytest.mark.parametrize("n_struct", [1, 3])
@pytest.mark.parametrize("key", KEYS)
def test_kernel_against_float64_reference(key, n_struct, shifted):
    c = case(key)
    out, values, flags, counts = run(c["x"][shifted][:n_struct], c["top"])
    compare(values, flags, counts, tuple(a[:n_struct] for a in c["ref"][shifted]), f"{key} S={n_struct} shifted={shifted}")
    R = c["top"].n_residues
    assert tuple(out["chi"].shape) == (n_struct, R, 4) and tuple(out["phi"].shape) == (n_struct, R)
    for k, name in enumerate(("phi", "psi", "omega")):
        assert out[name].data_ptr() == out["values"][..., k].data_ptr()
    assert torch.equal(out["v_ca"].isnan(), out["values"][..., 7].isnan())
    for k, name in enumerate(metrics.STEREO_COUNTS):
        assert torch.equal(out[name], out["counts"][:, k])
    bad = counts[:, [0, 1, 3, 4, 5]].sum(1)
    assert out["stereo_ok"].dtype == torch.bool and out["stereo_ok"].cpu().tolist() == (bad == 0).tolist()


@pytest.mark.gpu
def test_stereo_ok_ignores_cis_proline_only():
    n = 4
    z = np.zeros(n)
    rows = []
    for omega_pro, omega_ala in ((180.0, 180.0), (5.0, 180.0), (180.0, -10.0), (90.0, 180.0)):
        top, xyz = sr.build_chain(["SER", "PRO", "ALA", "THR"], z - 70, z + 140, np.array([180.0, omega_pro, omega_ala, 180.0]),
                                  np.full((n, 4), 60.0))
        rows.append(xyz)
    top_d, xyz_d = sr.build_chain(["SER", "PRO", "ALA", "THR"], z - 70, z + 140, z + 180, np.full((n, 4), 60.0), d_ca=[0, 0, 1, 0])
    top_s, xyz_s = sr.build_chain(["SER", "PRO", "ALA", "THR"], z - 70, z + 140, z + 180, np.full((n, 4), 60.0), d_side=[0, 0, 0, 1])
    out, _v, flags, counts = run(np.stack(rows + [xyz_d, xyz_s]).astype(np.float32), top)
    assert counts.tolist() == [[0, 0, 0, 0, 0, 0], [0, 0, 1, 0, 0, 0], [0, 0, 0, 1, 0, 0], [0, 0, 0, 0, 1, 0],
                               [1, 0, 0, 0, 0, 0], [0, 1, 0, 0, 0, 0]]
    assert out["stereo_ok"].cpu().tolist() == [True, True, False, False, False, False]
    assert flags[1].tolist() == [0, sr.CIS, 0, 0] and flags[3].tolist() == [0, sr.TWISTED, 0, 0]
    assert flags[4].tolist() == [0, 0, sr.INVERTED_CA, 0] and flags[5].tolist() == [0, 0, 0, sr.INVERTED_SIDE]


@pytest.mark.gpu
def test_results_are_bit_identical_and_independent_of_the_batch():
    for key, shifted in ((257, 0), (TWO_CHAINS, 1)):
        c = case(key)
        x = torch.from_numpy(c["x"][shifted]).cuda()
        a, b = metrics.stereo_check(x, c["top"]), metrics.stereo_check(x, c["top"])
        bits = lambda t: t.view(torch.int32) if t.dtype == torch.float32 else t                           # noqa: E731
        for k in ("values", "flags", "counts"):
            assert torch.equal(bits(a[k]), bits(b[k])), k
        for s in range(3):
            one = metrics.stereo_check(x[s:s + 1], c["top"])
            for k in ("values", "flags", "counts"):
                assert torch.equal(bits(one[k][0]), bits(a[k][s])), (k, s)
    top = case(257)["top"]
    assert set(top._stereo_tables) == {"host", "cuda:0"}                       # built once, kept on the topology
    with pytest.raises(ValueError, match="atoms"):
        metrics.stereo_check(torch.zeros(1, top.n_atoms - 1, 3, device="cuda"), top)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["nan", "coincident"])
def test_degenerate_input_marks_exactly_its_readers(kind):
    """Structure 1 of three gets one NaN coordinate (CA of residue 31, a HIS), or N of residue 31 moved onto its CA: `undefined`
    on the residues whose quantities read the atom (NaN) / lose their angle (coincident), everything else bit for bit as
    without the damage."""
    c = case(65)
    top, x = c["top"], c["x"][0].copy()
    assert top.res_names[31] == "HIS"                          # a residue with phi, psi, omega, chi1, chi2 and v_ca
    ca, n_atom = top.atom(31, "CA"), top.atom(31, "N")
    if kind == "nan":
        x[1, ca, 1] = np.nan
        touched = sr.readers(top, ca)
        assert touched == [31, 32]                             # residue 31 itself and omega_in of 32
    else:
        x[1, n_atom] = x[1, ca]
        touched = sorted(set(sr.readers(top, ca)) | set(sr.readers(top, n_atom)))
        assert touched == [30, 31, 32]
    ref = sr.reference(x, top)
    _o, base_v, base_f, base_c = run(c["x"][0], top)
    _o, values, flags, counts = run(x, top)
    assert np.array_equal(np.isnan(values), np.isnan(ref[0])) and np.array_equal(flags, ref[1]) and np.array_equal(counts, ref[2])
    undefined = np.nonzero(flags[1] & sr.UNDEFINED)[0].tolist()
    if kind == "nan":
        assert undefined == touched and counts[1, 5] == 2
        assert np.isnan(values[1, 31][np.isfinite(base_v[1, 31])]).all() and np.isnan(values[1, 32, 2])
        assert not (flags[1, 31] & (sr.INVERTED_CA | sr.CIS | sr.TWISTED))                # a NaN decides nothing
    else:
        # N = CA: phi (p1 = p2), psi and chi1 (p0 = p1) and omega_in (p2 = p3) of residue 31 have no angle; v_ca is exactly 0,
        # finite and not > 0; psi of 30 and omega_in of 32 still have an angle
        assert undefined == [31] and counts[1, 5] == 1
        assert np.isnan(values[1, 31, [0, 1, 2, 3]]).all() and values[1, 31, 7] == 0.0 and flags[1, 31] & sr.INVERTED_CA
        assert np.isfinite(values[1, 30, 1]) and np.isfinite(values[1, 32, 2]) and np.isfinite(values[1, 31, 4])
    rest = np.ones(flags.shape, dtype=bool)
    rest[1, touched] = False
    assert np.array_equal(values[rest].view(np.int32), base_v[rest].view(np.int32))      # bit for bit, NaN payloads included
    assert np.array_equal(flags[rest], base_f[rest]) and np.array_equal(counts[[0, 2]], base_c[[0, 2]])


@pytest.mark.gpu
def test_c_abi_treats_out_of_range_indices_as_absent():
    c = case(3)
    top = c["top"]
    sites, kind = (t.clone() for t in metrics.stereo_tables(top))
    sites[1, 0, 2] = top.n_atoms                               # phi of residue 1: one index just past the end
    sites[2, 7, 0] = 2 ** 31 - 1                               # v_ca of residue 2
    sites[1, 3, 1] = -7                                        # chi1 of residue 1: any negative index
    x = torch.from_numpy(c["x"][0][:1]).cuda()
    values = torch.zeros(1, 3, 9, device="cuda")
    flags = torch.zeros(1, 3, dtype=torch.uint8, device="cuda")
    counts = torch.full((1, 6), 99, dtype=torch.int32, device="cuda")
    p = _lib.ptr
    rc = _lib.lib().codlad_stereo_check(p(x), 1, top.n_atoms, p(sites.cuda()), p(kind.cuda()), 3, p(values), p(flags), p(counts),
                                        _lib.stream_ptr("cuda:0"))
    assert rc == 0
    base = metrics.stereo_check(x, top)
    gone = torch.zeros(1, 3, 9, dtype=torch.bool, device="cuda")
    gone[0, 1, 0] = gone[0, 2, 7] = gone[0, 1, 3] = True
    assert values[gone].isnan().all() and not base["values"][gone].isnan().any()
    assert torch.equal(values[~gone].view(torch.int32), base["values"][~gone].view(torch.int32))
    assert not (flags[0] & sr.UNDEFINED).any() and int(counts[0, 5]) == 0          # absent is not undefined


# ------------------------------------------------------------------------------------------------------------ end to end
def _cli(cwd, *extra):
    cmd = [sys.executable, os.path.join(ROOT, "test.py"), "--synthetic_weights", "--num_sampling_steps", "3", "--num_ensemble", "2",
           "--seed", "7"] + list(extra)
    res = subprocess.run(cmd, env=dict(os.environ, PYTHONPATH=ROOT), cwd=str(cwd), capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-1500:] + res.stderr[-3000:]
    files = {f: os.path.join(dp, f) for dp, _d, fs in os.walk(os.path.join(str(cwd), "logs")) for f in fs}
    return files, res.stdout


def _check_files(files, stem, top, E_B):
    xyz = np.load(files[f"{stem}_xyz_recon.npy"])
    counts, flags, tors = (np.load(files[f"{stem}_{k}.npy"]) for k in ("stereo", "stereo_flags", "torsions"))
    R = top.n_residues
    assert counts.dtype == np.int32 and counts.shape == (E_B, 6)
    assert flags.dtype == np.uint8 and flags.shape == (E_B, R)
    assert tors.dtype == np.float32 and tors.shape == (E_B, R, 9)
    by_hand = metrics.stereo_check(torch.from_numpy(xyz).cuda().reshape(E_B, -1, 3), top)
    assert np.array_equal(counts, by_hand["counts"].cpu().numpy()) and np.array_equal(flags, by_hand["flags"].cpu().numpy())
    assert np.array_equal(tors.view(np.int32), by_hand["values"].cpu().numpy().view(np.int32))
    assert np.isnan(tors[:, 0, 0]).all() and np.isnan(tors[:, -1, 1]).all()            # one chain: no phi at its start, no psi at its end
    return counts


@pytest.mark.gpu
def test_cli_stereo_check_end_to_end(tmp_path):
    from codlad_amd import synth
    from codlad_amd.utils.cg_input import template_topology
    from tests.test_dataset_builder import golden_frames, write_full_pdb
    # --synthetic: the three files per protein, equal to metrics.stereo_check on the saved coordinates
    os.makedirs(str(tmp_path / "syn"))
    files, stdout = _cli(tmp_path / "syn", "--synthetic", "--synthetic_frames", "2", "--data_type", "PED", "--vae_type", "N6",
                         "--stereo_check")
    for word in ("stereo_ok_ratio", "stereo_total_inverted_ca", "stereo_total_cis_nonpro", "stereo_worst_structure"):
        assert word in stdout, word
    assert "geometry_valid_ratio" not in stdout and not any(f.endswith("_geometry.npy") for f in files)    # its own flag
    for i, L in enumerate(synth.PED_LENGTHS):
        prot = synth.make_protein(L, 1000 + i, n_frames=2, phospho=False)
        names = [synth.IDX2THR[int(z)] for z in prot["z_full"]]
        _check_files(files, f"synthetic_L{L}", template_topology(names[1:-1]), 4)
    # without the flag no new file appears
    os.makedirs(str(tmp_path / "off"))
    files_off, stdout_off = _cli(tmp_path / "off", "--synthetic", "--synthetic_frames", "2", "--data_type", "PED", "--vae_type", "N6")
    assert set(files_off) == {f"synthetic_L{L}_xyz_recon.npy" for L in synth.PED_LENGTHS} and "stereo" not in stdout_off
    assert set(files) == set(files_off) | {f"synthetic_L{L}_{k}.npy" for L in synth.PED_LENGTHS
                                           for k in ("stereo", "stereo_flags", "torsions")}
    # --cg_pdb on a CA strip: beside the implied geometry check
    top, full, _og, _info, _g5 = golden_frames("N6_L46_B3")
    cg = tmp_path / "cg"
    os.makedirs(str(cg))
    write_full_pdb(str(cg / "full.pdb"), top, full)
    with open(str(cg / "full.pdb")) as f, open(str(cg / "ca.pdb"), "w") as g:
        g.writelines(l for l in f if l[:6] not in ("ATOM  ", "HETATM") or l[12:16].strip() == "CA")
    files, stdout = _cli(cg, "--cg_pdb", "ca.pdb", "--stereo_check")
    assert set(files) == {f"ca_{k}.npy" for k in ("xyz_recon", "geometry", "geometry_min", "stereo", "stereo_flags", "torsions")}
    assert "geometry_valid_ratio" in stdout and "stereo_ok_ratio" in stdout
    _check_files(files, "ca", template_topology(top.res_names).subset_residues(1, 47), 6)
