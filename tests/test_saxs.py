"""SAXS profiles on the device (codlad_amd/csrc/saxs_kernels.hip through codlad_amd.metrics) against the float64 Debye sum
of tests/saxs_ref.py.

The bound: |I_dev - I_ref| <= 4 * dev32(case) * A[s, k] for every case, structure and q, with A = sum f_i^2 + 2 sum |f_i f_j
sinc| and dev32(case) = max |I_r32 - I_ref| / A, I_r32 the float32 restatement of the header's sequence - reference and
restatement only, nothing of the device's output.  The restatement is operation for operation the kernel's, so the device
is expected at a ratio |I_dev - I_ref| / (dev32 A) near 1; every test prints what it observed."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from codlad_amd import metrics
from tests import saxs_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
NAN_KINDS = {"nan": float("nan"), "+inf": float("inf"), "-inf": float("-inf")}
MARGIN = 4.0


def dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)                    # a copy: the cached inputs are read-only


def run(c, x=None):
    return metrics.saxs_profile_lists(dev(c["x"] if x is None else x), c["types"], c["ff"], c["q"])


@pytest.mark.gpu
@pytest.mark.parametrize("key", sr.case_keys(), ids=sr.case_id)
def test_profile_against_the_float64_reference(key):
    c = sr.case(key)
    out = run(c)
    I = out["I"].cpu().numpy()
    assert I.dtype == np.float64 and I.shape == c["I"].shape and out["finite"].tolist() == [True] * sr.N_STRUCT
    err = np.abs(I - c["I"])
    scale = c["dev32"] * c["A"]
    ratio = float((err[scale > 0] / scale[scale > 0]).max()) if (scale > 0).any() else 0.0
    same = int((I == c["I32"]).sum())
    print(f"{sr.case_id(key)}: dev32 {c['dev32']:.3e}, max |I_dev - I_ref| / (dev32 A) {ratio:.3f}, elements with the "
          f"restatement's bits {same} of {I.size}")
    assert (err <= MARGIN * scale).all(), (key, np.argwhere(err > MARGIN * scale)[:5].tolist())


@pytest.mark.gpu
@pytest.mark.parametrize("key", [(300, 51, 5, 0.0, "plain"), (129, sr.CHUNK + 1, 5, 500.0, "q0"), (65, 51, 5, 0.0, "coincident"),
                                 (2, 1, 1, 500.0, "plain")], ids=sr.case_id)
def test_results_are_bit_identical_and_independent_of_the_batch(key):
    c = sr.case(key)
    a, b = run(c), run(c)
    assert torch.equal(a["I"], b["I"]) and torch.equal(a["finite"], b["finite"])
    for s in range(sr.N_STRUCT):
        alone = run(c, c["x"][s:s + 1])
        assert torch.equal(alone["I"][0], a["I"][s]), s
        moved = run(c, np.stack([c["x"][(s + 1) % 3], c["x"][(s + 2) % 3], c["x"][s]]))
        assert torch.equal(moved["I"][2], a["I"][s]), s


@pytest.mark.gpu
def test_hand_made_cases():
    q = np.linspace(0.05, 0.5, 8).astype(np.float32)
    ff = np.stack([np.float32(6.0) * np.exp(-q * q), np.float32(-1.5) * np.exp(-2 * q * q)]).astype(np.float32)
    f = ff.astype(np.float64)

    def lists(x, types, table=ff, qq=q):
        out = metrics.saxs_profile_lists(dev(np.array(x, dtype=np.float32)[None]), types, table, qq)
        assert out["finite"].tolist() == [True]
        return out["I"][0].cpu().numpy()

    def bound(x, types, table, qq):                                 # the bound of the module docstring for a hand-made case
        x = np.array(x, dtype=np.float32)[None]
        I, A = sr.debye64(x, types, table, qq)
        dev32 = (np.abs(sr.debye32(x[0], types, table, qq) - I[0]) / A[0]).max()
        return I[0], MARGIN * dev32 * A[0]

    # one atom: I = f^2, exactly (the product of two float32 numbers in float64)
    for t in (0, 1):
        assert np.array_equal(lists([[3.0, -2.0, 1.0]], [t]), f[t] * f[t])
    # two atoms 3 A apart at Q = 8 against the analytic curve
    x = [[1.0, 2.0, 3.0], [1.0, 5.0, 3.0]]
    got = lists(x, [0, 1])
    ref, tol = bound(x, [0, 1], ff, q)
    want = sr.two_atoms(f[0], f[1], 3.0, q)
    print(f"two atoms at 3 A: max |I_dev - analytic| / bound {(np.abs(got - want) / tol).max():.3f}")
    assert (np.abs(ref - want) <= 1e-13 * np.abs(want)).all() and (np.abs(got - want) <= tol + 1e-13 * np.abs(want)).all()
    # coincident atoms: sinc = 1 exactly, I = (f_0 + f_1)^2 up to the float64 roundings of three terms
    got = lists([[7.0, 7.0, 7.0], [7.0, 7.0, 7.0]], [0, 1])
    want = f[0] * f[0] + f[1] * f[1] + 2.0 * f[0] * f[1]
    assert (np.abs(got - want) <= 4 * 2.0 ** -53 * (f[0] * f[0] + f[1] * f[1] + 2 * np.abs(f[0] * f[1]))).all()
    # q = 0: I(0) = (sum f)^2 for any geometry, exactly here (sinc = 1 from the series, small integers)
    q0 = np.array([0.0, 0.3], dtype=np.float32)
    tab = np.array([[6.0, 5.0], [-1.0, -0.5], [8.0, 7.0]], dtype=np.float32)
    x = [[0.0, 0.0, 0.0], [1.5, 0.0, 0.0], [0.0, 40.0, 9.0], [3.0, 3.0, 3.0]]
    got = lists(x, [0, 1, 2, 2], tab, q0)
    ref, tol = bound(x, [0, 1, 2, 2], tab, q0)
    assert got[0] == (6.0 - 1.0 + 8.0 + 8.0) ** 2 and abs(got[1] - ref[1]) <= tol[1]


@pytest.mark.gpu
@pytest.mark.parametrize("n", [4, 129])
def test_non_finite_input_gets_the_defined_result_and_leaves_the_other_structures_alone(n):
    c = sr.case((129, sr.CHUNK + 1, 5, 500.0, "q0"))
    x = c["x"][:, :n]
    types = c["types"][:n]
    clean = metrics.saxs_profile_lists(dev(x), types, c["ff"], c["q"])
    assert clean["finite"].tolist() == [True] * 3 and not bool(torch.isnan(clean["I"]).any())
    for label, value in NAN_KINDS.items():
        for atom, comps, victim in ((0, (1,), 1), (n // 2, (0, 1, 2), 1), (n - 1, (2,), 1), (n // 2, (1,), 0), (n - 1, (0,), 2)):
            bad = x.copy()
            bad[victim, atom, list(comps)] = value
            out = metrics.saxs_profile_lists(dev(bad), types, c["ff"], c["q"])
            what = (label, atom, comps, victim)
            assert out["finite"].tolist() == [s != victim for s in range(3)], what
            assert bool(torch.isnan(out["I"][victim]).all()), what
            for s in range(3):
                if s != victim:
                    assert torch.equal(out["I"][s], clean["I"][s]), (what, s)


@pytest.mark.gpu
def test_buffers_are_written_before_they_are_read_and_only_inside():
    """tests/memcheck.py around the two functions: the results have the same bits under the three fills of every buffer
    the package allocates (the partials among them), every element of I, mean and finite is written, no zone byte changes."""
    from codlad_amd.utils.cg_input import template_topology
    from tests.test_buffer_discipline import hold
    c = sr.case((129, sr.CHUNK + 1, 5, 500.0, "q0"))
    top = template_topology(["ALA", "TRP", "GLY", "SEP", "LYS"])
    rng = np.random.default_rng(5)
    xt = (rng.uniform(-8, 8, (3, top.n_atoms, 3))).astype(np.float32)
    xt[1, 3, 0] = np.nan                                             # a row of NaN is a written row too

    def case(g):
        out = metrics.saxs_profile_lists(g(torch.from_numpy(c["x"]), "xyz"), c["types"], c["ff"], c["q"])
        prof = metrics.saxs_profile(g(torch.from_numpy(xt), "xyz_top"), top)
        top.__dict__.pop("_saxs_tables")                             # the next fill builds its own tables
        return dict(I=out["I"], finite=out["finite"], prof_I=prof["I"], prof_mean=prof["mean"], prof_finite=prof["finite"],
                    prof_q=prof["q"]), []
    hold("saxs", case)


@pytest.mark.gpu
def test_saxs_profile_on_a_topology_and_the_fit():
    from codlad_amd.utils.cg_input import template_topology
    names = ["MET", "ALA", "PRO", "TRP", "GLY", "SEP", "LYS", "HIS", "TPO", "ARG", "CYS", "ASP", "TYR", "GLN"]
    top = template_topology(names)
    rng = np.random.default_rng(11)
    x = (rng.uniform(-12, 12, (4, top.n_atoms, 3))).astype(np.float32)
    x[2, 5, 1] = np.inf
    out = metrics.saxs_profile(dev(x), top)
    q = out["q"].cpu().numpy()
    assert q.dtype == np.float32 and np.array_equal(q, np.linspace(0.0, 0.5, 51).astype(np.float32))
    assert out["finite"].tolist() == [True, True, False, True] and int(out["n_finite"]) == 3
    groups, types = metrics.saxs_groups(top)
    table = metrics.form_factors(np.linspace(0.0, 0.5, 51), groups).astype(np.float32)
    good = [0, 1, 3]
    ref, A = sr.debye64(x[good], types, table, q)
    dev32 = max((np.abs(sr.debye32(x[s], types, table, q) - ref[k]) / A[k]).max() for k, s in enumerate(good))
    I = out["I"].cpu().numpy()
    ratio = (np.abs(I[good] - ref) / (dev32 * A)).max()
    print(f"saxs_profile, {top.n_atoms} atoms, {len(groups)} groups: dev32 {dev32:.3e}, max ratio {ratio:.3f}")
    assert (np.abs(I[good] - ref) <= MARGIN * dev32 * A).all() and np.isnan(I[2]).all()
    assert abs(I[0, 0] - table[types, 0].astype(np.float64).sum() ** 2) <= MARGIN * dev32 * A[0, 0]
    mean = np.zeros(51)
    for s in good:                                                   # float64, index order
        mean = mean + I[s]
    assert np.array_equal(out["mean"].cpu().numpy(), mean / 3.0)
    lists = metrics.saxs_profile_lists(dev(x), types, table, q)
    assert torch.equal(lists["I"][good], out["I"][good])
    # cached once per (q, solvent density, device); another density is another table and another curve
    metrics.saxs_profile(dev(x), top)
    assert len(top._saxs_tables) == 1
    vac = metrics.saxs_profile(dev(x), top, solvent_density=0.0)
    assert len(top._saxs_tables) == 2 and bool((vac["I"][0, 0] > out["I"][0, 0]))
    none = metrics.saxs_profile(dev(x[2:3]), top)
    assert bool(torch.isnan(none["mean"]).all()) and int(none["n_finite"]) == 0
    with pytest.raises(ValueError, match="atoms"):
        metrics.saxs_profile(dev(x[:, :-1]), top)
    # the fit against numpy
    calc = out["mean"]
    sigma = 0.02 * np.abs(mean / 3.0) + 1e-3
    exp = 2.5 * (mean / 3.0) + sigma * rng.standard_normal(51)
    fit = metrics.saxs_fit(calc, q, exp, sigma)
    cn = mean / 3.0
    scale = (exp * cn / sigma ** 2).sum() / (cn * cn / sigma ** 2).sum()
    chi2 = (((scale * cn - exp) / sigma) ** 2).sum() / 50
    assert fit["scale"].dtype == torch.float64 and fit["scale"].is_cuda
    assert abs(float(fit["scale"]) - scale) <= 1e-12 * scale and abs(float(fit["chi2"]) - chi2) <= 1e-9 * chi2
    exact = metrics.saxs_fit(calc, q, 3.0 * cn, sigma)
    assert abs(float(exact["scale"]) - 3.0) <= 1e-12 and float(exact["chi2"]) <= 1e-20
    with pytest.raises(ValueError, match="same length"):
        metrics.saxs_fit(calc, q[:-1], exp, sigma)
    with pytest.raises(ValueError, match="positive"):
        metrics.saxs_fit(calc, q, exp, 0 * sigma)


# ---------------------------------------------------------------------------------------------------------------- CLI
def _cli(cwd, *extra):
    cmd = [sys.executable, os.path.join(ROOT, "test.py"), "--synthetic", "--synthetic_weights", "--num_sampling_steps", "4",
           "--num_ensemble", "2"] + list(extra)
    res = subprocess.run(cmd, env=dict(os.environ, PYTHONPATH=ROOT), cwd=str(cwd), capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-1500:] + res.stderr[-3000:]
    files = {f: os.path.join(dp, f) for dp, _d, fs in os.walk(os.path.join(str(cwd), "logs")) for f in fs}
    return files, res.stdout


@pytest.mark.gpu
def test_cli_saxs_end_to_end(tmp_path):
    from codlad_amd import synth
    from codlad_amd.utils.cg_input import template_topology
    for d in ("on", "off", "data"):
        (tmp_path / d).mkdir()
    on, stdout = _cli(tmp_path / "on", "--saxs", "16")
    off, stdout_off = _cli(tmp_path / "off")
    new = {f for f in on if f.endswith(("_saxs.npy", "_saxs_q.npy"))}
    assert set(on) - set(off) == new and set(off) <= set(on) and len(new) == 2 * 4           # the four PED-shaped proteins
    for f in off:
        assert open(on[f], "rb").read() == open(off[f], "rb").read(), f                       # nothing else changes
    assert "SAXS profile" in stdout and "saxs_I0" in stdout and "SAXS" not in stdout_off and "saxs" not in stdout_off
    i, L = 0, 46
    name = f"synthetic_L{L}"
    xyz = np.load(on[f"{name}_xyz_recon.npy"])
    n_atoms = xyz.shape[2]
    prot = synth.make_protein(L, 1000 + i, n_frames=1)
    top = template_topology([synth.IDX2THR[int(z)] for z in prot["z_full"]][1:-1])
    assert top.n_atoms == n_atoms
    I, q = np.load(on[f"{name}_saxs.npy"]), np.load(on[f"{name}_saxs_q.npy"])
    assert I.dtype == np.float64 and I.shape == (xyz.shape[0] * xyz.shape[1], 16)
    assert np.array_equal(q, np.linspace(0.0, 0.5, 16).astype(np.float32))
    flat = xyz.reshape(-1, n_atoms, 3)
    want = metrics.saxs_profile(dev(flat), top, q=np.linspace(0.0, 0.5, 16))
    assert np.array_equal(I, want["I"].cpu().numpy(), equal_nan=True)
    # --saxs_data on a file written from the reference curve: scale 1 and chi^2 0 within the bound
    groups, types = metrics.saxs_groups(top)
    table = metrics.form_factors(q.astype(np.float64), groups).astype(np.float32)
    ref, A = sr.debye64(flat, types, table, q)
    dev32 = (np.abs(sr.debye32(flat[0], types, table, q) - ref[0]) / A[0]).max()
    curve, sigma = ref.mean(0), 0.01 * np.abs(ref.mean(0))
    path = tmp_path / "curve.dat"
    path.write_text("# q I sigma, the float64 reference\n" + "".join(
        f"{float(a)!r} {float(b)!r} {float(s)!r}\n" for a, b, s in zip(q, curve, sigma)))
    _files, out = _cli(tmp_path / "data", "--saxs", "--saxs_data", str(path))
    block = next(b for b in out.split("vvvvvvvvv SAXS profile")[1:] if f"data_name {name}\n" in b)
    scale = float(block.split("saxs_scale ")[1].split()[0])
    chi2 = float(block.split("saxs_chi2 ")[1].split()[0])
    # every point of the device's mean lies within rel of the curve, relative to it; so does the scale, and a residual
    # (c - 1) calc + (calc - exp) within 2 rel |curve| = 200 rel sigma
    rel = MARGIN * dev32 * (A.mean(0) / np.abs(curve)).max()
    print(f"--saxs_data: scale {scale!r}, chi2 {chi2!r}, relative bound {rel:.3e}")
    assert abs(scale - 1.0) <= rel and chi2 <= (200.0 * rel) ** 2 * 16 / 15
