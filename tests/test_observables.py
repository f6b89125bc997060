"""Ensemble observables on the device (codlad_amd/csrc/observables_kernels.hip through codlad_amd.metrics): SASA, contact
counts and the radius of gyration against the float64 references of tests/observables_ref.py.

SASA decisions: per atom |exposed_dev - exposed_ref| <= the atom's UNDECIDED points (|m64| <= 4 ref_dev, ref_dev the float32
restatement's own deviation; tests/test_observables_host.py holds their number to 1 in 10^5) - exact almost everywhere.
Everything derived from the counts is held bit for bit to the header's statement.  Contact counts are exact (the inputs
keep every d^2 off the cut-off, asserted on the CPU).  Rg^2 is held to the bound tests/test_ensemble.py uses for G."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from codlad_amd import metrics
from tests import observables_ref as obr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
NAN_KINDS = {"nan": float("nan"), "+inf": float("inf"), "-inf": float("-inf")}


def dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)                    # a copy: the cached inputs are read-only


def run_case(key, n_struct=None):
    c = obr.sasa_case(*key)
    x = c["x"] if n_struct is None else c["x"][:n_struct]
    return metrics.sasa_lists(dev(x), c["vdw"], c["res_ptr"], probe=obr.PROBE, n_points=key[2])


def host(out):
    return {k: (None if v is None else v.cpu().numpy()) for k, v in out.items()}


def check_derived(out, c, n_points):
    """atom, residue and total from the device's own counts, as the header states them."""
    exposed, atom, residue, total = out["exposed"], out["atom"], out["residue"], out["total"]
    assert exposed.dtype == np.int32 and atom.dtype == np.float32 and residue.dtype == np.float32 and total.dtype == np.float64
    assert (exposed >= 0).all() and (exposed <= n_points).all() and out["finite"].all()
    assert np.array_equal(atom, exposed.astype(np.float32) * c["unit"][None])                      # one rounding
    rp = c["res_ptr"]
    for s in range(atom.shape[0]):
        for r in range(len(rp) - 1):
            acc = 0.0
            for v in atom[s, rp[r]:rp[r + 1]]:                                     # float64, index order
                acc += float(v)
            assert residue[s, r] == np.float32(acc), (s, r)
    n = atom.shape[1]
    for s in range(atom.shape[0]):
        exact = math.fsum(float(v) for v in atom[s])
        assert abs(total[s] - exact) <= n * 2.0 ** -53 * exact, (s, total[s], exact)


@pytest.mark.gpu
@pytest.mark.parametrize("key", obr.sasa_keys(), ids=lambda k: f"{k[0]}-{k[1]}-{k[2]}-{'shifted' if k[3] else 'built'}")
def test_sasa_against_the_float64_reference(key):
    c = obr.sasa_case(*key)
    want, undecided = obr.sasa_expected(key)
    for n_struct in sorted({1, c["x"].shape[0]}):
        out = host(run_case(key, n_struct))
        diff = np.abs(out["exposed"].astype(np.int64) - want[:n_struct])
        print(f"{key} S={n_struct}: ref_dev {obr.ref_dev():.3e}, undecided {int(undecided[:n_struct].sum())} of "
              f"{want[:n_struct].size * key[2]} points, atoms off the reference {int((diff > 0).sum())}, mean exposed "
              f"{out['exposed'].mean():.2f} of {key[2]}")
        assert (diff <= undecided[:n_struct]).all(), (key, np.argwhere(diff > undecided[:n_struct])[:5].tolist())
        check_derived(out, c, key[2])


@pytest.mark.gpu
def test_hand_made_cases():
    def run(x, vdw, n_points=96):
        return host(metrics.sasa_lists(dev(np.array(x, dtype=np.float32)[None]), vdw, probe=obr.PROBE, n_points=n_points))

    for P in (1, 64, 96, 960, 1024):
        out = run([[3.0, -2.0, 1.0]], [1.7], P)                                    # an isolated atom
        assert out["exposed"].tolist() == [[P]] and out["residue"] is None and out["finite"].tolist() == [True]
        area = 4.0 * math.pi * float(np.float32(3.1)) ** 2
        assert abs(out["total"][0] - area) <= 1e-6 * area and abs(out["atom"][0, 0] - area) <= 1e-6 * area
    out = run([[0.0, 0.0, 0.0], [100.0, 0.0, 0.0]], [1.7, 1.52])                   # far apart: both fully exposed
    assert out["exposed"].tolist() == [[96, 96]]
    # a small atom at the centre of one whose radius (with the probe) is twice its own: every point of the small one lies
    # at R inside 2 R; every point of the large one at 2 R outside R
    out = run([[1.0, 2.0, 3.0], [1.0, 2.0, 3.0]], [1.2, 2.6 * 2 - 1.4])
    assert out["exposed"].tolist() == [[0, 96]]
    # two overlapping equal spheres 3 A apart: the cap towards the partner is buried, h / (2 R) = (R - d / 2) / (2 R) of the area
    out = run([[0.0, 0.0, 0.0], [3.0, 0.0, 0.0]], [1.7, 1.7], 960)
    frac = (3.1 - 1.5) / (2 * 3.1)
    assert np.abs(out["exposed"][0] / 960 - (1 - frac)).max() < 1e-2                # the lattice's own error: a few points
    # the topology route: Bondi radii by element, residues by top.first_atom, tables cached on the topology
    from codlad_amd.utils.cg_input import template_topology
    top = template_topology(["ALA", "CYS", "GLY"])
    c = obr.sasa_case("chain", top.n_atoms, 96, False)
    x = dev(c["x"])
    a = metrics.sasa(x, top, n_points=96)
    b = metrics.sasa_lists(x, metrics.vdw_radii(top.element), top.first_atom, n_points=96)
    assert set(top._sasa_tables) == {(1.4, 96, "cuda:0")}
    assert all(torch.equal(a[k], b[k]) for k in a) and tuple(a["residue"].shape) == (c["x"].shape[0], 3)
    w = metrics.sasa(x, top, n_points=96, radii=[1.9] * top.n_atoms)
    assert bool((w["total"] > a["total"]).all())
    with pytest.raises(ValueError, match="atoms"):
        metrics.sasa(x[:, :-1], top)
    with pytest.raises(ValueError, match="res_ptr"):
        metrics.sasa_lists(x, [1.7] * top.n_atoms, [0, 5, 3, top.n_atoms])


@pytest.mark.gpu
@pytest.mark.parametrize("key", [("ball", 257, 96, True), ("chain", 65, 960, False), ("chain", 3, 1024, True)])
def test_results_are_bit_identical_and_independent_of_the_batch(key):
    a, b = run_case(key), run_case(key)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    S = obr.sasa_case(*key)["x"].shape[0]
    assert S == 3
    c = obr.sasa_case(*key)
    for s in range(S):
        for place in range(3):                                   # the structure alone, and at each place of a batch of 3
            others = [c["x"][(s + 1) % S], c["x"][(s + 2) % S]]
            batch = np.stack(others[:place] + [c["x"][s]] + others[place:])
            got = metrics.sasa_lists(dev(batch), c["vdw"], c["res_ptr"], probe=obr.PROBE, n_points=key[2])
            for k in a:
                assert torch.equal(got[k][place], a[k][s]), (k, s, place)
        alone = metrics.sasa_lists(dev(c["x"][s:s + 1]), c["vdw"], c["res_ptr"], probe=obr.PROBE, n_points=key[2])
        for k in a:
            assert torch.equal(alone[k][0], a[k][s]), (k, s)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [4, 257])
def test_non_finite_input_gets_the_defined_result_and_leaves_the_other_structures_alone(n):
    rng = np.random.default_rng(77 + n)
    x = np.stack([obr.ball(n, rng) for _ in range(3)]).astype(np.float32)
    vdw = rng.choice(obr.VDW, n)
    res_ptr = obr.residue_table(n)
    clean = metrics.sasa_lists(dev(x), vdw, res_ptr, n_points=96)
    assert bool(clean["finite"].all())
    for label, value in NAN_KINDS.items():
        for atom in (0, n // 2, n - 1):
            for comps in ((1,), (0, 1, 2)):
                for victim in (0, 1, 2):
                    if victim != 1 and (atom != n // 2 or comps != (1,)):
                        continue                                  # the middle structure everywhere, the others once per kind
                    bad = x.copy()
                    bad[victim, atom, list(comps)] = value
                    out = metrics.sasa_lists(dev(bad), vdw, res_ptr, n_points=96)
                    what = (label, atom, comps, victim)
                    assert out["finite"].tolist() == [s != victim for s in range(3)], what
                    assert bool((out["exposed"][victim] == -1).all()), what
                    assert bool(torch.isnan(out["atom"][victim]).all() and torch.isnan(out["residue"][victim]).all()), what
                    assert bool(torch.isnan(out["total"][victim])), what
                    for s in range(3):
                        if s != victim:
                            for k in ("atom", "residue", "total", "exposed"):
                                assert torch.equal(out[k][s], clean[k][s]), (what, k, s)


@pytest.mark.gpu
@pytest.mark.parametrize("m", obr.CONTACT_SIZES)
def test_contact_map_equals_the_float64_reference(m):
    c = obr.contact_case(m)
    for S in (1, obr.CONTACT_STRUCT):
        x = c["x"][:S]
        for sel, xx in ((c["sel"], x), (None, x[:, :m])):
            out = metrics.contact_map(dev(xx), sel=sel, cutoff=obr.CUTOFF)
            counts = out["counts"].cpu().numpy()
            cut2 = float(np.float32(obr.CUTOFF ** 2))
            want = (obr._d2(xx if sel is None else xx[:, sel], np.float64) < cut2).sum(0)
            np.fill_diagonal(want, 0)
            assert counts.dtype == np.int32 and counts.shape == (m, m) and out["n_struct"] == S
            assert np.array_equal(counts, want), (m, S, sel is None, int((counts != want).sum()))
            assert np.array_equal(counts, counts.T) and not np.diag(counts).any()
            assert out["frequency"].dtype == torch.float64
            assert np.array_equal(out["frequency"].cpu().numpy(), want / S)
    assert np.array_equal(want, c["counts_all"])                                   # the cached reference is this one


@pytest.mark.gpu
def test_contact_map_does_not_count_a_structure_for_the_pairs_of_its_nan_atom():
    c = obr.contact_case(65)
    sel = c["sel"]
    x = c["x"].copy()
    q = 17                                                                         # position in sel
    x[2, sel[q], 1] = np.nan
    x[4, sel[q]] = np.inf
    counts = metrics.contact_map(dev(x), sel=sel, cutoff=obr.CUTOFF)["counts"].cpu().numpy()
    cut2 = float(np.float32(obr.CUTOFF ** 2))
    hit = obr._d2(c["x"][:, sel], np.float64) < cut2
    want = hit.sum(0)
    want[q, :] = want[:, q] = hit[[0, 1, 3]][:, q, :].sum(0)
    np.fill_diagonal(want, 0)
    assert np.array_equal(counts, want) and (want[q] != c["counts_sel"][q]).any()
    with pytest.raises(ValueError, match="outside"):
        metrics.contact_map(dev(x), sel=[0, x.shape[1]])
    with pytest.raises(ValueError, match="cutoff"):
        metrics.contact_map(dev(x), cutoff=-1.0)


@pytest.mark.gpu
@pytest.mark.parametrize("n", obr.SIZES)
def test_radius_of_gyration_within_the_bound_of_the_moments(n):
    for shifted in (False, True):
        x = obr.sasa_case("ball", n, 96, shifted)["x"]
        got = metrics.radius_of_gyration(dev(x))
        assert got.dtype == torch.float64 and tuple(got.shape) == (x.shape[0],)
        want, g = obr.rg2(x)
        err = np.abs(got.cpu().numpy() ** 2 - want)
        bound = (n + 16) * 2.0 ** -52 * g / n
        print(f"n={n} shifted={shifted}: Rg {got.tolist()}, |Rg^2 - ref| / bound {(err / np.maximum(bound, 1e-300)).max():.3f}")
        assert (err <= bound).all(), (n, shifted, err, bound)
        if n >= 8:
            sel = list(range(0, n, 3))
            want, g = obr.rg2(x, sel)
            err = np.abs(metrics.radius_of_gyration(dev(x), sel=sel).cpu().numpy() ** 2 - want)
            assert (err <= (len(sel) + 16) * 2.0 ** -52 * g / len(sel)).all()
    bad = x.copy()
    bad[0, 0, 0] = np.nan
    out = metrics.radius_of_gyration(dev(bad))
    assert bool(torch.isnan(out[0])) and not bool(torch.isnan(out[1:]).any())


@pytest.mark.gpu
def test_buffers_are_written_before_they_are_read_and_only_inside():
    """tests/memcheck.py around the three functions: the results have the same bits under the three fills of every buffer
    the package allocates, and no byte outside a buffer changes."""
    from tests.test_buffer_discipline import hold
    c = obr.sasa_case("chain", 65, 96, False)
    cc = obr.contact_case(65)

    def case(g):
        x = g(torch.from_numpy(c["x"]), "xyz")
        out = metrics.sasa_lists(x, c["vdw"], c["res_ptr"], probe=obr.PROBE, n_points=96)
        res = {f"sasa_{k}": v for k, v in out.items()}
        xc = g(torch.from_numpy(cc["x"][:3]), "xyz_contacts")
        cm = metrics.contact_map(xc, sel=cc["sel"], cutoff=obr.CUTOFF)
        res.update(counts=cm["counts"], frequency=cm["frequency"], counts_all=metrics.contact_map(xc)["counts"])
        res.update(rg=metrics.radius_of_gyration(x), rg_sel=metrics.radius_of_gyration(x, sel=[0, 5, 64, 33]))
        return res, []
    hold("observables", case)


# ---------------------------------------------------------------------------------------------------------------- CLI
def _cli(cwd, *extra):
    cmd = [sys.executable, os.path.join(ROOT, "test.py"), "--synthetic", "--synthetic_weights", "--num_sampling_steps", "4",
           "--num_ensemble", "2"] + list(extra)
    res = subprocess.run(cmd, env=dict(os.environ, PYTHONPATH=ROOT), cwd=str(cwd), capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-1500:] + res.stderr[-3000:]
    files = {f: os.path.join(dp, f) for dp, _d, fs in os.walk(os.path.join(str(cwd), "logs")) for f in fs}
    return files, res.stdout


@pytest.mark.gpu
def test_cli_observables_end_to_end(tmp_path):
    from codlad_amd import synth
    from codlad_amd.utils.cg_input import template_topology
    (tmp_path / "on").mkdir()
    (tmp_path / "off").mkdir()
    on, stdout = _cli(tmp_path / "on", "--observables", "96")
    off, _ = _cli(tmp_path / "off")
    new = {f for f in on if f.endswith(("_sasa_residue.npy", "_rg.npy", "_ca_contacts.npy"))}
    assert set(on) - set(off) == new and set(off) <= set(on) and len(new) == 3 * 4        # the four PED-shaped proteins
    for f in off:
        assert open(on[f], "rb").read() == open(off[f], "rb").read(), f                   # nothing else changes
    assert "ensemble observables" in stdout and "Rg " in stdout and "SASA " in stdout
    for i, L in enumerate((46, 87, 92, 129)):
        name = f"synthetic_L{L}"
        xyz = np.load(on[f"{name}_xyz_recon.npy"])
        E, B, n_atoms = xyz.shape[:3]
        prot = synth.make_protein(L, 1000 + i, n_frames=1)
        top = template_topology([synth.IDX2THR[int(z)] for z in prot["z_full"]][1:-1])
        assert top.n_atoms == n_atoms and top.n_residues == L
        sasa, rg, ca = (np.load(on[f"{name}_{k}.npy"]) for k in ("sasa_residue", "rg", "ca_contacts"))
        assert sasa.shape == (E * B, L) and sasa.dtype == np.float32 and rg.shape == (E * B,) and ca.shape == (L, L)
        flat = dev(xyz.reshape(-1, n_atoms, 3))
        want = metrics.sasa(flat, top, n_points=96)
        assert np.array_equal(sasa, want["residue"].cpu().numpy(), equal_nan=True)
        assert np.array_equal(rg, metrics.radius_of_gyration(flat).cpu().numpy(), equal_nan=True)
        freq = metrics.contact_map(flat, sel=top.select("CA"), cutoff=8.0)["frequency"].cpu().numpy()
        assert np.array_equal(ca, freq) and (ca == ca.T).all() and not np.diag(ca).any() and ca.max() <= 1.0
