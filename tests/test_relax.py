"""Restrained clash relaxation on the device (codlad_relax / codlad_relax_energy, csrc/relax_kernels.hip; metrics.relax).

One evaluation is held to the float64 reference of tests/relax_ref.py on generic topologies (the graphs of
tests/test_geometry_check.py, with quads over random bonds), with margins asserted on the CPU - no free pair within 1e-4 A
of its sigma, no quad with a bond-angle |sin| in [0.05, 0.2] in the start structure - so that no inclusion decision can
differ.  Tolerance here: a POOLED one - |device - float64| <= 4 x ref_dev for each of the three energies and per gradient
component, ref_dev = the largest deviation, over ALL cases, of the SAME formulas evaluated in numpy float32 from float64.  One
structure sets the gradient's number (below), so this test alone lets a force that is wrong by 1 pass on every other atom of
every case, and holds energies of 0.02 to 14 000 to the same absolute 3e-3 to 6e-3.  It stays as a coarse net; the rule the
kernels are held to - per atom and per term, on these cases and on designed ones, and the loop step by step - is
tests/test_relax_fp64_parity.py's (tests/relax_cases.py).

The loop is held to its own rule EXACTLY, on its own numbers, from the trace of every run in this file (check_rule; against
float64 per step: tests/test_relax_fp64_parity.py), and to what it is for:
the planted clashes of tests/relax_ref.py (conditions asserted by tests/test_relax_host.py with the float64 reference)
must be gone, with the fixed atoms, the stereo flags and the covalent graph as they were.

Figures (printed by every run): ref_dev 7.11e-4 / 1.52e-3 / 1.11e-3 for the distance / torsion / repulsion energy and 0.620 per
gradient component (structure 2 of the 2 100-atom case has nearly coincident atoms and a gradient of 2.4e4; every other
structure is below 7e-4, one at 3.3e-3, on gradients of 30 to 3000); pooled bounds 2.84e-3 / 6.09e-3 / 4.46e-3 and 2.48; the
device's largest errors on an MI355X: 7.11e-4 / 1.52e-3 / 1.11e-3 and 0.622 - the float32 restatement's own.  Planted chains: clashes 7 / 6 / 8 -> 0, closest free pair 2.08 / 2.16 / 2.15 A after 200
iterations (160 / 163 / 159 accepted)."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from codlad_amd import _lib, metrics
from tests import relax_ref as rr
from tests import test_geometry_check as tg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = tg.SIZES                       # 2, 4, 255, 256, 257, 1023, 1024, 1025, 2100
MARGIN = 1e-4
F32 = np.float32


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(t):
    t = t.detach().cpu().contiguous()
    return t.view({4: torch.int32, 8: torch.int64, 1: torch.uint8}[t.element_size()])


# ------------------------------------------------------------------------------------------ one evaluation: the inputs
@functools.lru_cache(maxsize=None)
def case(n):
    """The graph of test_geometry_check.case(n) with quads over about a third of its bonds; xyz0 = its three structures,
    xyz = xyz0 + N(0, 0.1 A), both fp32, moved off the margins here.  -> dict with the float64 and float32 references."""
    radius, bonds, xyz0, _refs = tg.case(n)
    rng = np.random.default_rng(2000 + n)
    rigid = [tuple(b) for b in bonds.tolist() if rng.random() < 0.35]
    quads = metrics.torsion_quads(bonds, rigid, n).numpy().astype(np.int64)
    T = rr.tables(radius, bonds, quads)
    xyz0 = xyz0.copy()
    for s in range(3):
        for _ in range(200):                                  # quads near the weight threshold: move their atoms in xyz0
            sines = rr.angle_sines(xyz0[s].astype(np.float64), quads) if len(quads) else np.zeros((0, 2))
            bad = ((sines >= 0.05) & (sines <= 0.2)).any(-1)
            if not bad.any():
                break
            atoms = np.unique(quads[bad])
            xyz0[s, atoms] += rng.normal(0, 0.3, (len(atoms), 3)).astype(F32)
    xyz = (xyz0 + rng.normal(0, 0.1, xyz0.shape)).astype(F32)
    for s in range(3):
        for _ in range(50):                                   # free pairs near sigma: move one of their atoms in xyz
            near = np.nonzero(np.abs(_sigma_gap(xyz[s], T)) < MARGIN)[0]
            if not len(near):
                break
            atoms = np.unique(T["free_j"][near])
            xyz[s, atoms] += rng.normal(0, 0.01, (len(atoms), 3)).astype(F32)
    fixed = rng.random(n) < 0.2
    ref64 = [rr.energy(xyz[s], xyz0[s], T, fixed) for s in range(3)]
    ref32 = [rr.energy(xyz[s], xyz0[s], T, fixed, dtype=F32) for s in range(3)]
    return dict(radius=radius, bonds=bonds, quads=quads, T=T, xyz0=xyz0, xyz=xyz, fixed=fixed, ref64=ref64, ref32=ref32)


def _sigma_gap(x, T):
    d = rr._dist(x.astype(np.float64), T["free_i"], T["free_j"], np.float64)[1]
    return d - (T["radius"][T["free_i"]] + T["radius"][T["free_j"]]) * rr.DEFAULTS["contact_scale"]


@functools.lru_cache(maxsize=None)
def bounds():
    """(bound per energy [3], bound per gradient component, ref_dev of each) over ALL cases."""
    dev_e, dev_g = np.zeros(3), 0.0
    for n in SIZES:
        c = case(n)
        for (e64, g64, _), (e32, g32, _) in zip(c["ref64"], c["ref32"]):
            dev_e = np.maximum(dev_e, np.abs(e32 - e64))
            dev_g = max(dev_g, float(np.abs(g32.astype(np.float64) - g64).max()))
    print(f"ref_dev energies {dev_e} gradient {dev_g:.3e}; bounds {4 * dev_e} and {4 * dev_g:.3e}")
    return 4 * dev_e, 4 * dev_g, dev_e, dev_g


def test_inputs_keep_their_margins_and_use_every_term():
    quads_w0 = 0
    for n in SIZES:
        c = case(n)
        for s in range(3):
            assert np.abs(_sigma_gap(c["xyz"][s], c["T"])).min(initial=1.0) >= MARGIN, (n, s)
            if len(c["quads"]):
                sines = rr.angle_sines(c["xyz0"][s].astype(np.float64), c["quads"])
                assert not ((sines >= 0.05) & (sines <= 0.2)).any(), (n, s)
                quads_w0 += int((sines < 0.05).any(-1).sum())
            if n >= 255:
                assert (c["ref64"][s][0] > 0).all(), (n, s)                 # all three terms are active
    print(f"quads of weight 0 over all cases: {quads_w0}")
    _be, _bg, dev_e, dev_g = bounds()
    assert (dev_e > 0).all() and dev_g > 0


# --------------------------------------------------------------------------------------------------- one evaluation
@pytest.mark.gpu
@pytest.mark.parametrize("n_struct", [1, 3])
@pytest.mark.parametrize("n", SIZES)
def test_one_evaluation_against_float64(n, n_struct):
    c = case(n)
    tol_e, tol_g, _de, _dg = bounds()
    out = metrics.relax_energy_lists(cuda(c["xyz"][:n_struct]), c["radius"], c["bonds"], c["quads"], xyz0=cuda(c["xyz0"][:n_struct]),
                                     fixed=c["fixed"])
    e, g, gmax = out["energy"].cpu().numpy(), out["grad"].cpu().numpy(), out["gmax"].cpu().numpy()
    assert e.dtype == np.float64 and e.shape == (n_struct, 3) and g.dtype == F32 and g.shape == (n_struct, n, 3)
    err_e, err_g = np.zeros(3), 0.0
    for s in range(n_struct):
        e64, g64, _ = c["ref64"][s]
        err_e = np.maximum(err_e, np.abs(e[s] - e64))
        err_g = max(err_g, float(np.abs(g[s].astype(np.float64) - g64).max()))
        assert not g[s][c["fixed"]].any()
        assert gmax[s] == np.abs(g[s]).max()
    print(f"n={n} S={n_struct}: energy errors {err_e} (bounds {tol_e}), gradient error {err_g:.3e} (bound {tol_g:.3e})")
    assert (err_e <= tol_e).all() and err_g <= tol_g, (err_e, tol_e, err_g, tol_g)
    assert torch.equal(out["total"], (out["energy"][:, 0] + out["energy"][:, 1]) + out["energy"][:, 2])


# ------------------------------------------------------------------------------------------------------ the loop's rule
def check_rule(out, n_iter, h0=rr.DEFAULTS["h0"], h_max=rr.DEFAULTS["h_max"]):
    """The trace of one metrics.relax call against the rule, exactly, on the device's own numbers."""
    e, et = out["trace_energy"].cpu().numpy(), out["trial_energy"].cpu().numpy()
    h, acc, gm = out["step"].cpu().numpy(), out["accepted"].cpu().numpy(), out["gmax"].cpu().numpy()
    S = e.shape[0]
    assert e.shape == (S, n_iter + 1) and et.shape == h.shape == acc.shape == gm.shape == (S, n_iter)
    assert e.dtype == et.dtype == np.float64 and h.dtype == gm.dtype == F32 and acc.dtype == np.uint8
    assert np.array_equal(acc.astype(bool), et < e[:, :-1])
    assert np.array_equal(e[:, 1:], np.where(acc.astype(bool), et, e[:, :-1]))
    assert (np.diff(e, axis=1) <= 0).all()
    if n_iter:
        assert (h[:, 0] == F32(h0)).all()
        grown = np.minimum(h[:, :-1] * F32(1.2), F32(h_max)).astype(F32)
        halved = (h[:, :-1] * F32(0.5)).astype(F32)
        assert np.array_equal(h[:, 1:], np.where(acc[:, :-1].astype(bool), grown, halved))
        assert (gm >= 0).all()
    assert np.array_equal(out["n_accepted"].cpu().numpy(), acc.sum(1))
    assert np.array_equal(out["energy0"].cpu().numpy(), e[:, 0]) and np.array_equal(out["energy"].cpu().numpy(), e[:, -1])
    return e, acc


@pytest.mark.gpu
def test_zero_and_one_iteration_are_the_stated_formula_bit_for_bit():
    c = rr.planted_case("r32")
    x = cuda(c["xyz"][None])
    out0 = metrics.relax(x, c["top"], n_iter=0)
    check_rule(out0, 0)
    assert torch.equal(bits(out0["xyz"]), bits(x))
    ev = metrics.relax_energy(x, c["top"])
    assert torch.equal(bits(out0["energy0"]), bits(ev["total"]))
    out1 = metrics.relax(x, c["top"], n_iter=1)
    e, acc = check_rule(out1, 1)
    assert acc[0, 0] == 1                                                     # a clash: the first small step goes downhill
    g, gmax = ev["grad"].cpu().numpy()[0], ev["gmax"].cpu().numpy()[0]
    assert out1["gmax"].cpu().numpy()[0, 0] == gmax
    scale = F32(F32(rr.DEFAULTS["h0"]) / gmax)
    want = (c["xyz"] - (scale * g).astype(F32)).astype(F32)
    assert np.array_equal(out1["xyz"].cpu().numpy()[0].view(np.int32), want.view(np.int32))
    # the trial's energy is what one evaluation of the result gives, against the input as the start structure
    again = metrics.relax_energy(out1["xyz"], c["top"], xyz0=x)
    assert torch.equal(bits(again["total"]), bits(out1["trial_energy"][:, 0]))


# ---------------------------------------------------------------------------------------------------- planted clashes
@pytest.mark.gpu
@pytest.mark.parametrize("key", list(rr.PLANTED))
def test_planted_clashes_are_relaxed_away(key):
    c = rr.planted_case(key)
    top, T, n_iter = c["top"], c["T"], c["n_iter"]
    x = cuda(c["xyz"][None])
    before = metrics.geometry_check(x, top)
    ste0 = metrics.stereo_check(x, top)
    out = metrics.relax(x, top, n_iter=n_iter)
    e, acc = check_rule(out, n_iter)
    y = out["xyz"]
    after = metrics.geometry_check(y, top)
    ste1 = metrics.stereo_check(y, top)
    y_np = y.cpu().numpy()[0]
    d_min = float(rr.free_pair_distances(y_np, T).min())
    print(f"{key}: {top.n_atoms} atoms, clashes {int(before['clash'][0])} -> {int(after['clash'][0])}, min_dist "
          f"{float(before['min_dist'][0]):.3f} -> {float(after['min_dist'][0]):.3f} (float64: {d_min:.3f}), E {e[0, 0]:.2f} -> "
          f"{e[0, -1]:.4f}, {int(acc.sum())} of {n_iter} accepted")
    assert int(before["clash"][0]) == rr.clashes(c["xyz"], T) > 0
    assert rr.clashes(y_np, T) == 0 and int(after["clash"][0]) == 0
    assert e[0, -1] < e[0, 0]
    fixed = c["fixed"]
    assert fixed.sum() == top.n_residues
    assert np.array_equal(y_np[fixed].view(np.int32), c["xyz"][fixed].view(np.int32))
    assert torch.equal(ste1["flags"], ste0["flags"]) and torch.equal(ste1["counts"], ste0["counts"])
    assert int(after["broken"][0]) <= int(before["broken"][0]) and int(after["spurious"][0]) <= int(before["spurious"][0])


# ---------------------------------------------------------------------------------------- independence and determinism
@pytest.mark.gpu
def test_clean_structure_is_left_alone_and_structures_do_not_see_each_other():
    c, n_iter = rr.planted_case("r60"), 40
    top = c["top"]
    clean = cuda(c["xyz0"][None])
    out = metrics.relax(clean, top, n_iter=n_iter)
    e, acc = check_rule(out, n_iter)
    assert torch.equal(bits(out["xyz"]), bits(clean)) and not acc.any() and not e.any() and out["converged"].tolist() == [1]
    assert not out["gmax"].any()
    # a second planted structure: the same chain with the planted side chains of the first half only
    half = c["xyz0"].copy()
    first = np.isin(top.residue_of_atom, sorted(c["residues"])[:3])
    half[first] = c["xyz"][first]
    batch = cuda(np.stack([c["xyz"], c["xyz0"], half]))
    a = metrics.relax(batch, top, n_iter=n_iter)
    e, acc = check_rule(a, n_iter)
    assert a["converged"].tolist() == [0, 1, 0] and acc[0].any() and acc[2].any() and not acc[1].any()
    assert torch.equal(bits(a["xyz"][1]), bits(clean[0])) and not e[1].any()
    keys = ("xyz", "trace_energy", "trial_energy", "step", "accepted", "gmax", "converged")
    b = metrics.relax(batch, top, n_iter=n_iter)
    for k in keys:
        assert torch.equal(bits(a[k]), bits(b[k])), k                                    # two runs: the same bits
    for s in range(3):
        one = metrics.relax(batch[s:s + 1], top, n_iter=n_iter)
        for k in keys:
            assert torch.equal(bits(one[k][0]), bits(a[k][s])), (k, s)                  # alone: the same bits
    assert set(top._relax_tables) >= {(2, "host"), (2, "cuda:0")}                       # built once, kept on the topology
    # an explicit mask: nothing may move, so nothing does
    frozen = metrics.relax(batch, top, n_iter=3, fixed=np.ones(top.n_atoms, dtype=bool))
    assert torch.equal(bits(frozen["xyz"]), bits(batch)) and frozen["converged"].tolist() == [1, 1, 1]


# ------------------------------------------------------------------------------------------------------------ buffers
@pytest.mark.gpu
def test_buffers_are_written_before_they_are_read():
    """relax_energy and relax (n = 257: a second row block; S = 2; 8 iterations) under the four-run rule of
    tests/test_buffer_discipline.py.  Defined: energy, grad, gmax; xyz and every trace table.  Scratch: zone-checked only."""
    from tests.test_buffer_discipline import hold
    c = case(257)

    def run(g):
        x, x0 = g(torch.from_numpy(c["xyz"][:2]), "xyz"), g(torch.from_numpy(c["xyz0"][:2]), "xyz0")
        ev = metrics.relax_energy_lists(x, c["radius"], c["bonds"], c["quads"], xyz0=x0, fixed=c["fixed"])
        lo = metrics.relax_lists(x, c["radius"], c["bonds"], c["quads"], fixed=c["fixed"], n_iter=8)
        res = dict(energy=ev["energy"], grad=ev["grad"], gmax=ev["gmax"])
        res.update({f"loop_{k}": lo[k] for k in ("xyz", "trace_energy", "trial_energy", "step", "accepted", "gmax", "converged")})
        return res, []
    hold("relax n=257", run)


# ------------------------------------------------------------------------------------------------------------- errors
@pytest.mark.gpu
def test_bad_arguments_return_an_error_and_a_message():
    c = rr.planted_case("r32")
    top = c["top"]
    x = cuda(c["xyz"][None])
    with pytest.raises(ValueError, match="atoms"):
        metrics.relax(x[:, :-1].contiguous(), top)
    with pytest.raises(ValueError, match="atoms"):
        metrics.relax_energy(x[:, :-1].contiguous(), top)
    with pytest.raises(ValueError, match="n_iter"):
        metrics.relax(x, top, n_iter=-1)
    with pytest.raises(ValueError, match="fixed"):
        metrics.relax(x, top, fixed=[True])
    with pytest.raises(TypeError, match="k_x"):
        metrics.relax(x, top, k_x=1.0)
    for name in ("k_r", "k_t", "k_c", "contact_scale", "h0", "h_max"):
        with pytest.raises(RuntimeError, match="codlad_relax"):
            metrics.relax(x, top, n_iter=1, **{name: 0.0})
    for name in ("k_r", "k_t", "k_c", "contact_scale"):
        with pytest.raises(RuntimeError, match="codlad_relax_energy"):
            metrics.relax_energy(x, top, **{name: -1.0})
    # straight to the C ABI
    lib, p, f = _lib.lib(), _lib.ptr, C.c_float
    t = metrics._relax_tables_on(top, 2, x.device)
    n = top.n_atoms
    fx = torch.zeros(n, dtype=torch.uint8, device="cuda")
    out = torch.empty_like(x)
    e = torch.empty(1, 2, dtype=torch.float64, device="cuda")
    scratch = torch.empty(lib.codlad_relax_scratch_bytes(1, n, t["pair_j"].shape[0], t["quads"].shape[0], 1), dtype=torch.uint8,
                          device="cuda")
    tabs = metrics._relax_table_args(t)
    four = [torch.empty(1, 1, dtype=d, device="cuda") for d in (torch.float64, torch.float32, torch.uint8, torch.float32)]
    conv = torch.empty(1, dtype=torch.uint8, device="cuda")
    ok = [p(x), 1, n, p(t["radius"]), p(fx)] + tabs + [f(100), f(50), f(30), f(1.6), f(0.01), f(0.1), 1, p(out), p(e)] + \
        [p(a) for a in four] + [p(conv), p(scratch), None]
    assert lib.codlad_relax(*ok) == 0
    torch.cuda.synchronize()
    for k, bad in ((0, None), (1, 0), (2, 0), (2, 70000), (3, None), (4, None), (9, -1), (15, f(0.0)), (18, f(-1.0)), (19, f(0.0)),
                   (20, f(0.0)), (21, -1), (22, None), (22, p(x)), (23, None), (24, None), (28, None), (29, None)):
        args = list(ok)
        args[k] = bad
        assert lib.codlad_relax(*args) != 0, k
        assert b"codlad_relax" in lib.codlad_last_error(), k
    assert lib.codlad_relax_scratch_bytes(0, n, 0, 0, 1) < 0


# ---------------------------------------------------------------------------------------------------------------- CLI
def _cli(cwd, *extra):
    cmd = [sys.executable, os.path.join(ROOT, "test.py"), "--synthetic_weights", "--num_sampling_steps", "3", "--num_ensemble", "2",
           "--seed", "7"] + list(extra)
    res = subprocess.run(cmd, env=dict(os.environ, PYTHONPATH=ROOT), cwd=str(cwd), capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-1500:] + res.stderr[-3000:]
    files = {f: os.path.join(dp, f) for dp, _d, fs in os.walk(os.path.join(str(cwd), "logs")) for f in fs}
    return files, res.stdout


@pytest.mark.gpu
def test_cli_relax_end_to_end(tmp_path):
    from codlad_amd.utils.cg_input import template_topology
    from tests.test_dataset_builder import golden_frames, write_full_pdb
    top, full, _og, _info, _g5 = golden_frames("N6_L46_B3")
    out = {}
    for name, extra in (("on", ["--relax", "50", "--geometry_check"]), ("off", ["--geometry_check"])):
        d = tmp_path / name
        os.makedirs(str(d))
        write_full_pdb(str(d / "full.pdb"), top, full)
        with open(str(d / "full.pdb")) as f, open(str(d / "ca.pdb"), "w") as g:
            g.writelines(l for l in f if l[:6] not in ("ATOM  ", "HETATM") or l[12:16].strip() == "CA")
        out[name] = _cli(d, "--cg_pdb", "ca.pdb", *extra)
    (files, stdout), (files_off, stdout_off) = out["on"], out["off"]
    base = {f"ca_{k}.npy" for k in ("xyz_recon", "geometry", "geometry_min")}
    assert set(files_off) == base and "relax" not in stdout_off
    assert set(files) == base | {"ca_xyz_unrelaxed.npy", "ca_relax.npy"}
    assert "relax ca:" in stdout and "clashes" in stdout and "min_dist" in stdout
    inner = template_topology(top.res_names).subset_residues(1, 47)
    raw, relaxed = np.load(files["ca_xyz_unrelaxed.npy"]), np.load(files["ca_xyz_recon.npy"])
    # without the flag: the same bytes as the unrelaxed coordinates of the run with it (the sampler is seeded)
    assert np.array_equal(np.load(files_off["ca_xyz_recon.npy"]).view(np.int32), raw.view(np.int32))
    assert raw.shape == relaxed.shape and raw.dtype == relaxed.dtype == F32
    want = metrics.relax(cuda(raw).reshape(-1, inner.n_atoms, 3), inner, n_iter=50)
    assert np.array_equal(relaxed.reshape(-1, inner.n_atoms, 3).view(np.int32), want["xyz"].cpu().numpy().view(np.int32))
    trace = np.load(files["ca_relax.npy"])
    E_B = relaxed.reshape(-1, inner.n_atoms, 3).shape[0]
    assert trace.dtype == np.float64 and trace.shape == (E_B, 3)                  # energy0, energy, accepted steps
    assert np.array_equal(trace[:, 0], want["energy0"].cpu().numpy()) and np.array_equal(trace[:, 1], want["energy"].cpu().numpy())
    assert np.array_equal(trace[:, 2], want["n_accepted"].cpu().numpy().astype(np.float64))
    geo = np.load(files["ca_geometry.npy"])
    by_hand = metrics.geometry_check(cuda(relaxed).reshape(-1, inner.n_atoms, 3), inner)
    assert np.array_equal(geo, by_hand["counts"].cpu().numpy())                   # the check saw the relaxed coordinates
