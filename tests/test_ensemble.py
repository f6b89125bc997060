"""Ensemble analysis on the device (codlad_amd/csrc/ensemble_kernels.hip through codlad_amd.metrics) against the float64
SVD reference of tests/ensemble_ref.py.

The bound, everywhere: |msd_dev - max(msd_ref, 0)| <= (n + 16) 2^-52 e0 / n with e0 = Ga + Gb (ensemble_ref.msd_bound
states where it comes from).  Every (size, category, offset) is asserted; none is skipped."""
import os

import numpy as np
import pytest
import torch

from codlad_amd import metrics as gm
from tests import ensemble_ref as er
from tests.cli_script import load_cli

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _two_prod(x, y):
    """x * y = p + e exactly in float64 (Veltkamp split, Dekker's product)."""
    p = x * y
    cx, cy = 134217729.0 * x, 134217729.0 * y
    xh, yh = cx - (cx - x), cy - (cy - y)
    xl, yl = x - xh, y - yh
    return p, ((xh * yh - p) + xh * yl + xl * yh) + xl * yl


def msd_after(a, R, t, b):
    """msd of a @ R.T + t against b for the transform as reported, in float64 with a compensated evaluation: every
    residual R a + t - b is the correctly rounded sum (math.fsum) of its eight exact float64 parts (three products as
    p + e, t, -b), and so is the sum of their squares.  A plain float64 evaluation rounds every moved coordinate to
    2^-53 |x|, which for a structure 1000 A from the origin and a residual of 0.1 A is an error of 1e-14 A^2 of the CHECK
    - more than the whole bound when e0 / n is 0.01 A^2 (two atoms)."""
    import math
    a, b = a.astype(np.float64), b.astype(np.float64)
    parts = []
    for c in range(3):
        p, e = _two_prod(a[:, c:c + 1], R[None, :, c])              # [n, 3]: R[r][c] a[c]
        parts += [p, e]
    parts += [np.broadcast_to(t, b.shape), -b]
    parts = np.stack(parts, -1).reshape(-1, 8)
    d = np.array([math.fsum(row) for row in parts.tolist()])
    sq, lo = _two_prod(d, d)
    return math.fsum(np.concatenate((sq, lo)).tolist()) / a.shape[0]


@pytest.mark.parametrize("n", er.SIZES)
def test_msd_and_transform_hold_the_bound_for_every_category(n):
    """Tests 1 and 2 of the issue in one launch per size: the msd bound; R proper orthogonal; the msd of the moved
    coordinates equals the reported msd within the same bound; for the noisy and the rigid copies of n >= 4 atoms
    `superpose` equals the host-aligned coordinates rounded to fp32 within 2 ulp of max |b|."""
    labels, a, b, refs = er.cases_of_size(n)
    msd, R, t = gm.superposed_rmsd_batch(dev(a), dev(b), squared=True, return_transform=True)
    rmsd = gm.superposed_rmsd_batch(dev(a), dev(b))
    moved = gm.superpose(dev(a), dev(b)).cpu().numpy()
    assert msd.dtype == R.dtype == t.dtype == torch.float64 and moved.dtype == np.float32
    msd, R, t, rmsd = msd.cpu().numpy(), R.cpu().numpy(), t.cpu().numpy(), rmsd.cpu().numpy()
    for k, ((cat, off), ref) in enumerate(zip(labels, refs)):
        what = (n, cat, off)
        bound = er.msd_bound(n, ref["e0n"])
        err = abs(msd[k] - max(ref["msd"], 0.0))
        print(f"n={n} {cat} off={off}: msd {msd[k]:.6e} err/bound {err / bound if bound else err:.3f}")
        if ref["e0n"] == 0.0:
            assert msd[k] == 0.0, what
        assert err <= bound, (what, msd[k], ref["msd"], bound)
        assert abs(rmsd[k] - np.sqrt(msd[k])) <= er.EPS * rmsd[k], what          # the same msd, one square root each
        assert np.abs(R[k].T @ R[k] - np.eye(3)).sum(1).max() <= 64 * er.EPS, what
        assert np.linalg.det(R[k]) > 0, what
        back = msd_after(a[k], R[k], t[k], b[k])
        assert abs(back - msd[k]) <= bound, (what, back, msd[k], bound)
        if cat in ("noisy", "rigid") and n >= 4:
            host = (a[k].astype(np.float64) @ ref["R"].T + ref["t"]).astype(np.float32)
            lim = 2 * 2.0 ** -23 * float(np.abs(b[k]).max())
            assert np.abs(host.astype(np.float64) - moved[k].astype(np.float64)).max() <= lim, what


@pytest.mark.parametrize("P", (1, 7, 300))
def test_batches_of_pairs_and_a_single_target(P):
    """P pairs per launch, and the [n, 3] form of b (one target for all)."""
    n = 257
    a, b = er.batch(P, n, 40 + P)
    msd = gm.superposed_rmsd_batch(dev(a), dev(b), squared=True).cpu().numpy()
    one = gm.superposed_rmsd_batch(dev(a), dev(b[0]), squared=True).cpu().numpy()
    assert msd.shape == one.shape == (P,)
    for k in range(P):
        ref = er.kabsch(a[k], b[k])
        assert abs(msd[k] - max(ref["msd"], 0.0)) <= er.msd_bound(n, ref["e0n"]), k
    for k in range(0, P, 37):
        ref = er.kabsch(a[k], b[0])
        assert abs(one[k] - max(ref["msd"], 0.0)) <= er.msd_bound(n, ref["e0n"]), k
    assert one[0] == msd[0]


def test_selection_fits_the_subset_and_moves_all_atoms():
    n = 300
    a, b = er.batch(7, n, 77)
    sel = [5, 3, 299, 0, 128, 64, 63, 255, 256, 17, 200]
    ia = np.array(sel)
    got, R, t = gm.superposed_rmsd_batch(dev(a), dev(b), sel=sel, squared=True, return_transform=True)
    sub, Rs, ts = gm.superposed_rmsd_batch(dev(a[:, ia]), dev(b[:, ia]), squared=True, return_transform=True)
    assert torch.equal(got, sub) and torch.equal(R, Rs) and torch.equal(t, ts)      # the same sums in the same order
    moved = gm.superpose(dev(a), dev(b), sel=torch.tensor(sel)).cpu().numpy()
    R, t = R.cpu().numpy(), t.cpu().numpy()
    for k in range(7):
        want = (a[k].astype(np.float64) @ R[k].T + t[k]).astype(np.float32)
        # fp64 on both sides and one rounding each: equal up to 1 ulp where the two fp64 results straddle a tie
        assert np.abs(want.astype(np.float64) - moved[k]).max() <= 2.0 ** -23 * float(np.abs(b[k]).max()), k
        assert not np.array_equal(moved[k][1], a[k][1])                               # an atom outside sel moved too
    with pytest.raises(ValueError, match="outside"):
        gm.superposed_rmsd_batch(dev(a), dev(b), sel=[0, n])


def test_replay_is_bit_identical_and_a_pair_does_not_see_its_neighbours():
    n, P = 1000, 300
    a, b = er.batch(P, n, 9)
    da, db = dev(a), dev(b)
    first = [x.clone() for x in gm.superposed_rmsd_batch(da, db, squared=True, return_transform=True)]
    again = gm.superposed_rmsd_batch(da, db, squared=True, return_transform=True)
    for x, y in zip(first, again):
        assert torch.equal(x, y)
    for k in (0, 1, 149, 299):
        alone = gm.superposed_rmsd_batch(da[k:k + 1], db[k:k + 1], squared=True, return_transform=True)
        for x, y in zip(first, alone):
            assert torch.equal(x[k:k + 1], y), k
    perm = torch.randperm(P, generator=torch.Generator().manual_seed(1)).to(DEV)
    shuffled = gm.superposed_rmsd_batch(da[perm].contiguous(), db[perm].contiguous(), squared=True, return_transform=True)
    for x, y in zip(first, shuffled):
        assert torch.equal(x[perm], y)


@pytest.mark.parametrize("G,F,n,sel", [(2, 1, 65, None), (2, 3, 65, None), (5, 1, 65, None), (5, 3, 65, None),
                                       (5, 3, 300, list(range(0, 300, 7))),
                                       (3, 2, 4099, None), (3, 1, 5376, None), (2, 2, 5377, None)])
def test_pairwise_rmsd_is_symmetric_with_a_zero_diagonal_and_the_pair_kernels_bits(G, F, n, sel):
    """Up to 5376 atoms (or selected atoms) conformation i is staged in LDS, from 5377 on it is read from memory: both
    walks must return the pair kernel's bits."""
    rng = np.random.default_rng(G * 1000 + F * 10 + n)
    x = (rng.standard_normal((1, F, n, 3)) * 5.0 + rng.standard_normal((G, F, n, 3)) * 0.8 + 300.0).astype(np.float32)
    dx = dev(x)
    m = gm.pairwise_rmsd(dx, sel=sel)
    assert m.shape == (F, G, G) and m.dtype == torch.float64
    assert torch.equal(m, m.transpose(1, 2))
    assert torch.equal(torch.diagonal(m, dim1=1, dim2=2), torch.zeros(F, G, dtype=torch.float64, device=DEV))
    iu = [(i, j) for i in range(G) for j in range(i + 1, G)]
    for f in range(F):
        a = torch.stack([dx[i, f] for i, _ in iu])
        b = torch.stack([dx[j, f] for _, j in iu])
        want = gm.superposed_rmsd_batch(a, b, sel=sel)
        got = torch.stack([m[f, i, j] for i, j in iu])
        assert torch.equal(got, want), f
        assert float(want.min()) > 0.1                       # the pairs are not trivially superposable


def test_non_finite_coordinates_and_bad_indices_give_nan_not_a_perfect_fit():
    """A NaN or infinite coordinate (a diverged sample) must come back as NaN from every entry, never as RMSD 0; so must
    an out-of-range sel entry or pair index handed straight to the C ABI, as include/codlad_hip.h promises (the Python
    wrappers reject those before the call).  The diagonal of the pairwise matrix is written, not computed: it stays 0."""
    from codlad_amd import _lib
    n = 70
    a, b = er.batch(3, n, 5)
    for bad in (float("nan"), float("inf")):
        for pool in (0, 1):
            da, db = dev(a).clone(), dev(b).clone()
            (da, db)[pool][1, 69, 2] = bad
            for squared in (True, False):
                out, R, t = gm.superposed_rmsd_batch(da, db, squared=squared, return_transform=True)
                assert torch.isnan(out).tolist() == [False, True, False], (bad, pool, out)
                assert bool(torch.isnan(R[1]).any()) and not bool(torch.isnan(R[0]).any())
            assert bool(torch.isnan(gm.superpose(da, db)[1]).all())
    for n_big in (n, 5400):                                    # staged in LDS / read from memory
        x = dev(np.random.default_rng(3).standard_normal((3, 2, n_big, 3)).astype(np.float32) * 4.0)
        x[1, 0, n_big - 1, 0] = float("nan")
        m = gm.pairwise_rmsd(x)
        want = torch.tensor([[[0, 1, 0], [1, 0, 1], [0, 1, 0]], [[0, 0, 0]] * 3], dtype=torch.bool, device=DEV)
        assert torch.equal(torch.isnan(m), want), m
        assert torch.equal(torch.diagonal(m, dim1=1, dim2=2), torch.zeros(2, 3, dtype=torch.float64, device=DEV))
    gen = dev(a)[None].repeat(2, 1, 1, 1).contiguous()
    gen[0, 2, 0, 0] = float("nan")
    to_ref, to_mean = gm.diversity_terms(gen, dev(b))
    assert bool(torch.isnan(to_ref[0, 2])) and bool(torch.isnan(to_mean[:, 2]).all()) and not bool(torch.isnan(to_ref[1]).any())
    assert np.isnan(gm.compute_div([g for g in gen], dev(b)))
    # straight to the C ABI
    lib, st = _lib.lib(), _lib.stream_ptr(DEV)
    da, db = dev(a), dev(b)
    mom = lambda x, sel, k: gm._moments(x, x.shape[0], n, sel, k)  # noqa: E731
    pairs = torch.tensor([[0, 0], [1, 1], [2, 2]], dtype=torch.int32, device=DEV)
    out, Rt = torch.zeros(3, dtype=torch.float64, device=DEV), torch.zeros(3, 12, dtype=torch.float64, device=DEV)
    for entry in (n, -1, 2 ** 31 - 1):
        sel = torch.tensor([0, 5, entry, 9], dtype=torch.int32, device=DEV)
        ma, mb = mom(da, sel, 4), mom(db, sel, 4)
        assert bool(torch.isnan(ma).all()) and bool(torch.isnan(mb).all())
        rc = lib.codlad_ens_pair_msd(_lib.ptr(da), _lib.ptr(ma), 3, _lib.ptr(db), _lib.ptr(mb), 3, n, _lib.ptr(sel), 4,
                                     _lib.ptr(pairs), 3, 1, _lib.ptr(out), _lib.ptr(Rt), st)
        assert rc == 0 and bool(torch.isnan(out).all()), (entry, out)
        x = torch.stack((da, db)).contiguous()                           # [2, 3, n, 3]
        pw = torch.zeros(3, 2, 2, dtype=torch.float64, device=DEV)
        rc = lib.codlad_ens_pairwise(_lib.ptr(x), _lib.ptr(mom(x.reshape(6, n, 3), sel, 4)), 2, 3, n, _lib.ptr(sel), 4, 0,
                                     _lib.ptr(pw), st)
        assert rc == 0 and bool(torch.isnan(pw[:, 0, 1]).all()) and bool(torch.isnan(pw[:, 1, 0]).all()), (entry, pw)
    ma, mb = mom(da, None, 0), mom(db, None, 0)
    for bad_pair in ([1, 3], [3, 1], [-1, 0]):
        pp = torch.tensor([[0, 0], bad_pair, [2, 2]], dtype=torch.int32, device=DEV)
        rc = lib.codlad_ens_pair_msd(_lib.ptr(da), _lib.ptr(ma), 3, _lib.ptr(db), _lib.ptr(mb), 3, n, None, 0,
                                     _lib.ptr(pp), 3, 1, _lib.ptr(out), _lib.ptr(Rt), st)
        assert rc == 0 and torch.isnan(out).tolist() == [False, True, False] and bool(torch.isnan(Rt[1]).all()), bad_pair


def _div_inputs():
    """G = 4, F = 3, n = 257.  Coordinates are multiples of 2^-10 below 2^10 in magnitude: the fp32 sum of four of them
    is exact in any order, so the member mean of the device path (a torch op on the GPU) and of the host loop (a torch op
    on the CPU) are the same numbers and the two paths superpose on identical targets."""
    rng = np.random.default_rng(2024)
    base = rng.standard_normal((1, 3, 257, 3)) * 5.0 + 100.0
    gen = base + 0.8 * rng.standard_normal((4, 3, 257, 3))
    ref = base[0] + 0.5 * rng.standard_normal((3, 257, 3))
    q = lambda v: (np.round(v * 1024.0) / 1024.0).astype(np.float32)  # noqa: E731
    return q(gen), q(ref)


def test_diversity_terms_and_compute_div_against_the_host_loop():
    gen, ref = _div_inputs()
    G, F, n = gen.shape[:3]
    mean = torch.from_numpy(gen).mean(0).numpy()
    assert np.array_equal(mean, gen.astype(np.float64).mean(0).astype(np.float32))      # exact, see _div_inputs
    to_ref, to_mean = gm.diversity_terms(dev(gen), dev(ref))
    as_list = gm.diversity_terms([dev(g) for g in gen], dev(ref))
    assert torch.equal(as_list[0], to_ref) and torch.equal(as_list[1], to_mean)
    assert to_ref.shape == to_mean.shape == (G, F) and to_ref.dtype == torch.float64
    to_ref, to_mean = to_ref.cpu().numpy(), to_mean.cpu().numpy()
    rel = 0.0                                  # the largest relative error bound of a term
    for g in range(G):
        for p in range(F):
            for got, target in ((to_ref[g, p], ref[p]), (to_mean[g, p], mean[p])):
                r = er.kabsch(gen[g, p], target)
                want = np.sqrt(max(r["msd"], 0.0))
                host = gm.superposed_rmsd(torch.from_numpy(gen[g, p]), torch.from_numpy(target))
                # r_dev - r_ref = (msd_dev - msd_ref) / (r_dev + r_ref), plus half an ulp for each square root
                tol = er.msd_bound(n, r["e0n"]) / (got + want) + er.EPS * want
                tol_host = er.msd_bound(n, r["e0n"]) / (got + host) + er.EPS * host
                assert abs(got - want) <= tol and abs(got - host) <= tol_host, (g, p)
                rel = max(rel, tol_host / host)
    # compute_div = 1 - M / R with M, R the means of G F terms each.  Every term of the device path is within
    # rel * term of the host loop's, so is each mean; the two means are summed in different orders in fp64: G F 2^-52
    # relative each.  d(M / R) <= (M / R) (dM / M + dR / R), and the final division and subtraction round once each.
    cpu = gm.compute_div([torch.from_numpy(g) for g in gen], torch.from_numpy(ref))
    got = gm.compute_div([dev(g) for g in gen], dev(ref))
    ratio = 1.0 - cpu
    tol = ratio * 2 * (rel + G * F * er.EPS) + 2 * er.EPS
    print(f"compute_div device {got!r} cpu {cpu!r} diff {abs(got - cpu):.3e} tol {tol:.3e}")
    assert isinstance(got, float) and abs(got - cpu) <= tol
    assert 0.0 < got < 1.0


def _cli():
    return load_cli("codlad_cli_superpose")


def test_cli_superpose_helper():
    """What --superpose calls, on a fabricated [E, B, n, 3] ensemble whose members are rigidly displaced noisy copies."""
    cli = _cli()
    E, B, n = 4, 3, 130
    rng = np.random.default_rng(31)
    base = rng.standard_normal((B, n, 3)) * 6.0
    xyz = np.empty((E, B, n, 3), dtype=np.float32)
    for e in range(E):
        for f in range(B):
            xyz[e, f] = (base[f] + 0.4 * rng.standard_normal((n, 3))) @ er._rotation(rng).T + rng.standard_normal(3) * 20.0
    dxyz = dev(xyz)
    assert cli.superpose_models(dxyz, "none") is dxyz
    sel = list(range(1, n, 5))                      # stands in for the CA atoms
    for use in (None, sel):
        out = cli.superpose_models(dxyz, "first", sel=use)
        assert out.shape == dxyz.shape and out.dtype == torch.float32
        assert torch.equal(out[0], dxyz[0])
        idx = slice(None) if use is None else use
        sup = gm.superposed_rmsd_batch(dxyz[1:].reshape(-1, n, 3), dxyz[0].repeat(E - 1, 1, 1), sel=use).reshape(E - 1, B)
        plain_before = (dxyz[1:] - dxyz[0])[:, :, idx].pow(2).sum(-1).mean(-1).sqrt()
        plain_after = (out[1:].double() - out[0].double())[:, :, idx].pow(2).sum(-1).mean(-1).sqrt()
        assert bool((plain_before > 5.0).all())
        # the written coordinates are fp32: each carries 2^-24 |x| of rounding on top of the superposed RMSD
        assert torch.allclose(plain_after, sup, rtol=0, atol=4 * 2.0 ** -24 * float(dxyz.abs().max()))
    ref = dev((base + 0.0).astype(np.float32))
    out = cli.superpose_models(dxyz, "ref", ref=ref)
    after = (out.double() - ref.double()).pow(2).sum(-1).mean(-1).sqrt()
    sup = gm.superposed_rmsd_batch(dxyz.reshape(-1, n, 3), ref.repeat(E, 1, 1)).reshape(E, B)
    assert torch.allclose(after, sup, rtol=0, atol=4 * 2.0 ** -24 * float(dxyz.abs().max()))
    with pytest.raises(ValueError, match="true coordinates"):
        cli.superpose_models(dxyz, "ref")
    names = ["GLY", "ALA", "SER", "GLY"]
    atoms = [["CA"], ["N", "CA", "C", "O", "CB"], ["N", "CA", "C", "O", "CB", "OG"], ["CA"]]
    assert cli.ca_indices((names, atoms)) == [1, 6]


def test_evaluation_keeps_the_ensemble_on_the_device():
    """Evaluation.add no longer copies the reconstructed ensemble to the host, and report's diversity is the device
    path's number.  Against the host loop on CPU copies: the member mean is an fp32 sum whose order may differ between
    CPU and GPU, by at most one ulp of the largest coordinate X per coordinate of the target; an RMSD is a distance, so
    every to-mean term moves by at most sqrt(3) 2^-23 X, and so does their mean M; the diversity is 1 - M / R."""
    import types
    from tests import cases
    cli = _cli()
    d = {k: v.to(DEV) for k, v in cases.metric_inputs("small").items()}
    n_atoms = d["xyz"].shape[0] // 2
    z = torch.full((2 * n_atoms,), 6.0, device=DEV)
    batch = {"nxyz": torch.cat([z[:, None], d["xyz"]], 1), "num_atoms": torch.tensor([n_atoms, n_atoms]),
             "bond_edge_list": d["edge_list"], "nbr_list": d["nbr_list"], "bb_NO_list": d["bb_NO_list"],
             "interaction_list": d["interaction_list"], "pi_pi_list": d["pi_pi_list"], "ic": d["ic"], "mask": d["mask"],
             "mask_xyz_list": torch.tensor([3, 77], device=DEV)}
    ev = cli.Evaluation()
    g = torch.Generator().manual_seed(8)
    for member in range(3):
        noise = (0.2 * torch.randn(2, n_atoms, 3, generator=g)).to(DEV)
        ev.add(batch, d["ic_recon"], d["xyz_recon"].reshape(2, n_atoms, 3) + noise, n_atoms)
    assert all(t.is_cuda for t in ev.recon) and ev.true.is_cuda
    stats = ev.report("fabricated", types.SimpleNamespace(data_type="PED", num_ensemble=3, experiment="latent"))
    assert stats["diversity"] == gm.compute_div(ev.recon, ev.true)
    host = gm.compute_div([t.cpu() for t in ev.recon], ev.true.cpu())
    X = float(torch.stack(ev.recon).abs().max())
    R = float(gm.diversity_terms(ev.recon, ev.true)[0].mean())
    assert abs(stats["diversity"] - host) <= 3 ** 0.5 * 2.0 ** -23 * X / R + 1e-12


def test_cli_save_pdb_superpose_first_end_to_end(tmp_path):
    """test.py --save_pdb --superpose first on the synthetic PED set, one run: the real topology's CA atoms, the .npy
    left as sampled, the written models 1.. of every frame superposed on model 0 of that frame."""
    import subprocess
    import sys
    cmd = [sys.executable, os.path.join(ROOT, "test.py"), "--synthetic", "--synthetic_weights", "--synthetic_frames", "2",
           "--num_ensemble", "3", "--data_type", "PED", "--vae_type", "N6", "--exp", "clisup", "--num_sampling_steps", "3",
           "--save_pdb", "--superpose", "first"]
    res = subprocess.run(cmd, env=dict(os.environ, PYTHONPATH=ROOT), cwd=str(tmp_path), capture_output=True, text=True,
                         timeout=600)
    assert res.returncode == 0, res.stdout[-1500:] + res.stderr[-3000:]
    out_dir = os.path.join(str(tmp_path), "logs", "generated_samples_0_best", "clisup_PED")
    E, B = 3, 2
    for L in (46, 129):
        xyz = np.load(os.path.join(out_dir, f"synthetic_L{L}_xyz_recon.npy"))              # [E, B, n, 3], as sampled
        n = xyz.shape[2]
        models, names = [], []
        for line in open(os.path.join(out_dir, f"generated_traj_synthetic_L{L}.pdb")):
            if line.startswith("MODEL"):
                models.append([])
                names.append([])
            elif line.startswith("ATOM"):
                models[-1].append([float(line[30:38]), float(line[38:46]), float(line[46:54])])
                names[-1].append(line[12:16].strip())
        pdb = np.array(models).reshape(E, B, n, 3)
        ca = [k for k, nm in enumerate(names[0]) if nm == "CA"]
        assert len(ca) == L
        assert np.abs(pdb[0] - xyz[0]).max() <= 0.00051                                     # model 0: untouched, 3 decimals
        dx = dev(xyz)
        sup = gm.superposed_rmsd_batch(dx[1:].reshape(-1, n, 3), dx[0].repeat(E - 1, 1, 1), sel=ca).reshape(E - 1, B).cpu().numpy()
        plain = np.sqrt(((pdb[1:] - pdb[0])[:, :, ca] ** 2).sum(-1).mean(-1))
        before = np.sqrt(((xyz[1:] - xyz[0])[:, :, ca] ** 2).sum(-1).mean(-1))
        # every written coordinate is rounded to 0.0005 A: sqrt(3) * 0.0005 per atom on either side of the difference
        assert np.abs(plain - sup).max() <= 2 * 3 ** 0.5 * 0.0005, (L, plain, sup)
        assert (sup <= before + 1e-6).all()
