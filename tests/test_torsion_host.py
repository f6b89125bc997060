"""CPU checks of the torsion feature: the C ABI of codlad_torsion_* and codlad_feature_covariance (declared once, exported,
counted in _SIGS, limits mirrored, bad arguments refused before any HIP call), the kernels' registers, dihedral_quads
against stereo_tables, what the Python layer refuses, the float64 restatement of tests/torsion_ref.py within the header's
feature bound of longdouble on every pool the device suite uses, planted angles and answers derived by hand, and that the
cut-offs of the bitmap cases leave no pair undecided.  Largest fraction of the feature bound: 0.05 (random-walk chains),
0.04 (the planted peptide)."""
import json
import os
import re

import numpy as np
import pytest
import torch

from codlad_amd import _lib, build, metrics
from tests import stereo_ref as sr
from tests import torsion_ref as tr
from tests.test_cluster_host import _FakeCuda

LD = tr.LD
ENTRY_POINTS = (("int", "codlad_torsion_features", 8), ("long long", "codlad_torsion_mean_scratch_bytes", 2),
                ("int", "codlad_torsion_mean", 10), ("long long", "codlad_torsion_matrix_scratch_bytes", 2),
                ("int", "codlad_torsion_matrix", 13), ("int", "codlad_torsion_pairs", 10),
                ("long long", "codlad_feature_covariance_scratch_bytes", 2), ("int", "codlad_feature_covariance", 10))
KERNELS = ("torsion_features_kernel", "torsion_weight_kernel", "torsion_mean_kernel", "torsion_finish_kernel", "torsion_dev_kernel",
           "torsion_gram_kernelILi0", "torsion_gram_kernelILi1", "torsion_gram_kernelILi2", "torsion_pairs_kernel")


def test_header_declares_and_library_exports_the_entry_points():
    header = tr.HEADER
    lib = _lib.lib()
    for res, name, n_args in ENTRY_POINTS:
        decl = re.findall(r"\b" + res + r"\s+" + name + r"\s*\(([^;]*)\)\s*;", header)
        assert len(decl) == 1, name
        assert name in _lib.exported_symbols() and hasattr(lib, name)
        assert len(_lib._SIGS[name][1]) == decl[0].count(",") + 1 == n_args, name
    for macro, value, mine in (("MAX_T", 2048, _lib.TORSION_MAX_T), ("X_OPS", 11, _lib.TORSION_X_OPS), ("Y_OPS", 13, _lib.TORSION_Y_OPS)):
        assert f"#define CODLAD_TORSION_{macro} {value}\n" in header and mine == value == tr.macro(macro)
    assert metrics.TORSION_MAX_T == tr.MAX_T and 2 * tr.MAX_T == _lib.PCA_MAX_DIM and _lib.CLUSTER_MAX_N == _lib.PCA_MAX_N == 65536
    assert tr.matrix_bound(33) == 69 * tr.EPS and tr.pairs_bound(129) == 14 * tr.EPS and tr.term_bound() == 4 * tr.EPS
    assert tr.EPS == 2.0 ** -52 and float(tr.feature_bound(LD(0))) == 2 * tr.EPS
    # the chunk rule the mean bound stands on, on both sides of every threshold
    for N in (1, 16, 511, 512, 513, 527, 528, 529, 1473, 16383, 16384, 16385, 65535, 65536):
        nch, chunk = tr.chunks_of(N)
        assert nch <= 32 and chunk % 16 == 0 and nch * chunk >= N > (nch - 1) * chunk and min(N, chunk) <= tr.chunk_max(N)
        assert lib.codlad_torsion_mean_scratch_bytes(N, 7) == 8 * nch * 15
        assert tr.mean_bound(N) == (tr.chunk_max(N) + tr.chunk_max(N) // 64 + 72) * tr.EPS
    assert lib.codlad_torsion_matrix_scratch_bytes(130, 0) == 8 * 192 and lib.codlad_torsion_matrix_scratch_bytes(65, 3) == 8 * 192
    assert "#define CODLAD_ABI_VERSION 19\n" in header and _lib.ABI_VERSION == 19 and lib.codlad_abi_version() == 19
    assert "torsion_kernels.hip" in build.SOURCES and build.EXTRA_FLAGS["torsion_kernels.hip"] == ["-ffp-contract=off"]
    for name in ("dihedral_quads", "torsion_features", "circular_stats", "dihedral_pca", "dihedral_pca_project", "torsion_matrix",
                 "torsion_neighbours", "torsion_pairs", "cluster_torsion"):
        assert callable(getattr(metrics, name)) and name in metrics.torsion.__all__


def test_torsion_kernels_use_no_scratch_and_spill_nothing():
    build.build(force=False, verbose=False)
    if not os.path.exists(build.RESOURCES):
        build.build(force=True, verbose=False)
    with open(build.RESOURCES) as f:
        table = json.load(f)
    mine = {k: v for k, v in table.items() if v.get("source") == "torsion_kernels.hip"}
    for kernel in KERNELS:
        assert any(kernel in k for k in mine), (kernel, sorted(mine))
    assert len(mine) == len(KERNELS), sorted(mine)
    for name, r in mine.items():
        assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0, (name, r)
    trace = [v for k, v in table.items() if "pca_trace_kernel" in k]
    assert len(trace) == 1 and trace[0]["source"] == "pca_kernels.hip" and trace[0]["ScratchSize"] == 0


def test_argument_errors_return_a_negative_code_before_any_hip_call():
    """No GPU here: a call that got as far as a launch would return a positive hipError_t (or crash)."""
    lib = _lib.lib()
    buf = np.zeros(64, dtype=np.float64)                 # any non-null host address: never dereferenced
    p = buf.ctypes.data

    def refuses(fn, ok, cases):
        for k, bad in cases:
            args = list(ok)
            args[k] = bad
            assert getattr(lib, fn)(*args) < 0, (fn, k, bad)
            assert fn.encode() in lib.codlad_last_error(), (fn, k, bad)

    #     x  N  n_atoms quads T  F  finite stream
    ok = [p, 4, 36, p, 33, p, p, None]
    refuses("codlad_torsion_features", ok, [(k, None) for k in (0, 3, 5, 6)] +
            [(1, 0), (1, -1), (1, 65537), (2, 0), (2, -1), (4, 0), (4, -1), (4, tr.MAX_T + 1)])
    #     F  finite w   N  T   mean scal D  scratch stream
    ok = [p, p, None, 4, 33, p, p, None, p, None]
    refuses("codlad_torsion_mean", ok, [(k, None) for k in (0, 1, 5, 6, 8)] + [(3, 0), (3, 65537), (4, 0), (4, tr.MAX_T + 1)])
    #     Fx fx Na Fy    fy    Nb T  cut2 squared tmsd bits scratch stream
    ok = [p, p, 4, None, None, 0, 33, 1.0, 0, p, p, p, None]
    refuses("codlad_torsion_matrix", ok, [(k, None) for k in (0, 1, 11)] +
            [(2, 0), (2, -1), (2, 65537), (5, 3), (5, -1), (6, 0), (6, tr.MAX_T + 1), (7, -1.0), (7, float("inf")), (7, float("nan")),
             (3, p), (4, p)])
    args = list(ok)
    args[9] = args[10] = None                            # neither the table nor the bitmap
    assert lib.codlad_torsion_matrix(*args) < 0 and b"neither" in lib.codlad_last_error()
    cross = list(ok)
    cross[3], cross[4], cross[5] = p, p, 3               # two pools take no bitmap, and want Fy, Nb and finite_y together
    assert lib.codlad_torsion_matrix(*cross) < 0 and b"two pools" in lib.codlad_last_error()
    cross[10] = None
    refuses("codlad_torsion_matrix", cross, [(3, None), (4, None), (5, 0), (5, 65537)])
    #     Fa na Fb nb T  pairs K tmsd terms stream
    ok = [p, 4, p, 3, 33, p, 2, p, None, None]
    refuses("codlad_torsion_pairs", ok, [(k, None) for k in (0, 2, 5, 7)] + [(1, 0), (3, 0), (3, -1), (4, 0), (4, tr.MAX_T + 1), (6, 0), (6, -1)])
    #     D  w     finite N  d  scal cov total scratch stream
    ok = [p, None, p, 4, 7, p, p, p, p, None]
    refuses("codlad_feature_covariance", ok, [(k, None) for k in (0, 2, 5, 6, 7, 8)] + [(3, 0), (3, 65537), (4, 0), (4, 4097)])
    for fn, bads in (("codlad_torsion_mean_scratch_bytes", ((0, 3), (65537, 3), (4, 0), (4, tr.MAX_T + 1))),
                     ("codlad_torsion_matrix_scratch_bytes", ((0, 0), (65537, 0), (4, -1), (4, 65537))),
                     ("codlad_feature_covariance_scratch_bytes", ((0, 7), (65537, 7), (4, 0), (4, 4097)))):
        for bad in bads:
            assert getattr(lib, fn)(*bad) < 0 and fn.encode() in lib.codlad_last_error(), (fn, bad)
    # any d, where codlad_pca_covariance asks d % 3 == 0; the same scratch where both take it
    assert lib.codlad_feature_covariance_scratch_bytes(700, 66) == lib.codlad_pca_covariance_scratch_bytes(700, 66) == 8 * 2 * 3 * 4096
    assert lib.codlad_feature_covariance_scratch_bytes(4, 7) == 8 * 4096 and lib.codlad_pca_covariance_scratch_bytes(4, 7) < 0


def test_python_layer_refuses_what_it_cannot_run():
    x = torch.zeros(4, 7, 3)
    F = _FakeCuda(x)
    quads = tr.chain_quads(4)
    pairs = torch.tensor([[0, 1]])
    calls = (lambda x, q, **kw: metrics.torsion_features(x, q), lambda x, q, **kw: metrics.circular_stats(x, q, **kw),
             lambda x, q, **kw: metrics.dihedral_pca(x, q, 2, **kw), lambda x, q, **kw: metrics.torsion_matrix(x, q),
             lambda x, q, **kw: metrics.torsion_neighbours(x, q, 1.0), lambda x, q, **kw: metrics.torsion_pairs(x, F, pairs, q),
             lambda x, q, **kw: metrics.cluster_torsion(x, q, 1.0, **kw))
    for call in calls:
        with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
            call(x, quads)
        with pytest.raises(ValueError, match="non-empty"):
            call(_FakeCuda(torch.zeros(4, 7)), quads)
        with pytest.raises(ValueError, match=f"1 .. {tr.MAX_T} torsions, got 0"):
            call(F, np.zeros((0, 4), dtype=np.int32))
        with pytest.raises(ValueError, match=f"1 .. {tr.MAX_T} torsions, got {tr.MAX_T + 1}"):
            call(F, np.zeros((tr.MAX_T + 1, 4), dtype=np.int32))
        for bad in ([[0, 1, 2, 7]], [[-1, 1, 2, 3]]):
            with pytest.raises(ValueError, match="outside"):
                call(F, bad)
        with pytest.raises(ValueError, match="integer \\[T, 4\\] table"):
            call(F, quads.astype(np.float64))
        with pytest.raises(ValueError, match="integer \\[T, 4\\] table"):
            call(F, quads[:, :3])
        with pytest.raises(ValueError, match="at most 65536 structures"):
            call(_FakeCuda(torch.zeros(1, 1, 3).expand(65537, 7, 3)), quads)
    for call in (metrics.torsion_neighbours, metrics.cluster_torsion):
        for bad in (0.0, -1.0, float("nan"), float("inf"), "x"):
            with pytest.raises(ValueError, match="cutoff must be a positive finite number"):
                call(F, quads, bad)
    for call in (calls[1], calls[2], calls[6]):
        for bad, msg in (([1.0] * 3, "one value per structure"), ([1.0, float("nan"), 1.0, 1.0], "finite and >= 0"),
                         ([1.0, -1.0, 1.0, 1.0], "finite and >= 0")):
            with pytest.raises(ValueError, match=msg):
                call(F, quads, weights=bad)
    for bad in (0, 9, 1.0, True):                        # 1 .. min(64, 2 T) = 8
        with pytest.raises(ValueError, match="n_components must be an integer in 1 .. 8"):
            metrics.dihedral_pca(F, quads, n_components=bad)
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        metrics.torsion_matrix(F, quads, y=x)
    with pytest.raises(ValueError, match="7 and 8 atoms"):
        metrics.torsion_matrix(F, quads, y=_FakeCuda(torch.zeros(3, 8, 3)))
    with pytest.raises(ValueError, match="7 and 8 atoms"):
        metrics.torsion_pairs(F, _FakeCuda(torch.zeros(3, 8, 3)), pairs, quads)
    for bad in (torch.zeros(0, 2, dtype=torch.int64), torch.zeros(3, dtype=torch.int64), torch.zeros(3, 2)):
        with pytest.raises(ValueError, match="non-empty integer"):
            metrics.torsion_pairs(F, F, bad, quads)
    for bad in ([[0, 4]], [[4, 0]], [[-1, 0]]):
        with pytest.raises(ValueError, match="outside the pools"):
            metrics.torsion_pairs(F, F, torch.tensor(bad), quads)
    with pytest.raises(ValueError, match="model must be the dict"):
        metrics.dihedral_pca_project(F, dict(mean=None))
    with pytest.raises(ValueError, match="different names"):
        metrics.dihedral_quads(None, ("phi", "chi5"))
    with pytest.raises(ValueError, match="different names"):
        metrics.dihedral_quads(None, ("phi", "phi"))


def test_dihedral_quads_against_stereo_tables():
    pl = sr.planted(30, seed=4, chain_breaks=(11,))
    top, _ = sr.build_chain(**pl)
    sites = metrics.stereo_tables(top)[0]
    q = metrics.dihedral_quads(top)
    assert q is metrics.dihedral_quads(top, ["psi", "phi"])                       # cached on the topology, the order of a residue
    quads, res, col = q["quads"], q["residue"].tolist(), q["column"].tolist()
    assert quads.dtype == torch.int32 and tuple(quads.shape) == (56, 4) and int(quads.min()) >= 0       # 2 x 30 - 2 starts - 2 ends
    assert (0, 0) not in zip(res, col) and (11, 0) not in zip(res, col)          # no phi at a chain start
    assert (10, 1) not in zip(res, col) and (29, 1) not in zip(res, col)         # no psi at a chain end
    assert (10, 0) in zip(res, col) and (11, 1) in zip(res, col) and list(zip(res, col)) == sorted(zip(res, col))
    for t, (r, c) in enumerate(zip(res, col)):
        assert (quads[t] == sites[r, c]).all()
    assert (quads[res.index(5) + (col[res.index(5)] != 0)] == torch.tensor([top.atom(4, "C")] + [top.atom(5, a) for a in ("N", "CA", "C")])).all()
    chi = metrics.dihedral_quads(top, ("chi1", "chi2", "chi3", "chi4"))
    per_res = np.bincount(chi["residue"].numpy(), minlength=30)
    assert per_res.tolist() == [sr.N_CHI[nm] for nm in pl["seq"]] and set(chi["column"].tolist()) == {3, 4, 5, 6}
    everything = metrics.dihedral_quads(top, metrics.TORSION_NAMES)
    assert everything["quads"].shape[0] == int((sites[:, :7] >= 0).all(-1).sum()) == 56 + 28 + per_res.sum()


def test_the_restatement_lies_within_the_feature_bound_of_longdouble_on_every_device_case():
    worst = 0.0
    for N, T in tr.CASES:
        c = tr.case(N, T)
        ref, bound = tr.features_ld(c["x"], c["quads"])
        f = float((np.abs(c["F"].astype(LD) - ref) / bound).max())
        worst = max(worst, f)
        assert f <= 1.0, (N, T, f)
        assert np.abs((c["F"].reshape(N, T, 2) ** 2).sum(-1) - 1.0).max() <= 4 * tr.EPS       # unit vectors
    print(f"largest fraction of the feature bound: {worst:.4f}")
    # a nearly collinear quad: the bound says it is ill-conditioned, and still holds
    x = np.array([[[0, 0, 0], [1, 1, 1], [2 + 1e-4, 2, 2], [3 + 1e-4, 3 + 1e-4, 3]]], dtype=np.float32)
    ref, bound = tr.features_ld(x, tr.chain_quads(1))
    got, ok = tr.features64(x, tr.chain_quads(1))
    assert ok.all() and float(bound.max()) > 1e3 * tr.EPS and (np.abs(got.astype(LD) - ref) <= bound).all()
    # collinear: no angle
    x = np.array([[[0, 0, 0], [1, 0, 0], [2, 0, 0], [3, 0, 1]], [[0, 0, 0], [1, 0, 0], [1, 1, 0], [1, 1, 1]]], dtype=np.float32)
    got, ok = tr.features64(x, tr.chain_quads(1))
    assert ok.tolist() == [False, True] and np.isnan(got[0]).all() and (got[1] == [0.0, 1.0]).all()      # x, y, z steps: +90 degrees, IUPAC


def test_planted_angles_come_back():
    for n_states in (2, 3):
        p = tr.planted(n_states)
        q = metrics.dihedral_quads(p["top"])
        F, ok = tr.features64(p["x"], q["quads"].numpy())
        assert ok.all()
        ang = np.stack([(p["phi"] if c == 0 else p["psi"])[:, r] for r, c in zip(q["residue"].tolist(), q["column"].tolist())], 1)
        want = tr.angles_to_features(ang).reshape(F.shape)
        ref, bound = tr.features_ld(p["x"], q["quads"].numpy())
        f = float((np.abs(F.astype(LD) - ref) / bound).max())
        print(f"planted {n_states} states: largest fraction of the feature bound: {f:.4f}")
        assert f <= 1.0
        # the builder's own error: its float64 coordinates are rounded to fp32, every atom moves by at most sqrt(3) 2^-24
        # max|x|, which turns a torsion by at most that over the atom's distance from the axis (at least 1.2 A: the shortest
        # bond times the sine of the widest angle) - the two inner atoms count twice
        builder = 6 * np.sqrt(3.0) * 2.0 ** -24 * float(np.abs(p["x"]).max()) / 1.2
        gap = float(np.abs(F.astype(LD) - want).max())
        print(f"planted {n_states} states: |features - planted| {gap:.2e}, allowed {builder + float(bound.max()):.2e}")
        assert gap <= builder + float(bound.max())


def test_answers_by_hand():
    T = 7
    ang = np.linspace(-170.0, 160.0, T)
    one = tr.angles_to_features(ang).reshape(-1).astype(np.float64)
    same = np.tile(one, (5, 1))
    mean, _, W = tr.mean_ld(same, np.ones(5, bool))
    R = np.sqrt(mean[0::2] ** 2 + mean[1::2] ** 2)
    assert float(W) == 5.0 and np.abs(R - 1).max() <= 4 * tr.EPS                                  # all equal: R = 1
    flipped = tr.angles_to_features(ang + 180.0).reshape(-1).astype(np.float64)
    mean, _, _ = tr.mean_ld(np.stack([one, flipped]), np.ones(2, bool))
    assert np.abs(mean).max() <= 4 * tr.EPS                                                      # theta and theta + 180: R = 0
    mean, _, W = tr.mean_ld(np.stack([one, flipped, flipped]), np.ones(3, bool), np.array([2.0, 1.0, 1.0]))
    assert float(W) == 4.0 and np.abs(mean).max() <= 4 * tr.EPS
    mean, _, _ = tr.mean_ld(np.stack([one, flipped]), np.array([True, False]))
    assert np.abs(mean - one).max() == 0                                                         # a structure that is not finite takes no part
    other = ang.copy()
    other[3] += 180.0
    b = tr.angles_to_features(other).reshape(-1).astype(np.float64)
    tmsd, scale = tr.tmsd_cross(np.stack([one, b]), np.stack([one, b]))
    assert abs(float(tmsd[0, 1]) - 4.0 / T) <= 8 * tr.EPS and float(tmsd[0, 0]) == 0 and float(tmsd[0, 1]) == float(tmsd[1, 0])
    assert abs(float(scale[0, 1]) - (2 * T + 2 * (T - 2)) / T) <= 8 * tr.EPS                     # G = T, C = T - 2
    far = tr.angles_to_features(ang + 180.0).reshape(-1).astype(np.float64)
    assert abs(float(tr.tmsd_cross(one[None], far[None])[0][0, 0]) - 4.0) <= 16 * tr.EPS          # the largest distance is 2


@pytest.mark.parametrize("N,T", tr.BITMAP_CASES)
def test_the_cut_offs_of_the_bitmap_cases_leave_no_pair_undecided(N, T):
    c = tr.case(N, T)
    cutoff = tr.cutoff_of(c)
    cut2 = cutoff * cutoff
    iu = np.triu_indices(N, 1)
    v = np.sort(c["tmsd"][iu])
    k = int(np.searchsorted(v, LD(cut2)))
    assert 0 < k < v.size and v[k - 1] < cut2 < v[k]
    lim = float((LD(tr.matrix_bound(T)) * c["scale"][iu]).max())
    assert float(v[k] - v[k - 1]) > 2 * lim and abs(cut2 - 0.5 * float(v[k - 1] + v[k])) <= 4 * tr.EPS * cut2      # the midpoint of the gap
    assert not tr.undecided(c, cut2)[~np.eye(N, dtype=bool)].any()
    assert 0.2 < k / v.size < 0.8                                                                # both decisions occur


def test_the_planted_pools_separate_in_torsion_space_whatever_the_orientation():
    for n_states in (2, 3):
        p = tr.planted(n_states)
        q = metrics.dihedral_quads(p["top"])["quads"].numpy()
        F, _ = tr.features64(p["x"], q)
        d = np.sqrt(tr.tmsd_cross(F, F)[0].astype(np.float64))
        same = p["state"][:, None] == p["state"][None, :]
        assert d[same].max() < 0.25 < 0.9 < d[~same].min()                                       # cluster_torsion's cut-off is 0.5
        assert sorted(np.bincount(p["state"]).tolist()) == ([20, 20] if n_states == 2 else [13, 13, 14])
