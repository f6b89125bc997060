"""CPU checks of the dRMSD feature: the C ABI of codlad_drmsd_matrix and codlad_drmsd_pairs (declared once, exported,
counted in _SIGS, bad arguments refused before any HIP call, the split rule on both sides of its thresholds), the
kernels' registers, what the Python layer refuses, the references of tests/drmsd_ref.py against answers derived by hand,
and that the cut-offs of the bitmap cases leave no pair undecided."""
import json
import os
import re

import numpy as np
import pytest
import torch

from codlad_amd import _lib, build, metrics
from tests import drmsd_ref as dr
from tests.test_cluster_host import _FakeCuda

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = (("int", "codlad_drmsd_groups", 4), ("long long", "codlad_drmsd_matrix_scratch_bytes", 4),
                ("int", "codlad_drmsd_matrix", 16), ("int", "codlad_drmsd_pairs", 13))
KERNELS = ("finite_kernel", "gram_kernelILi0", "gram_kernelILi1", "gram_kernelILi2", "norm_finish_kernel", "finish_kernelILi1",
           "finish_kernelILi2", "pairs_kernel")


def test_header_declares_and_library_exports_the_entry_points():
    header = open(os.path.join(ROOT, "include", "codlad_hip.h")).read()
    lib = _lib.lib()
    for res, name, n_args in ENTRY_POINTS:
        decl = re.findall(r"\b" + res + r"\s+" + name + r"\s*\(([^;]*)\)\s*;", header)
        assert len(decl) == 1, name
        assert name in _lib.exported_symbols() and hasattr(lib, name)
        assert len(_lib._SIGS[name][1]) == decl[0].count(",") + 1 == n_args, name
    for macro, value, mine in (("MAX_SEL", 8192, _lib.DRMSD_MAX_SEL), ("WINDOW", 16, _lib.DRMSD_WINDOW),
                               ("SLAB_TILES", 64, _lib.DRMSD_SLAB_TILES), ("SPLIT_MAX_BLOCKS", 256, _lib.DRMSD_SPLIT_MAX_BLOCKS)):
        assert f"#define CODLAD_DRMSD_{macro} {value}\n" in header and mine == value == dr.macro(macro)
    assert dr.SCRATCH_BUDGET == 256 << 20 and metrics.DRMSD_MAX_SEL == dr.MAX_SEL >= 4325 and dr.MAX_SEL == _lib.POLYMER_MAX_SEL
    for name, expr in (("MATRIX_BOUND(P)", "((P) + 3.0)"), ("PAIRS_BOUND(m)", "(((m) + 63) / 64 + ((m) + 3) / 4 + 12.0)"),
                       ("POSITION_BOUND(m)", "(((m) + 63) / 64 + 9.0)")):
        assert f"#define CODLAD_DRMSD_{name} ({expr} * 2.220446049250313e-16)\n" in header
    assert dr.matrix_bound(8256) == 8259 * dr.EPS and dr.pairs_bound(129) == (3 + 33 + 12) * dr.EPS
    assert dr.position_bound(129) == 12 * dr.EPS and dr.EPS == 2.0 ** -52
    assert "#define CODLAD_ABI_VERSION 19\n" in header and _lib.ABI_VERSION == 19 and lib.codlad_abi_version() == 19
    assert "drmsd_kernels.hip" in build.SOURCES and build.EXTRA_FLAGS["drmsd_kernels.hip"] == ["-ffp-contract=off"]
    for name in ("drmsd_matrix", "drmsd_neighbours", "drmsd_pairs", "cluster_drmsd"):
        assert callable(getattr(metrics, name)) and name in metrics.drmsd.__all__


def test_drmsd_kernels_use_no_scratch_and_spill_nothing():
    build.build(force=False, verbose=False)
    if not os.path.exists(build.RESOURCES):
        build.build(force=True, verbose=False)
    with open(build.RESOURCES) as f:
        table = json.load(f)
    mine = {k: v for k, v in table.items() if v.get("source") == "drmsd_kernels.hip"}
    for kernel in KERNELS:
        assert any(kernel in k for k in mine), (kernel, sorted(mine))
    assert len(mine) == len(KERNELS), sorted(mine)
    for name, r in mine.items():
        assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0, (name, r)


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

    #     x  Na y     Nb n_atoms sel n_sel min_sep cut2 squared msd bits fx fy    scratch stream
    ok = [p, 4, None, 0, 87, None, 0, 1, 1.0, 0, p, p, p, None, p, None]
    refuses("codlad_drmsd_matrix", ok, [(k, None) for k in (0, 12, 14)] +
            [(1, 0), (1, -1), (1, 65537), (3, 5), (3, -1), (4, 0), (4, -1), (4, 1), (4, dr.MAX_SEL + 1), (6, 3), (6, -1),
             (7, 0), (7, -1), (7, 87), (7, 88), (8, -1.0), (8, float("inf")), (8, float("nan")), (13, p)])
    args = list(ok)
    args[10] = args[11] = None                           # neither the table nor the bitmap
    assert lib.codlad_drmsd_matrix(*args) < 0 and b"neither" in lib.codlad_last_error()
    args = list(ok)
    args[5] = p                                          # sel without n_sel
    assert lib.codlad_drmsd_matrix(*args) < 0 and b"disagree" in lib.codlad_last_error()
    for n_sel, what in ((1, b"m outside"), (dr.MAX_SEL + 1, b"m outside"), (5, b"min_sep")):
        args[6], args[7] = n_sel, (5 if n_sel == 5 else 1)      # one atom has no pair; one more than the limit; min_sep = m
        assert lib.codlad_drmsd_matrix(*args) < 0 and what in lib.codlad_last_error()
    cross = list(ok)
    cross[2], cross[3], cross[13] = p, 3, p              # cross mode takes no bitmap, and wants y, Nb and finite_y together
    assert lib.codlad_drmsd_matrix(*cross) < 0 and b"cross" in lib.codlad_last_error()
    cross[11] = None
    refuses("codlad_drmsd_matrix", cross, [(2, None), (3, 0), (13, None)])
    #     a  na b  nb n_atoms sel n_sel min_sep pairs K msd position stream
    ok = [p, 4, p, 3, 87, None, 0, 1, p, 2, p, None, None]
    refuses("codlad_drmsd_pairs", ok, [(k, None) for k in (0, 2, 8, 10)] +
            [(1, 0), (3, 0), (3, -1), (4, 0), (4, 1), (4, dr.MAX_SEL + 1), (6, 3), (7, 0), (7, 87), (9, 0), (9, -1)])
    args = list(ok)
    args[5] = p
    assert lib.codlad_drmsd_pairs(*args) < 0 and b"disagree" in lib.codlad_last_error()
    for fn in ("codlad_drmsd_groups", "codlad_drmsd_matrix_scratch_bytes"):
        for bad in ((0, 0, 87, 1), (-1, 0, 87, 1), (65537, 0, 87, 1), (4, -1, 87, 1), (4, 0, 1, 1), (4, 0, dr.MAX_SEL + 1, 1),
                    (4, 0, 87, 0), (4, 0, 87, 87)):
            assert getattr(lib, fn)(*bad) < 0 and fn.encode() in lib.codlad_last_error(), (fn, bad)


def test_the_split_rule_stands_on_both_sides_of_its_thresholds():
    lib = _lib.lib()
    groups, nbytes = lib.codlad_drmsd_groups, lib.codlad_drmsd_matrix_scratch_bytes
    m1 = 161                                             # 11 rows of windows, 66 windows: the first size with two slabs
    assert dr.n_slabs(m1 - 1) == 1 and dr.n_slabs(m1) == 2 and (m1 - 1) % dr.WINDOW == 0
    assert groups(2, 0, m1 - 1, 1) == 1 and groups(2, 0, m1, 1) == 2 == groups(2, 0, m1, m1 - 1)
    # few blocks: a workgroup per slab; SPLIT_MAX_BLOCKS blocks or more: a workgroup per block
    assert groups(32, 0, 4325, 1) == dr.n_slabs(4325) == 576 and groups(2, 0, 1100, 1) == groups(2, 0, 1100, 3) == 38
    n_lo, n_hi = 64 * 22, 64 * 22 + 1                    # 253 and 276 blocks of one pool
    assert dr.n_blocks(n_lo) == 253 < dr.SPLIT_MAX_BLOCKS <= dr.n_blocks(n_hi) == 276
    assert groups(n_lo, 0, m1, 1) == 2 and groups(n_hi, 0, m1, 1) == 1
    assert groups(64 * 15, 64 * 17, m1, 1) == 2 and groups(64 * 16, 64 * 16, m1, 1) == 1       # 255 and 256 blocks, cross
    # the budget: 8192 partial blocks of 32 KiB
    assert dr.n_blocks(64 * 5) * 576 > 8192 >= dr.n_blocks(64 * 4) * 576
    assert groups(64 * 5, 0, 4325, 1) == 1 and groups(64 * 4, 0, 4325, 1) == 576
    for case in ((400, 0, 87), (4096, 0, 129), (16384, 0, 129), (4096, 0, 1075), (32, 0, 4325), (65, 3, 87), (3, 130, 1100), (2, 0, 2)):
        assert groups(*case, 1) == dr.groups(*case), case
    # the scratch: G of every padded structure, and with the split the partial norms and blocks
    assert nbytes(130, 0, 87, 1) == 8 * 192 and nbytes(65, 3, 87, 1) == 8 * (128 + 64)
    assert nbytes(2, 0, 1100, 1) == 8 * 64 + 256 * ((8 * 38 * 64 + 255) // 256) + 8 * 38 * 4096
    assert nbytes(32, 0, 4325, 1) == 8 * 64 + 8 * 576 * 64 + 8 * 576 * 4096


def test_python_layer_refuses_what_it_cannot_run():
    x = torch.zeros(4, 5, 3)
    F = _FakeCuda(x)
    pairs = torch.tensor([[0, 1]])
    calls = (lambda x, **kw: metrics.drmsd_matrix(x, **kw), lambda x, **kw: metrics.drmsd_neighbours(x, 1.0, **kw),
             lambda x, **kw: metrics.drmsd_pairs(x, F, pairs, **kw), lambda x, **kw: metrics.cluster_drmsd(x, 1.0, **kw))
    for call in calls:
        with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
            call(x)
        with pytest.raises(ValueError, match="non-empty"):
            call(_FakeCuda(torch.zeros(4, 5)))
        with pytest.raises(ValueError, match="outside"):
            call(F, sel=[0, 5])
        with pytest.raises(ValueError, match="sel is empty"):
            call(F, sel=[])
        with pytest.raises(ValueError, match="names an atom twice"):
            call(F, sel=[0, 2, 2])
        with pytest.raises(ValueError, match=f"2 .. {dr.MAX_SEL} selected atoms, got {dr.MAX_SEL + 1}"):
            call(_FakeCuda(torch.zeros(2, dr.MAX_SEL + 1, 3)))
        with pytest.raises(ValueError, match=f"2 .. {dr.MAX_SEL} selected atoms, got 1"):
            call(F, sel=[3])
        for bad in (0, 5, -1, 1.0, True):                # 1 .. m - 1 = 4
            with pytest.raises(ValueError, match="min_sep must be an integer in 1 .. 4"):
                call(F, min_sep=bad)
    for call in (metrics.drmsd_neighbours, metrics.cluster_drmsd):
        for bad in (0.0, -1.0, float("nan"), float("inf"), "x"):
            with pytest.raises(ValueError, match="cutoff must be a positive finite number"):
                call(F, bad)
    big = _FakeCuda(torch.zeros(1, 1, 3).expand(65537, 5, 3))
    for call in (metrics.drmsd_matrix, lambda x: metrics.drmsd_neighbours(x, 1.0), lambda x: metrics.cluster_drmsd(x, 1.0)):
        with pytest.raises(ValueError, match="at most 65536 structures"):
            call(big)
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        metrics.drmsd_matrix(F, y=x)
    with pytest.raises(ValueError, match="5 and 6 atoms"):
        metrics.drmsd_matrix(F, y=_FakeCuda(torch.zeros(3, 6, 3)))
    with pytest.raises(ValueError, match="5 and 6 atoms"):
        metrics.drmsd_pairs(F, _FakeCuda(torch.zeros(3, 6, 3)), pairs)
    for bad in (torch.zeros(0, 2, dtype=torch.int64), torch.zeros(3, dtype=torch.int64), torch.zeros(3, 2)):
        with pytest.raises(ValueError, match="non-empty integer"):
            metrics.drmsd_pairs(F, F, bad)
    for bad in ([[0, 4]], [[4, 0]], [[-1, 0]]):
        with pytest.raises(ValueError, match="outside the pools"):
            metrics.drmsd_pairs(F, F, torch.tensor(bad))
    for bad, msg in (([1.0] * 3, "one value per structure"), ([1.0, -1.0, 1.0, 1.0], "finite and >= 0")):
        with pytest.raises(ValueError, match=msg):
            metrics.cluster_drmsd(F, 1.0, weights=bad)


def test_the_pair_order_meets_every_pair_once():
    for m, min_sep in ((2, 1), (5, 2), (17, 1), (33, 3), (87, 86), (200, 1)):
        pairs, slabs = dr.pair_order(m, min_sep)
        want = {(k, l) for k in range(m) for l in range(k + min_sep, m)}
        assert len(pairs) == len(want) == dr.n_pairs(m, min_sep) and set(pairs) == want
        assert slabs == sorted(slabs) and (not slabs or slabs[-1] < dr.n_slabs(m))
    # the first window of a row of windows is the diagonal one; the order does not know N
    pairs, slabs = dr.pair_order(33, 1)
    assert pairs[:3] == [(0, 1), (0, 2), (0, 3)] and pairs[15] == (1, 2) and pairs[120] == (0, 16) and pairs[-1] == (31, 32)
    assert set(dr.pair_order(200, 1)[1]) == {0, 1}


def test_the_reference_by_hand_rods_mirror_and_translate():
    for m, min_sep in ((2, 1), (3, 1), (17, 1), (17, 3), (129, 2)):
        D = dr.distances(dr.rods(m), None, min_sep)
        msd, scale = dr.msd_cross(D, D)
        want = dr.rods_msd(m, min_sep)
        assert (np.abs(msd - want) <= 2 * dr.EPS * want).all() and (np.diag(msd) == 0).all()      # want is rounded to float64
        assert abs(scale[0, 1] - 9 * want[0, 1]) <= 4 * dr.EPS * float(scale[0, 1])                # sum (s + 2 s)^2 / P
    assert dr.rods_msd(2)[0, 1] == 1.0 and dr.rods_msd(3)[0, 2] == 4.0 * (2 * 1 + 1 * 4) / 3
    c = dr.case(3, 65)
    D = c["D"]
    assert (dr.distances(dr.mirrored(c["x"])) == D).all()
    q, moved = dr.translated(c["x"])
    assert (moved != q).any() and (dr.distances(moved) == dr.distances(q)).all()
    msd, _ = dr.msd_cross(dr.distances(q), dr.distances(moved))
    assert (np.diag(msd) == 0).all() and msd[0, 1] > 0
    # the direct sum against the pair loop of the kernel's order, and against per-position means
    x = c["x"]
    pairs, _ = dr.pair_order(65, 2)
    ta, tb = dr.table32(x[0]), dr.table32(x[1])
    by_loop = sum((dr.LD(ta[k, l]) - dr.LD(tb[k, l])) ** 2 for k, l in pairs) / dr.LD(len(pairs))
    direct = dr.msd_cross(dr.distances(x[:1], None, 2), dr.distances(x[1:2], None, 2))[0][0, 0]
    assert abs(by_loop - direct) <= 1e-15 * float(direct)
    pos = dr.position_ld(ta, tb, 65, 2)
    partners = np.array([max(0, k - 1) + max(0, 65 - k - 2) for k in range(65)])
    assert abs((pos * partners).sum() / 2 / len(pairs) - direct) <= 1e-15 * float(direct)
    # a selection, and a structure that is not finite
    s = dr.case(3, 33, 1, "subset")
    assert (dr.distances(s["x"], s["sel"]) == dr.distances(np.ascontiguousarray(s["x"][:, s["sel"]]))).all()
    bad = c["x"].copy()
    bad[1, 7, 0] = np.inf
    f = dr.finite_of(bad)
    msd, scale = dr.msd_cross(dr.distances(bad), dr.distances(bad), f, f)
    assert f.tolist() == [True, False, True] and np.isnan(msd[1]).all() and np.isnan(msd[:, 1]).all() and msd[0, 2] == c["msd"][0, 2]


@pytest.mark.parametrize("N,m,min_sep", dr.BITMAP_CASES)
def test_the_cut_offs_of_the_bitmap_cases_leave_no_pair_undecided(N, m, min_sep):
    c = dr.case(N, m, min_sep)
    cutoff = dr.cutoff_of(c)
    cut2 = cutoff * cutoff
    und = dr.undecided(c, cut2)
    assert not und[~np.eye(N, dtype=bool)].any()
    inside = (c["msd"] <= cut2)[np.triu_indices(N, 1)]
    assert 0.4 <= inside.mean() <= 0.6                   # a cut-off that splits the pairs, not one that all pass or fail


def test_the_planted_pool_is_three_conformations_whatever_their_orientation():
    from tests import cluster_ref as cr
    for rotate in (False, True):
        x, member = dr.planted(rotate=rotate)
        D = dr.distances(x)
        msd, scale = dr.msd_cross(D, D)
        same = member[:, None] == member[None, :]
        cut = 1.0                                        # A: copies differ by noise of 0.01 A, conformations by many A
        assert float(np.sqrt(msd[same].max())) < 0.1 < 3.0 < float(np.sqrt(msd[~same].min()))
        assert not (np.abs(msd - cut * cut) <= dr.matrix_bound(D.shape[1]) * scale).any()
        out = cr.daura(msd <= cut * cut)
        assert out["n_clusters"] == 3 and sorted(out["sizes"].tolist()) == [5, 7, 9]
        for k in range(3):
            assert len(set(member[out["labels"] == k])) == 1
