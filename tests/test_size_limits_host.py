"""What tests/test_size_limits.py rests on, held on the CPU: the closed forms and generators of the cases at the limits
include/codlad_hip.h declares against the existing small references, the caps on the undecided pairs of the DSSP inputs,
and the refusals one past every limit through the C ABI (an argument error returns before any HIP call)."""
import numpy as np
import pytest

from codlad_amd import _lib
from tests import cluster_ref as cr
from tests import dssp_ref as dr
from tests import pair_hist_ref as pr

UNDECIDED_CAP = 1e-4                                                 # tests/test_dssp.py's
# the planted row of the R = 4096 call (seed 1) has 9 undecided pairs and one undecided kappa, and seeds 1 .. 8 all leave
# 1 .. 6 undecided pairs in the planted structure taken alone: at this size the call is held on its decided pairs only
PLANTED_DECIDED = {257: True, 1025: True, 4096: False}


# --------------------------------------------------------------------------------------------------------------- DSSP
@pytest.mark.parametrize("R", (130, 200, 257))
def test_the_sparse_bridge_loop_equals_the_full_loop(R):
    maps = ([dr.handmade(R)[:3]] if R in (130, 200) else []) + [dr.random_maps(R, seed) for seed in (1, 2, 3)]
    found = 0
    for hb, link, bend in maps:
        full, quick = dr.assign(hb, link, bend), dr.assign(hb, link, bend, sparse=True)
        assert all(np.array_equal(a, b) for a, b in zip(full, quick))
        found += int((full[1] >= 0).sum())
    assert found > 20                                                # the maps have bridges to lose


@pytest.mark.parametrize("kind", dr.HIGH_KINDS)
def test_hand_written_maps_at_high_word_indices_have_the_hand_derived_labels(kind):
    R = dr.MAX_RES
    hb, link, bend, checks = dr.handmade_high(R, kind)
    ss, bridge, counts = dr.assign(hb, link, bend, sparse=True)
    got = dr.labels(ss)
    assert {r: got[r] for r in checks} == checks
    assert int(counts.sum()) == R and counts[dr.E] == 24 and counts[dr.B] == 0
    b_anti, b_par = (4032, 256) if kind == "a" else (1280, 4032)
    assert bridge[10:17, 1].tolist() == [b_anti + 2 - k for k in range(7)] and (bridge[10:17, 0] == -1).all()
    assert bridge[20:25, 0].tolist() == [b_par - 4 + k for k in range(5)] and (bridge[20:25, 1] == -1).all()
    assert bridge[b_anti - 4:b_anti + 3, 1].tolist() == [16 - k for k in range(7)]
    assert bridge[b_par - 4:b_par + 1, 0].tolist() == [20 + k for k in range(5)]
    # what the cases are there for: partners on both sides of a word border, runs on both sides of a trip border
    assert {(b_anti - 4) >> 6, (b_anti + 2) >> 6} == {b_anti // 64 - 1, b_anti // 64}
    assert {(b_par - 4) >> 6, b_par >> 6} == {b_par // 64 - 1, b_par // 64}
    for code, lo in (("G", 511), ("H", 1023 if kind == "a" else 255)):
        assert got[lo] == got[lo + 1] == code


@pytest.mark.parametrize("R", tuple(dr.LIMIT_SIZES))
def test_the_sized_inputs_beyond_one_trip_hold_the_cap_on_undecided_pairs(R):
    top, xyz, m = dr.limit_call(R)
    assert top.n_residues == R and xyz.shape[0] == 1 + dr.LIMIT_SIZES[R]
    undecided, eligible = int(m["undecided_e"].sum()), int(m["r64"]["eligible"].sum())
    planted = int(m["undecided_e"][0].sum()) + int(m["undecided_k"][0].sum()) + int(m["undecided_d"][0].sum())
    print(f"R={R} seed {dr.SIZED_SEED[R]}: undecided {undecided} of {eligible} eligible pairs, kappa {int(m['undecided_k'].sum())}, "
          f"links {int(m['undecided_d'].sum())}; in the planted row {planted}")
    assert undecided <= UNDECIDED_CAP * eligible
    assert (planted == 0) == PLANTED_DECIDED[R]
    assert m["r64"]["hb"].sum() > R                                  # helices all along the chain


def test_dssp_refuses_one_residue_too_many_before_any_hip_call():
    lib = _lib.lib()
    buf = np.zeros(64, dtype=np.float64)
    p = buf.ctypes.data                                              # 16-byte aligned or not, the size is refused first or second
    R = dr.MAX_RES + 1
    assert lib.codlad_dssp_hbonds(p, 1, 8, (p + 15) // 16 * 16, p, R, p, p, p, p, p, p, p, None) < 0
    assert b"codlad_dssp_hbonds: more than CODLAD_DSSP_MAX_RES residues" in lib.codlad_last_error()
    assert lib.codlad_dssp_assign(p, p, p, p, 1, R, p, p, p, None) < 0
    assert b"codlad_dssp_assign: more than CODLAD_DSSP_MAX_RES residues" in lib.codlad_last_error()


# ---------------------------------------------------------------------------------------------------------- clustering
@pytest.mark.parametrize("N,fill", ((129, False), (300, False), (300, True), (1000, True)))
def test_the_closed_form_of_disjoint_cliques_is_dauras_rule(N, fill):
    cliques = cr.limit_cliques(N, fill)
    members = cr.clique_members(cliques)
    assert sum(len(m) > 1 for m in members) > 10 and [0, 1, 2, N - 1] in members
    nb = cr.clique_matrix(N, cliques)
    assert not nb.diagonal().any() and np.array_equal(nb, nb.T)
    masks = [None]
    fin = np.ones(N, dtype=bool)
    fin[[0, 10, members[-1][0]]] = False              # the would-be centres of the first, the largest and the last clique
    masks.append(fin)
    for finite in masks:
        want, got = cr.daura(nb, finite), cr.clique_answer(N, cliques, finite)
        for k in ("labels", "centres", "sizes"):
            assert got[k].dtype == np.int32 and got[k].tolist() == want[k].tolist(), k
        assert got["n_clusters"] == want["n_clusters"] and got["rounds"] == int((want["sizes"] > 1).sum()) + 1
    masked = cr.clique_answer(N, cliques, fin)
    assert masked["labels"][10] == -1 and masked["centres"][masked["labels"][11]] == 11 and masked["sizes"][masked["labels"][11]] == 29
    # a clique given as a list, and a pool without a singleton: no closing launch
    got = cr.clique_answer(6, [[0, 5], (1, 4)])
    assert got["labels"].tolist() == [1, 0, 0, 0, 0, 1] and got["centres"].tolist() == [1, 0] and got["rounds"] == 2
    assert got["labels"].tolist() == cr.daura(cr.clique_matrix(6, [[0, 5], (1, 4)]))["labels"].tolist()


def test_the_limit_cliques_reach_the_words_they_are_there_for():
    filled = cr.clique_members(cr.limit_cliques(4097, fill=True))
    assert 90 < 4097 - sum(len(m) for m in filled) < 110 and sum(len(m) == 389 for m in filled) >= 9
    assert all(m[-1] // 64 - m[0] // 64 >= 6 for m in filled if len(m) == 389) and sum(len(m) > 1 for m in filled) > 64
    for N, borders in ((4097, (64, 4032, 4096)), (65536, (64, 4032, 4096, 4160, 32768, 65472))):
        members = cr.clique_members(cr.limit_cliques(N))
        flat = {i for m in members for i in m}
        assert [0, 1, 2, N - 1] in members                           # the last structure with members of word 0
        answer = cr.clique_answer(N, cr.limit_cliques(N))            # ... which wins its tie with the four of word 4
        assert [300, 301, 302, 303] in members and answer["labels"][300] == answer["labels"][0] + 1
        if N == 4097:
            borders = borders[:-1]                                   # word 64 holds that structure alone
        for b in borders:                                            # a run of consecutive structures on both sides of the border
            assert any(m[0] < b <= m[-1] and m[-1] - m[0] == len(m) - 1 for m in members), (N, b)
        assert sum(len(m) > 1 for m in members) > 64                 # a second batch of rounds
        W = (N + 63) // 64
        assert all(any(i not in flat for i in range(64 * w, min(64 * w + 64, N))) or w == W - 1 for w in range(W))
        assert N - len(flat) > 3000 or N < 5000                      # thousands of singletons, in every word


def test_clustering_refuses_one_structure_or_round_too_many_before_any_hip_call():
    lib = _lib.lib()
    buf = np.zeros(64, dtype=np.float64)
    p = buf.ctypes.data
    N = cr.MAX_N + 1
    assert lib.codlad_rmsd_matrix_scratch_bytes(N, 1) < 0 and b"codlad_rmsd_matrix_scratch_bytes" in lib.codlad_last_error()
    assert lib.codlad_cluster_scratch_bytes(N) < 0 and b"codlad_cluster_scratch_bytes" in lib.codlad_last_error()
    assert lib.codlad_rmsd_matrix_scratch_bytes(cr.MAX_N, 1) > 0 and lib.codlad_cluster_scratch_bytes(cr.MAX_N) == 16 * 1024 + 4 * cr.MAX_N
    assert lib.codlad_rmsd_matrix(p, p, N, 4, None, 0, 1.0, 0, p, p, p, p, None) < 0
    assert b"codlad_rmsd_matrix: bad sizes" in lib.codlad_last_error()
    assert lib.codlad_cluster_daura(p, None, N, 1, p, p, p, p, p, None) < 0
    assert b"codlad_cluster_daura: bad size" in lib.codlad_last_error()
    assert lib.codlad_cluster_daura(p, None, 8, _lib.CLUSTER_MAX_ROUNDS + 1, p, p, p, p, p, None) < 0
    assert b"rounds outside 0 .. CODLAD_CLUSTER_MAX_ROUNDS" in lib.codlad_last_error()
    assert lib.codlad_cluster_populations(p, p, N, 1, p, None) < 0


# ------------------------------------------------------------------------------------------------- SAXS, hydration, P(r)
def test_saxs_refuses_one_q_type_or_grid_point_too_many_before_any_hip_call():
    from tests import saxs_hydration_ref as hr
    from tests import saxs_ref as sr
    lib = _lib.lib()
    buf = np.zeros(64, dtype=np.float64)
    p = buf.ctypes.data
    for Q, T in ((sr.MAX_Q + 1, 1), (1, sr.MAX_TYPES + 1)):
        assert lib.codlad_saxs_debye(p, 1, 4, p, T, p, p, Q, p, p, None, p, None) < 0
        assert b"codlad_saxs_debye" in lib.codlad_last_error()
        assert lib.codlad_saxs_partials(p, 1, 4, p, T, p, p, p, p, Q, p, p, None, p, None) < 0
        assert b"codlad_saxs_partials" in lib.codlad_last_error()
    assert hr.MAX_GRID == 4096
    #                                  P  B  Q  f_w G  n_c1 c2 n_c2 I_exp sigma I_grid scale chi2 best I_best stream
    for n1, n2, Q in ((17, 241, 8), (1, hr.MAX_GRID + 1, 8), (hr.MAX_GRID + 1, 1, 8), (64, 64, sr.MAX_Q + 1)):
        assert lib.codlad_saxs_hydration_fit(p, 1, Q, p, p, n1, p, n2, p, p, p, p, p, p, p, None) < 0, (n1, n2, Q)
        assert b"codlad_saxs_hydration_fit" in lib.codlad_last_error()


def test_the_lattice_histogram_in_closed_form_is_the_float32_restatement():
    """300 atoms on a line: the closed form against pair_hist_ref.hist32 at every bin width the large case uses (scaled), then
    the fp32 sequence itself for every distance of the 65535-atom lattice."""
    n = 300
    x = pr.lattice(n)
    types = np.zeros(n, dtype=np.int32)
    for dr_, B in ((16, 19), (16, 4096), (16, 7), (1, 1), (1, 299), (1, 298), (4, 75), (4, 74)):
        H32, over32, d32 = pr.hist32(x, types, 1, float(dr_), B)
        H, over, d_bin = pr.lattice_hist(n, dr_, B)
        assert np.array_equal(H32[0, 0], H) and int(over32[0, 0]) == over and int(d32[0]) == d_bin, (dr_, B)
        assert int(H.sum()) + over == n * (n - 1) // 2
    # the two calls of the large case: every pair inside at dr = 16, every pair beyond the one bin at dr = 1
    n = pr.MAX_ATOMS
    pairs = n * (n - 1) // 2
    assert pairs == 2147385345 and 2 ** 31 - pairs == 98303
    H, over, d_bin = pr.lattice_hist(n, 16, pr.MAX_BINS)
    assert over == 0 and d_bin == 4095 and int(H.sum()) == pairs and int(H[0]) == sum(n - d for d in range(1, 16))
    assert int(H[1]) == sum(n - d for d in range(16, 32)) and int(H[4095]) == sum(n - d for d in range(65520, 65535)) == 120
    H, over, d_bin = pr.lattice_hist(n, 1, 1)
    assert int(H[0]) == 0 and over == pairs and d_bin == -1
    d = np.arange(1, n, dtype=np.float32)
    r = np.sqrt((d * d + np.float32(0) * np.float32(0)) + np.float32(0) * np.float32(0))
    assert r.dtype == np.float32 and np.array_equal(r, d)
    t = r * np.float32(1.0 / 16.0)
    assert np.array_equal(t.astype(np.int64), np.arange(1, n) // 16) and (t < np.float32(4096)).all()
    assert not (r * np.float32(1.0) < np.float32(1)).any()
