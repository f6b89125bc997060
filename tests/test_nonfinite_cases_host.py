"""CPU: the cases and restatements of tests/nonfinite_cases.py are what they claim.

The k-NN rule of features_kernel BEFORE the total order, restated, leaves neighbour slots unwritten on the planted traces
(the table below is the emulation that found the fault; the device stored those slots into E_idx all the same).  The total
order is a permutation on every case and the parent rule on every clean one, so finite input cannot tell them apart."""
import numpy as np
import pytest

from tests import nonfinite_cases as nc
from tests import test_geometry_check as tg


def _planted(L, bad):
    return nc.plant(nc.ca_trace(L), 7, bad, "y")


# L: (nodes with an unwritten slot | slots at node 7) for a NaN at residue 7's y, slots at node 7 for +inf there
PARENT_TABLE = {46: ("all", 45, 1), 64: ("all", 63, 1), 65: ("node7", 63, 0), 87: ("node7", 63, 0)}


@pytest.mark.parametrize("L", sorted(PARENT_TABLE))
def test_parent_rank_rule_leaves_slots_unwritten(L):
    who, at7, at7_inf = PARENT_TABLE[L]
    miss = nc.unwritten(nc.knn_rows(_planted(L, "nan"), nc.parent_ranks))
    assert miss[7] == at7
    others = np.delete(miss, 7)
    assert (others == 1).all() if who == "all" else (others == 0).all()
    # +inf: the self distance of residue 7 is inf - inf = NaN and takes rank 0 beside the first inf
    miss = nc.unwritten(nc.knn_rows(_planted(L, "+inf"), nc.parent_ranks))
    assert miss[7] == at7_inf and (np.delete(miss, 7) == 0).all()
    assert not nc.unwritten(nc.knn_rows(nc.ca_trace(L), nc.parent_ranks)).any()


@pytest.mark.parametrize("L", nc.KNN_LENGTHS)
def test_total_order_is_a_permutation_and_the_parent_rule_on_clean_input(L):
    x = nc.ca_trace(L)
    for i in range(L):
        d = nc.distance_row(x, i)
        assert np.isfinite(d).all() and np.array_equal(nc.total_ranks(d), nc.parent_ranks(d))
    K = min(nc.KNN, L)
    seen_parent_fault = False
    for label, row, xb in nc.knn_cases(L):
        assert nc.bad_rows(xb).tolist() == [row], label
        rows = nc.knn_rows(xb)
        for i in range(L):
            r = nc.total_ranks(nc.distance_row(xb, i))
            assert sorted(r.tolist()) == list(range(L)), (label, i)
        assert rows.shape == (L, K) and (rows >= 0).all() and (rows < L).all(), label
        assert all(len(set(r.tolist())) == K for r in rows), label
        seen_parent_fault |= bool(nc.unwritten(nc.knn_rows(xb, nc.parent_ranks)).any())
        # a NaN distance sorts last: where K = L the bad residue closes the row of every other node, and at the bad node
        # itself, where every distance is NaN, the row is the index order
        if label.startswith("nan") and L <= nc.KNN:
            assert (np.delete(rows[:, -1], row) == row).all() and rows[row].tolist() == list(range(L)), label
    assert seen_parent_fault                              # each length shows the fault the total order removes


def test_total_order_on_hand_made_rows():
    nan, inf = nc.NAN, nc.INF
    f = lambda *v: np.array(v, dtype=np.float32)                                  # noqa: E731
    assert nc.total_ranks(f(2, nan, 1, 1, inf, nan, 0)).tolist() == [3, 5, 1, 2, 4, 6, 0]
    assert nc.parent_ranks(f(2, nan, 1, 1, inf, nan, 0)).tolist() == [3, 0, 1, 2, 4, 0, 0]
    assert nc.total_ranks(f(nan, nan, nan)).tolist() == [0, 1, 2]
    assert nc.neighbour_row(np.array([3, 0, 1, 2, 4, 0, 0]), 4).tolist() == [6, 2, 3, 0]
    assert nc.neighbour_row(np.array([0, 0, 0]), 3).tolist() == [2, -1, -1]


def test_edge_reader_set():
    L = 10
    assert nc.readers(0, 9, L) == {0, 1, 8, 9} and nc.readers(4, 5, L) == {3, 4, 5, 6}
    for bad in (0, 5, 9):
        unread = {(i, j) for i in range(L) for j in range(L) if nc.unread_edge(i, j, L, [bad])}
        want = {(i, j) for i in range(L) for j in range(L) if abs(i - bad) > 1 and abs(j - bad) > 1}
        assert unread == want and len(want) > 0
    # the claim behind it, on the distance the edge carries: an edge no bad residue reads keeps its distance bits
    for label, row, xb in nc.knn_cases(46):
        x = nc.ca_trace(46)
        for i in range(46):
            same = nc.distance_row(xb, i).view(np.int32) == nc.distance_row(x, i).view(np.int32)
            assert all(same[j] for j in range(46) if nc.unread_edge(i, j, 46, [row])), (label, i)


def test_plants_cover_what_they_claim():
    assert len(nc.PLANTS) == 18 and len(set(nc.PLANTS)) == 18
    x = np.zeros((7, 3), dtype=np.float32)
    assert [nc.position(7, p) for p in nc.POSITIONS] == [0, 3, 6]
    y = nc.plant(x, 3, "-inf", "y")
    assert np.isneginf(y[3, 1]) and np.isfinite(np.delete(y.reshape(-1), 10)).all() and not x.any()
    assert np.isnan(nc.plant(x, 6, "nan", "xyz")[6]).all()
    assert nc.geometry_rows(4) == [0, 3] and nc.geometry_rows(1025) == [0, 1024] and nc.geometry_rows(257) == [0, 256]


@pytest.mark.parametrize("n", nc.GEOMETRY_SIZES)
def test_geometry_restatement(n):
    radius, bonds, xyz, refs = tg.case(n)
    for s in range(3):                                   # clean: the reference of test_geometry_check, to the count
        counts, dmin, valid = nc.geometry_reference(xyz[s], radius, bonds)
        assert counts == refs[s][0] and dmin == refs[s][1] and valid == (counts[0] == 0 and counts[1] == 0)
    n_touching = lambda row: int(((bonds[:, 0] == row) | (bonds[:, 1] == row)).sum())        # noqa: E731
    for label, row, batch in nc.geometry_cases(n):
        assert np.array_equal(batch[0], xyz[0]) and np.array_equal(batch[2], xyz[2])
        counts, dmin, valid = nc.geometry_reference(batch[1], radius, bonds)
        assert np.isnan(dmin) and not valid, label
        assert counts[2] == len(bonds) - counts[0] + counts[1], label
        # every template bond of the bad atom is broken, whether its distance is NaN or inf
        rest = np.delete(np.arange(n), row)
        keep = np.isin(bonds, rest).all(1)
        remap = np.full(n, -1)
        remap[rest] = np.arange(n - 1)
        sub = nc.geometry_reference(xyz[1][rest], radius[rest], remap[bonds[keep]])[0]
        assert counts[0] == sub[0] + n_touching(row), label
