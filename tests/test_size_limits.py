"""The analysis kernels at the sizes include/codlad_hip.h declares: past the first trip of every strided loop, with the LDS
tables full, at word indices >= 64 and next to the int32 ceiling - and the refusal one past each limit.  Every case runs
the checker of its family (tests/test_dssp.py, test_cluster.py, test_reweight.py, test_saxs.py, test_saxs_hydration.py,
test_pair_hist.py) with that checker's bounds; no tolerance is introduced here.  Where an all-pairs reference is out of
reach the case is held to a closed form (tests/test_size_limits_host.py holds those to the small references) or to the
documented independence: an element depends on its pair alone, a problem or a structure not on the rest of the call.
DESIGN.md, "Declared limits", has the table of what is run where, and the measured times."""
import numpy as np
import pytest
import torch

from codlad_amd import _lib, metrics
from tests import cluster_ref as cr
from tests import dssp_ref as dr
from tests import ensemble_ref as er
from tests import pair_hist_ref as pr
from tests import reweight_ref as rr
from tests import saxs_hydration_ref as hr
from tests import saxs_ref as sr
from tests import test_cluster as tc
from tests import test_dssp as td
from tests import test_reweight as tr
from tests import test_saxs as ts
from tests import test_saxs_hydration as th
from tests.test_buffer_discipline import hold
from tests.test_saxs import dev

pytestmark = pytest.mark.gpu
p = _lib.ptr


def last_error():
    return _lib.lib().codlad_last_error().decode()


# --------------------------------------------------------------------------------------------------------------- DSSP
@pytest.mark.parametrize("R", tuple(dr.LIMIT_SIZES))
def test_dssp_stage1_against_float64_beyond_one_trip_and_at_the_limit(R):
    """test_dssp.check_stage1 at 257, 1025 and CODLAD_DSSP_MAX_RES residues.  At 4096 the planted row itself has undecided
    pairs (tests/test_size_limits_host.py): the call is held on its decided pairs, under the same cap."""
    top, xyz, m = dr.limit_call(R)
    out = td.host(metrics.hbonds(dev(xyz), top))
    assert out["acc"].shape == (xyz.shape[0], R, (R + 63) // 64) and out["acc"].dtype == np.int64
    undecided, eligible = td.check_stage1(out, m, R, planted_rows=[0] if R < dr.MAX_RES else [])
    assert undecided <= td.UNDECIDED_CAP * eligible


@pytest.mark.parametrize("R", tuple(dr.LIMIT_SIZES))
def test_dssp_stage2_equals_the_loops_on_the_devices_own_bitmaps(R):
    top, xyz, _m = dr.limit_call(R)
    out = td.host(metrics.dssp(dev(xyz), top))
    hb = dr.unpack_bits(td.words(out["acc"]), R)
    ss, bridge, counts = dr.assign_batch(hb, out["geom"], out["finite"], sparse=True)
    assert np.array_equal(out["ss"], ss) and np.array_equal(out["bridge"], bridge) and np.array_equal(out["counts"], counts)
    assert (out["counts"].sum(1) == R).all() and counts[0, [dr.H, dr.G, dr.I]].sum() > R // 2
    print(f"R={R}: counts of the planted structure {dict(zip(dr.CODES, counts[0].tolist()))}")


def _stage2(maps, finite, last_link):
    hb, link, bend = (np.stack([m[k] for m in maps]) for k in range(3))
    if last_link:
        link = link.copy()
        link[:, -1] = True                                           # the link bit of the last residue is ignored
    out, geom, fin = td.assign_on_device(hb, link, bend, finite=finite)
    ss, bridge, counts = dr.assign_batch(hb, geom, fin, sparse=True)
    assert np.array_equal(out["ss"], ss) and np.array_equal(out["bridge"], bridge) and np.array_equal(out["counts"], counts)
    dead = np.nonzero(np.asarray(fin) == 0)[0]
    assert (out["ss"][dead] == dr.UNDEFINED).all() and (out["bridge"][dead] == -1).all() and (out["counts"][dead] == -1).all()
    return out


def test_dssp_stage2_on_hand_written_bitmaps_at_high_word_indices():
    """Ladders between word 0 and words 62 / 63, partners across bits 4031 / 4032, 1279 / 1280 and 255 / 256, H, G and I runs
    across the borders of the per-residue trips (256 residues each), at R = CODLAD_DSSP_MAX_RES: the plain loops on the
    same maps, and the labels derived by hand.  Then the same maps with the last link bit set and a structure marked not
    finite in between."""
    R = dr.MAX_RES
    maps = [dr.handmade_high(R, kind) for kind in dr.HIGH_KINDS]
    out = _stage2(maps, None, False)
    for s, (_hb, _link, _bend, checks) in enumerate(maps):
        got = dr.labels(out["ss"][s])
        assert {r: got[r] for r in checks} == checks, dr.HIGH_KINDS[s]
    again = _stage2([maps[0], maps[1], maps[0]], [1, 0, 1], True)
    assert np.array_equal(again["ss"][[0, 2]], out["ss"][[0, 0]]) and np.array_equal(again["bridge"][2], out["bridge"][0])


@pytest.mark.parametrize("R", (257, 1025))
def test_dssp_stage2_on_random_bitmaps_beyond_one_trip(R):
    maps = [dr.random_maps(R, seed) for seed in (1, 2, 3)]
    out = _stage2(maps, None, False)
    assert (out["counts"][:, dr.E] > 0).all() and (out["counts"][:, dr.H] > 0).all()
    _stage2(maps, [0, 1, 1], True)


def test_dssp_refuses_one_residue_too_many():
    from codlad_amd.utils.cg_input import template_topology
    R = dr.MAX_RES + 1
    top = template_topology(["GLY"] * R)
    x = torch.zeros(1, top.n_atoms, 3, device="cuda")
    for fn in (metrics.hbonds, metrics.dssp):
        with pytest.raises(ValueError, match=f"{R} residues"):
            fn(x, top)
    W = (R + 63) // 64
    acc = torch.zeros(1, R, W, dtype=torch.int64, device="cuda")
    geom, fin = torch.zeros(1, R, dtype=torch.uint8, device="cuda"), torch.ones(1, dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError, match=f"{R} residues"):
        metrics.dssp_assign(acc, acc, geom, fin)
    # the C entry points: a non-zero return and the message, and every output keeps the sentinel
    lib = _lib.lib()
    bb, kind = (t.to("cuda").contiguous() for t in metrics.dssp_tables(top))
    i64 = lambda *shape: torch.full(shape, 0x5a5a5a5a5a5a5a5a, dtype=torch.int64, device="cuda")      # noqa: E731
    outs = dict(acc=i64(1, R, W), don=i64(1, R, W), geom=i64(R).view(torch.uint8)[:R], kappa=i64(R).view(torch.float32)[:R],
                e_best=i64(R).view(torch.float32), partner=i64(R).view(torch.int32), finite=i64(1).view(torch.uint8)[:1],
                ss=i64(R).view(torch.uint8)[:R], bridge=i64(R).view(torch.int32), counts=i64(4).view(torch.int32))
    rc = lib.codlad_dssp_hbonds(p(x), 1, top.n_atoms, p(bb), p(kind), R, p(outs["acc"]), p(outs["don"]), p(outs["geom"]),
                                p(outs["kappa"]), p(outs["e_best"]), p(outs["partner"]), p(outs["finite"]), _lib.stream_ptr(x.device))
    assert rc != 0 and "codlad_dssp_hbonds: more than CODLAD_DSSP_MAX_RES residues" in last_error()
    rc = lib.codlad_dssp_assign(p(acc), p(acc), p(geom), p(fin), 1, R, p(outs["ss"]), p(outs["bridge"]), p(outs["counts"]),
                                _lib.stream_ptr(x.device))
    assert rc != 0 and "codlad_dssp_assign: more than CODLAD_DSSP_MAX_RES residues" in last_error()
    torch.cuda.synchronize()
    for k, t in outs.items():
        assert bool((t.view(torch.uint8) == 0x5a).all()), k


# ---------------------------------------------------------------------------------------------------------- clustering
def _same_answer(o, want):
    assert o["labels"].dtype == torch.int32
    for k in ("labels", "centres", "sizes"):
        assert np.array_equal(o[k].cpu().numpy(), want[k]), k
    assert o["n_clusters"] == want["n_clusters"]


def test_cluster_beyond_64_words_against_the_loop_and_the_closed_form():
    """N = 4097: W = 65, the last word holds one structure; count_kernel's lanes take a second word.  Cliques across bits
    4031 / 4032, the last structure with members of word 0, more non-singleton cliques than one batch of rounds - with the
    padding bits clear and set, and with a finite mask that takes three would-be centres away.  Most of the rest sits in
    cliques of 389 over six or seven words each, a hundred structures stay singletons."""
    N = 4097
    cliques = cr.limit_cliques(N, fill=True)
    nb = cr.clique_matrix(N, cliques)
    fin = np.ones(N, dtype=bool)
    mid = next(m for m in cr.clique_members(cliques) if m[0] < 2048 <= m[-1])
    fin[[0, 10, mid[0]]] = False
    for finite in (None, fin):
        want, closed = cr.daura(nb, finite), cr.clique_answer(N, cliques, finite)
        assert all(want[k].tolist() == closed[k].tolist() for k in ("labels", "centres", "sizes"))
        for garbage in (False, True):
            o = metrics.cluster_neighbours(dev(cr.pack(nb, garbage)), N, finite=None if finite is None else dev(finite))
            _same_answer(o, want)
            assert o["rounds"] == closed["rounds"] > metrics.CLUSTER_BATCH
    assert o["labels"][N - 1].item() == o["labels"][1].item() and o["labels"][0].item() == -1


def _device_bitmap(N, cliques):
    """int64 [N, W] on the device from torch integer ops: the rows of a clique hold its members, without the diagonal."""
    W = (N + 63) // 64
    bits = torch.zeros(N, W, dtype=torch.int64, device="cuda")
    for m in cr.clique_members(cliques):
        idx = torch.tensor(m, dtype=torch.int64, device="cuda")
        row = torch.zeros(W, dtype=torch.int64, device="cuda")
        for w in sorted({i >> 6 for i in m}):                        # one word at a time: distinct bits add up to their OR
            row[w] = (torch.ones_like(idx) << (idx & 63))[(idx >> 6) == w].sum()
        bits[idx] = row
        bits[idx, idx >> 6] ^= torch.ones_like(idx) << (idx & 63)
    return bits


def test_cluster_at_the_largest_pool_against_the_closed_form():
    """N = CODLAD_CLUSTER_MAX_N: W = 1024 = the threads of pick_kernel, set[] / act[] of count_kernel full, 16 trips of its
    word loop; a 512 MB bitmap built on the device.  Cliques in and across words 0, 1, 62 .. 65, 511 / 512, 1022 / 1023,
    more than 65 000 singletons in every word for the closing scan."""
    N = cr.MAX_N
    cliques = cr.limit_cliques(N)
    bits = _device_bitmap(N, cliques)
    small = _device_bitmap(4097, cr.limit_cliques(4097))              # the builder itself, against numpy's
    assert np.array_equal(small.cpu().numpy(), cr.pack(cr.clique_matrix(4097, cr.limit_cliques(4097))))
    want = cr.clique_answer(N, cliques)
    o = metrics.cluster_neighbours(bits, N)
    _same_answer(o, want)
    assert o["rounds"] == want["rounds"] and int(o["sizes"].sum()) == N and want["n_clusters"] > 65000
    fin = torch.ones(N, dtype=torch.bool, device="cuda")
    fin[[10, 4091, 65535]] = False
    o = metrics.cluster_neighbours(bits, N, finite=fin)
    _same_answer(o, cr.clique_answer(N, cliques, fin.cpu().numpy()))
    del bits
    with pytest.raises(ValueError, match="65536"):
        metrics.cluster_neighbours(torch.zeros(1, 1, dtype=torch.int64, device="cuda"), N + 1)
    x = torch.zeros(N + 1, 1, 3, device="cuda")
    for fn in (lambda: metrics.rmsd_matrix(x), lambda: metrics.rmsd_neighbours(x, 1.0), lambda: metrics.cluster(x, 1.0)):
        with pytest.raises(ValueError, match="at most 65536 structures"):
            fn()


def _daura_abi(bits, N, rounds, calls):
    lib = _lib.lib()
    scratch = torch.empty((lib.codlad_cluster_scratch_bytes(N) + 7) // 8, dtype=torch.int64, device="cuda")
    state = torch.zeros(_lib.CLUSTER_STATE_WORDS, dtype=torch.int32, device="cuda")
    out = torch.full((3, N), -7, dtype=torch.int32, device="cuda")
    shots = []
    for _ in range(calls):
        rc = lib.codlad_cluster_daura(p(bits), None, N, rounds, p(state), p(out[0]), p(out[1]), p(out[2]), p(scratch),
                                      _lib.stream_ptr(bits.device))
        assert rc == 0, last_error()
        shots.append((state.cpu().numpy().copy(), out.cpu().numpy().copy()))
    return shots


def test_cluster_rounds_at_their_maximum_through_the_c_abi():
    """One call with rounds = CODLAD_CLUSTER_MAX_ROUNDS on the N = 4097 bitmap: the bits of the Python path's batches of 64;
    a second call, every launch of it after PH_DONE, changes nothing.  rounds = 4097 is refused."""
    N = 4097
    bits = dev(cr.pack(cr.clique_matrix(N, cr.limit_cliques(N, fill=True)), garbage=True))
    o = metrics.cluster_neighbours(bits, N)
    K = o["n_clusters"]
    (state, out), (state2, out2) = _daura_abi(bits, N, _lib.CLUSTER_MAX_ROUNDS, 2)
    assert state[_lib.CLUSTER_ST_PHASE] == 3 and state[_lib.CLUSTER_ST_ACTIVE] == 0 and state[_lib.CLUSTER_ST_CLUSTERS] == K
    assert state[_lib.CLUSTER_ST_ROUNDS] == o["rounds"]
    assert np.array_equal(out[0], o["labels"].cpu().numpy()) and np.array_equal(out[1, :K], o["centres"].cpu().numpy())
    assert np.array_equal(out[2, :K], o["sizes"].cpu().numpy())
    assert np.array_equal(state, state2) and np.array_equal(out, out2)
    (state0, out0), = _daura_abi(bits, N, 0, 1)                      # no round: set up, nothing picked
    assert state0[_lib.CLUSTER_ST_CLUSTERS] == 0 and state0[_lib.CLUSTER_ST_ACTIVE] == N and (out0[0] == -1).all() and (out0[1:] == -7).all()
    lib = _lib.lib()
    sent = torch.full((3, N), -7, dtype=torch.int32, device="cuda")
    st = torch.zeros(_lib.CLUSTER_STATE_WORDS, dtype=torch.int32, device="cuda")
    for n, rounds, msg in ((N, _lib.CLUSTER_MAX_ROUNDS + 1, "rounds outside"), (cr.MAX_N + 1, 1, "bad size")):
        assert lib.codlad_cluster_daura(p(bits), None, n, rounds, p(st), p(sent[0]), p(sent[1]), p(sent[2]), p(bits), None) != 0
        assert msg in last_error()
    assert lib.codlad_rmsd_matrix_scratch_bytes(cr.MAX_N + 1, 1) < 0 and lib.codlad_cluster_scratch_bytes(cr.MAX_N + 1) < 0
    torch.cuda.synchronize()
    assert bool((sent == -7).all()) and not bool(st.any())


# --------------------------------------------------------------------------------- the RMSD matrix past 64 words a row
RMSD_N, RMSD_ATOMS, RMSD_BLOBS = 4160, 4, 6
SUB = (0, 63, 64, 65, 4030, 4031, 4032, 4033, 4094, 4095, 4096, 4097, 4158, 4159)


def test_rmsd_matrix_and_bitmap_at_65_blocks_a_side():
    """N = 4160: 65 x 65 blocks, word indices I, J = 64, rows of 65 words.  The bitmap is msd <= cut2 of the device's own
    matrix everywhere; the matrix is symmetric to the bit; a fixed sample of pairs whose indices cover blocks 0, 1, 63, 64,
    and the whole sub-pool SUB, are within ensemble_ref.msd_bound of the float64 SVD route; the sub-pool's own matrix is the
    big matrix's sub-block to the bit; cluster() is the plain loop on that bitmap."""
    N, n = RMSD_N, RMSD_ATOMS
    x, blob = cr.planted(N, n, RMSD_BLOBS)
    xd = dev(x)
    cut2 = cr.PLANTED_CUTOFF * cr.PLANTED_CUTOFF
    msd_d = metrics.rmsd_matrix(xd, squared=True)
    assert tuple(msd_d.shape) == (N, N) and torch.equal(msd_d, msd_d.T) and bool((msd_d.diagonal() == 0).all())
    nbm = metrics.rmsd_neighbours(xd, cr.PLANTED_CUTOFF, return_matrix=True)
    assert torch.equal(nbm["rmsd"], msd_d.sqrt()) and bool(nbm["finite"].all())
    msd = msd_d.cpu().numpy()
    del msd_d
    bits = nbm["bits"].cpu().numpy()
    assert bits.shape == (N, 65) and bits.dtype == np.int64
    nb = cr.unpack(bits, N)
    assert nb.shape == (N, N) and (nb == (msd <= cut2)).all() and nb.diagonal().all()      # N = 65 * 64: no padding bit
    assert nb[:, 4096:].any() and nb[4096:, :].any() and not np.array_equal(nb[:4096, :4096], np.zeros((4096, 4096), bool))
    # the sample: both indices from blocks 0, 1, 63, 64 (half of it), the rest from everywhere
    rng = np.random.default_rng(4160)
    edge = np.concatenate([np.arange(0, 128), np.arange(4032, 4160)])
    I = np.concatenate([rng.choice(edge, 1000), rng.integers(0, N, 1000)])
    J = np.concatenate([rng.choice(edge, 1000), rng.integers(0, N, 1000)])
    keep = I != J
    I, J = I[keep], J[keep]
    assert {0, 1, 63, 64} <= set((I // 64).tolist()) and {0, 1, 63, 64} <= set((J // 64).tolist())
    worst = 0.0
    for a in range(0, I.shape[0], 250):                              # cluster_ref.all_pairs, 250 pairs (500 structures) a time
        ii, jj = I[a:a + 250], J[a:a + 250]
        ref, e0n = cr.all_pairs(np.concatenate([x[ii], x[jj]]))
        k = np.arange(ii.shape[0])
        ref, bound = np.maximum(ref[k, k + ii.shape[0]], 0.0), er.msd_bound(n, e0n[k, k + ii.shape[0]])
        err = np.abs(msd[ii, jj] - ref)
        worst = max(worst, float((err / bound).max()))
        assert (err <= bound).all()
    sub = np.array(SUB)
    ref, e0n = cr.all_pairs(x[sub])
    off = ~np.eye(sub.shape[0], dtype=bool)
    big = np.ascontiguousarray(msd[np.ix_(sub, sub)])
    assert (np.abs(big - np.maximum(ref, 0.0))[off] <= er.msd_bound(n, e0n)[off]).all()
    print(f"N={N}: max |msd_dev - msd_ref| / bound over {I.shape[0]} sampled pairs {worst:.3f}")
    assert tc.same(metrics.rmsd_matrix(dev(x[sub]), squared=True).cpu().numpy(), big)
    o = tc.host(metrics.cluster(xd, cr.PLANTED_CUTOFF))
    assert tc.same(o["bits"], bits)
    want = cr.daura(nb)
    assert o["labels"].tolist() == want["labels"].tolist() and o["centres"].tolist() == want["centres"].tolist()
    assert o["sizes"].tolist() == want["sizes"].tolist() and o["n_clusters"] == len(set(blob.tolist())) == RMSD_BLOBS


# --------------------------------------------------------------------------------------------------------- reweighting
BIG_N = 16400                                                        # chunk 528, 32 chunks (the last of 32 rows), 65 row blocks


@pytest.mark.parametrize("M", (3, 65))
def test_reweight_past_16384_structures_meets_the_stop_rule_and_its_outputs_follow_mu(M):
    """test_reweight's two checks, unchanged, on (16400, 3) and (16400, 65): the covariance chunk is a rounded quotient, the
    last chunk partial, more than 64 row blocks; M = 65 has two covariance tiles a side."""
    tr.test_device_mu_meets_the_stop_rule_in_longdouble(BIG_N, M)
    tr.test_outputs_are_consistent_with_mu(BIG_N, M)


@pytest.mark.parametrize("M", (3, 65))
def test_reweight_excluded_rows_in_the_last_partial_chunk(M):
    """Rows 16383 / 16384 (the border of 32 chunks of 512 and of the 64th row block) and rows of the last, partial chunk,
    excluded by w0 = 0 and by a NaN: weight exactly 0, the bits of the solve whose excluded rows hold 1e300, and the stop
    rule at the device's mu in longdouble (test_reweight's allowance, from the float64 reference of the same problem)."""
    c = rr.case(BIG_N, M)
    zero, nan = [16383, 16399], [16384, 16390]
    bad = sorted(zero + nan)
    Y, w0 = c["Y"].copy(), np.ones(BIG_N)
    w0[zero] = 0.0
    Y[16384, 0], Y[16390, M - 1] = np.nan, np.nan
    thetas = [10.0, 1.0]
    got = tr.host(metrics.reweight(dev(Y), c["y"], c["sigma"], thetas, w0=dev(w0)))
    assert (got["status"] == 0).all() and (got["w"][:, bad] == 0.0).all() and not got["used"][bad].any()
    assert got["used"].sum() == BIG_N - len(bad) and (np.delete(got["w"], bad, axis=1) > 0).all()
    w0_clean, Y2 = w0.copy(), c["Y"].copy()
    w0_clean[bad] = 0.0
    Y2[bad] = 1e300
    assert tr.same_bits(got, tr.host(metrics.reweight(dev(Y2), c["y"], c["sigma"], thetas, w0=dev(w0_clean))))
    for t, theta in enumerate(thetas):
        ref = rr.solve(c["Y"], c["y"], c["sigma"], theta, w0=w0_clean)
        allow = 4 * abs(rr.residual(c["Y"], c["y"], c["sigma"], theta, ref["mu"], w0=w0_clean)[0] -
                        rr.residual(c["Y"], c["y"], c["sigma"], theta, ref["mu"], w0=w0_clean, dtype=np.float64)[0])
        rel, _g2 = rr.residual(c["Y"], c["y"], c["sigma"], theta, got["mu"][t], w0=w0_clean)
        assert ref["status"] == 0 and rel <= tr.GTOL + allow, (theta, rel, allow)
        assert abs(got["w"][t].sum() - 1.0) <= 2 * BIG_N * tr.EPS


def test_reweight_with_every_usable_row_in_the_last_partial_chunk():
    """w0 = 0 everywhere but in rows 16368 .. 16399, the 32 rows of the 32nd covariance chunk: the Hessian is that chunk's
    alone.  A solver that leaves the chunk out is left with theta I and steepest descent; this one is held to status 0, the
    stop rule in longdouble at its mu, the Newton step count of the float64 reference (the same iteration in the same
    arithmetic) and the bits of the solve whose excluded rows hold 1e300."""
    M, first = 3, 31 * 528
    c = rr.case(BIG_N, M)
    w0 = np.zeros(BIG_N)
    w0[first:] = 1.0
    assert BIG_N - first == 32
    thetas = [10.0, 1.0, 0.1]
    got = tr.host(metrics.reweight(dev(c["Y"]), c["y"], c["sigma"], thetas, w0=dev(w0)))
    Y2 = c["Y"].copy()
    Y2[:first] = 1e300
    assert tr.same_bits(got, tr.host(metrics.reweight(dev(Y2), c["y"], c["sigma"], thetas, w0=dev(w0))))
    assert got["used"].sum() == 32 and (got["w"][:, :first] == 0).all()
    for t, theta in enumerate(thetas):
        ref = rr.solve(c["Y"], c["y"], c["sigma"], theta, w0=w0)
        allow = 4 * abs(rr.residual(c["Y"], c["y"], c["sigma"], theta, ref["mu"], w0=w0)[0] -
                        rr.residual(c["Y"], c["y"], c["sigma"], theta, ref["mu"], w0=w0, dtype=np.float64)[0])
        rel, _g2 = rr.residual(c["Y"], c["y"], c["sigma"], theta, got["mu"][t], w0=w0)
        print(f"theta {theta:g}: {got['n_iter'][t]} it (ref {ref['n_iter']}), rel {rel:.2e}, allowance {allow:.1e}")
        assert ref["status"] == 0 and got["status"][t] == 0 and rel <= tr.GTOL + allow, (theta, rel, allow)
        assert got["n_iter"][t] == ref["n_iter"] > 1, (theta, got["n_iter"][t], ref["n_iter"])


def test_reweight_offsets_of_4096_problems_past_2_to_the_31_elements():
    """CODLAD_REWEIGHT_MAX_PROBLEMS problems of case (16400, 129): 32 chunks x 6 tiles x 4096 doubles of covariance partials a
    problem, 3.2e9 doubles in all - the index of the last problems' partials does not fit 32 bits.  Every problem has the
    bits of the four-problem call's problem with its theta (compared on the device: w alone is 537 MB)."""
    N, M, P = BIG_N, 129, _lib.REWEIGHT_MAX_PROBLEMS
    assert P * 32 * 6 * 4096 > 2 ** 31
    c = rr.case(N, M)
    Y = dev(c["Y"])
    four = metrics.reweight(Y, c["y"], c["sigma"], list(rr.THETAS))
    out = metrics.reweight(Y, c["y"], c["sigma"], [rr.THETAS[i % 4] for i in range(P)])
    assert four["status"].tolist() == [0] * 4
    for k in tr.OUTPUTS:
        want = four[k] if k == "used" else four[k].repeat(*([P // 4] + [1] * (four[k].dim() - 1)))
        assert out[k].shape == want.shape and torch.equal(out[k], want), k


def test_reweight_at_4096_problems_and_weighted_mean_at_4096_sets():
    """CODLAD_REWEIGHT_MAX_PROBLEMS problems of case (3, 2), the thetas cycling: every problem has the bits of the
    four-problem call's problem with its theta.  Its w [4096, 3] then goes through weighted_mean against the host loop in
    index order.  One problem more is refused."""
    N, M, P = 3, 2, _lib.REWEIGHT_MAX_PROBLEMS
    c, four = rr.case(N, M), tr.solved(3, 2)
    Y = dev(c["Y"])
    thetas = [rr.THETAS[i % 4] for i in range(P)]
    out = metrics.reweight(Y, c["y"], c["sigma"], thetas)
    got = tr.host(out)
    cyc = np.arange(P) % 4
    assert (got["status"] == 0).all()
    for k in tr.OUTPUTS:
        want = four[k] if k == "used" else four[k][cyc]
        assert got[k].shape == want.shape and np.array_equal(got[k], want), k
    values = np.random.Generator(np.random.PCG64(4096)).standard_normal((N, 7, 3))
    want = np.zeros((P, 7, 3))
    for s in range(N):
        want = want + got["w"][:, s, None, None] * values[s][None]
    avg = metrics.weighted_mean(dev(values), out["w"]).cpu().numpy()
    assert avg.shape == (P, 7, 3) and avg.dtype == np.float64 and np.array_equal(avg, want)
    with pytest.raises(ValueError, match=f"1 .. {P} positive finite numbers"):
        metrics.reweight(Y, c["y"], c["sigma"], thetas + [1.0])
    # CODLAD_REWEIGHT_MAX_ITER iterations enqueued: the launches after the stop rule held change nothing
    long = tr.host(metrics.reweight(Y, c["y"], c["sigma"], list(rr.THETAS), max_iter=_lib.REWEIGHT_MAX_ITER))
    assert tr.same_bits(long, four)
    with pytest.raises(ValueError, match="max_iter must be an integer in 1 .. 1000"):
        metrics.reweight(Y, c["y"], c["sigma"], 1.0, max_iter=_lib.REWEIGHT_MAX_ITER + 1)


# ------------------------------------------------------------------------------------------- SAXS, hydration and P(r)
Q_KEYS = ((65, sr.MAX_Q, sr.MAX_TYPES, 500.0, "q0"), (129, sr.MAX_Q, sr.MAX_TYPES, 0.0, "plain"))


@pytest.mark.parametrize("key", Q_KEYS, ids=sr.case_id)
def test_saxs_profile_at_512_q_values_and_32_types(key):
    ts.test_profile_against_the_float64_reference(key)


@pytest.mark.parametrize("key", Q_KEYS, ids=sr.case_id)
def test_saxs_partials_at_512_q_values_and_32_types(key):
    th.test_partials_against_float64_the_plain_profile_and_the_combination(key)


def test_saxs_refuses_one_q_value_or_type_too_many():
    c = sr.case((2, 1, 1, 500.0, "plain"))
    x = dev(c["x"])
    q = np.linspace(0.0, 0.5, sr.MAX_Q + 1)
    wt = torch.zeros(3, 2, device="cuda")
    for Q, T in ((sr.MAX_Q + 1, 1), (4, sr.MAX_TYPES + 1)):
        tab = np.ones((T, Q), dtype=np.float32)
        with pytest.raises(ValueError, match="at most 512 q values and 1 .. 32 atom types"):
            metrics.saxs_profile_lists(x, c["types"], tab, q[:Q])
        with pytest.raises(ValueError, match="at most 512 q values and 1 .. 32 atom types"):
            metrics.saxs_partials_lists(x, c["types"], tab, tab, wt, q[:Q])
    lib = _lib.lib()
    I = torch.full((3, 513), -7.0, dtype=torch.float64, device="cuda")
    fin = torch.full((8,), 0x5a, dtype=torch.uint8, device="cuda")
    typ, qd = dev(c["types"]), dev(q.astype(np.float32))
    tab = torch.ones(513, dtype=torch.float32, device="cuda")
    rc = lib.codlad_saxs_debye(p(x), 3, 2, p(typ), 1, p(tab), p(qd), 513, p(I), p(I), None, p(fin), _lib.stream_ptr(x.device))
    assert rc != 0 and "codlad_saxs_debye" in last_error()
    torch.cuda.synchronize()
    assert bool((I == -7.0).all()) and bool((fin == 0x5a).all())


def test_hydration_fit_on_a_grid_of_exactly_4096_points():
    """test_fit_returns_the_planted_grid_point...'s check on 64 x 64 = CODLAD_SAXS_HYD_MAX_GRID points, the planted point the
    last of the grid; 4097 points are refused."""
    c = hr.case(hr.FIT_KEY)
    c1, c2 = np.arange(64, dtype=np.float64) * 0.002 + 0.95, np.arange(64, dtype=np.float64) * 0.1 - 2.0
    assert c1.shape[0] * c2.shape[0] == hr.MAX_GRID
    a, b = 63, 63
    exp = 3.7 * hr.combine64(c["P"][0], c["q"], c["water"], c1[a], c2[b])
    sigma = 0.01 * exp + 1e-3 * exp[0]
    ref = hr.fit64(c["P"][0], c["q"], c["water"], exp, sigma, c1, c2)
    order = np.sort(ref["chi2_grid"].reshape(-1))
    assert ref["index"] == hr.MAX_GRID - 1 and order[0] < 1e-20 and order[1] > 1e-6
    P = th.run(c)["P"]
    fit = metrics.saxs_hydration_fit(P[0], c["q"], c["water"], exp, sigma, c1=c1, c2=c2)
    assert int(fit["index"]) == ref["index"] and float(fit["c1"]) == c1[a] and float(fit["c2"]) == c2[b]
    own = hr.fit64(P[0].cpu().numpy(), c["q"], c["water"], exp, sigma, c1, c2)
    chi2 = fit["chi2_grid"].cpu().numpy()
    assert chi2.shape == (64, 64) and np.array_equal(chi2, own["chi2_grid"])
    assert np.array_equal(fit["scale_grid"].cpu().numpy(), own["scale_grid"])
    assert float(fit["scale"]) == own["scale_grid"][a, b] and float(fit["chi2"]) == own["chi2_grid"][a, b]
    assert np.array_equal(fit["I"].cpu().numpy(), own["I"]) and abs(float(fit["scale"]) - 3.7) < 1e-4
    many = metrics.saxs_hydration_fit(P, c["q"], c["water"], exp, sigma, c1=c1, c2=c2)       # a batch of three at the limit
    assert all(torch.equal(many[k][0], fit[k]) for k in fit)
    with pytest.raises(ValueError, match="1 .. 4096 points"):
        metrics.saxs_hydration_fit(P[0], c["q"], c["water"], exp, sigma, c1=c1, c2=np.arange(65) * 0.1)
    with pytest.raises(ValueError, match="1 .. 4096 points"):
        metrics.saxs_hydration_fit(P[0], c["q"], c["water"], exp, sigma, c1=np.linspace(0.95, 1.05, 17), c2=np.arange(241) * 0.01)


def _full_hist_inputs():
    """129 atoms of 32 types, every type four times or more (every one of the 528 classes has a pair), and a bin width that
    puts the last of 4096 bins near the median distance: pairs in the last bins and beyond."""
    n, T, B = 129, pr.MAX_TYPES, pr.MAX_BINS
    rng = np.random.default_rng(528)
    x = (rng.uniform(-0.5, 0.5, (3, n, 3)) * 4.0 * n ** (1.0 / 3.0)).astype(np.float32)
    x[2] += 500.0
    types = rng.permutation(np.arange(n) % T).astype(np.int32)
    return x, types, T, B, 1.0 / 320.0


def test_pair_hist_at_4096_bins_and_32_types():
    x, types, T, B, dr_ = _full_hist_inputs()
    out = metrics.pair_histogram_lists(dev(x), types, T, dr=dr_, r_max=B * dr_)
    H, over, d_bin = (out[k].cpu().numpy() for k in ("H", "over", "d_bin"))
    H32, over32, d32 = pr.hist32(x, types, T, dr_, B)
    assert H.shape == (3, 528, B) and H.dtype == np.int32 and out["finite"].tolist() == [True] * 3
    assert np.array_equal(H, H32) and np.array_equal(over, over32) and np.array_equal(d_bin, d32)
    count = np.bincount(types, minlength=T)
    for ci, (a, b) in enumerate(pr.classes(T)):
        want = count[a] * count[b] if a < b else count[a] * (count[a] - 1) // 2
        assert want > 0 and (H[:, ci].sum(1) + over[:, ci] == want).all(), (a, b)
    # what the case is there for: the last bins are occupied, pairs lie beyond them, the last class has its share
    assert (H[:, :, B - 64:].sum((1, 2)) > 20).all() and (over.sum(1) > 1000).all() and (d_bin > B - 8).all()
    assert (H[:, 527].sum(1) + over[:, 527] > 0).all() and H.sum() > 5000
    with pytest.raises(ValueError, match="at most 4096 bins"):
        metrics.pair_histogram_lists(dev(x), types, T, dr=dr_, r_max=(B + 1) * dr_)
    with pytest.raises(ValueError, match="1 .. 32 atom types"):
        metrics.pair_histogram_lists(dev(x), types, T + 1, dr=dr_, r_max=B * dr_)


def test_pair_hist_at_65535_atoms_next_to_the_int32_ceiling():
    """One structure of CODLAD_PAIR_HIST_MAX_ATOMS atoms on a line, one type: 2 147 385 345 pairs, 98 303 below 2^31.  At
    dr = 16 and 4096 bins every pair is inside and H is pair_hist_ref.lattice_hist's closed form; at dr = 1 and one bin
    every pair lies beyond it and `over` is the whole count - a counter that wraps, or a sum that passes through a
    narrower type, cannot give it.  65536 atoms are refused.  (2.1e9 pairs a call: the measured time is in DESIGN.md.)"""
    n = pr.MAX_ATOMS
    x = dev(pr.lattice(n))
    types = np.zeros(n, dtype=np.int32)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    ev[0].record()
    wide = metrics.pair_histogram_lists(x, types, 1, dr=16.0, r_max=16.0 * pr.MAX_BINS)
    ev[1].record()
    one = metrics.pair_histogram_lists(x, types, 1, dr=1.0, r_max=1.0)
    ev[2].record()
    torch.cuda.synchronize()
    print(f"n={n}: {ev[0].elapsed_time(ev[1]):.1f} ms at 4096 bins, {ev[1].elapsed_time(ev[2]):.1f} ms at one bin (tables included)")
    H, over, d_bin = pr.lattice_hist(n, 16, pr.MAX_BINS)
    assert wide["H"].dtype == torch.int32 and np.array_equal(wide["H"].cpu().numpy().reshape(-1), H)
    assert wide["over"].tolist() == [[0]] and wide["d_bin"].tolist() == [d_bin] == [4095] and wide["finite"].tolist() == [True]
    assert one["H"].tolist() == [[[0]]] and one["over"].tolist() == [[2147385345]] and one["d_bin"].tolist() == [-1]
    with pytest.raises(ValueError, match="at most 65535 atoms"):
        metrics.pair_histogram_lists(dev(pr.lattice(n + 1)), np.zeros(n + 1, dtype=np.int32), 1, dr=16.0, r_max=65536.0)


# ------------------------------------------------------------------------------------------------ poison and red zones
def test_buffers_are_written_before_they_are_read_at_the_sizes_that_first_take_the_new_paths():
    """tests/memcheck.py (the three fills of every allocation, the zones around it) around one call per family at the size
    that first takes the new path: DSSP at 257 residues, cluster_neighbours at 4097 structures, reweight at (16400, 3),
    SAXS and its partials at 512 q values, pair_hist at 4096 bins and 32 types."""
    top, xyz, _m = dr.limit_call(257)
    N = 4097
    bitmap = cr.pack(cr.clique_matrix(N, cr.limit_cliques(N, fill=True)), garbage=True)
    rw = rr.case(BIG_N, 3)
    w0 = np.ones(BIG_N)
    w0[[16383, 16399]] = 0.0
    sx = sr.case(Q_KEYS[0])
    hx = hr.case(Q_KEYS[0])
    px, ptypes, T, B, dr_ = _full_hist_inputs()

    def dssp(g):
        out = metrics.dssp(g(torch.from_numpy(xyz.copy()), "xyz"), top)
        top.__dict__.pop("_dssp_tables")                             # the next fill builds its own tables
        return {k: out[k] for k in td.KEYS}, []

    def cluster(g):
        o = metrics.cluster_neighbours(g(torch.from_numpy(bitmap.copy()), "bits"), N)
        return {k: o[k] for k in ("labels", "centres", "sizes", "populations")}, []

    def reweight(g):
        o = metrics.reweight(g(torch.from_numpy(rw["Y"].copy()), "Y"), rw["y"], rw["sigma"], [10.0, 1.0], w0=g(torch.from_numpy(w0), "w0"))
        return {k: o[k] for k in tr.OUTPUTS}, o["status"].tolist()

    def saxs(g):
        a = metrics.saxs_profile_lists(g(torch.from_numpy(sx["x"].copy()), "xyz"), sx["types"], sx["ff"], sx["q"])
        b = metrics.saxs_partials_lists(g(torch.from_numpy(hx["x"].copy()), "xyz_h"), hx["types"], hx["ff_t"], hx["ff_d"],
                                        g(torch.from_numpy(hx["weight"].copy()), "weight"), hx["q"])
        return dict(I=a["I"], finite=a["finite"], P=b["P"], P_finite=b["finite"]), []

    def hist(g):
        o = metrics.pair_histogram_lists(g(torch.from_numpy(px.copy()), "xyz"), ptypes, T, dr=dr_, r_max=B * dr_)
        return {k: o[k] for k in ("H", "over", "d_bin", "finite")}, []

    for label, case in (("dssp 257", dssp), ("cluster 4097", cluster), ("reweight 16400", reweight), ("saxs 512", saxs),
                        ("pair_hist 4096 x 32", hist)):
        hold(label, case)
