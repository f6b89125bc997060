"""CPU: the jobs of tests/large_job_cases.py are what they claim to be.

The GPU test (test_dispatch_thresholds.py) only means something if every case lands exactly on its target - one node or one
tile more and it sits on the other side of its threshold -, if the job mixes one- and two-tile nodes and pairing and
non-pairing last tiles all along, if the last 32-node tile of the first eight-wave job really holds a single node, and
if the members that a mismatch report or the float64 check names at a chunk bound are the ones that lie there."""
import numpy as np
import pytest

from tests import large_job_cases as lj

CUS = (256, 304, 64)


def _tiles_by_count(lens, members):
    """The job's tile list as engine.Job builds it: one entry per node with K <= 32, two per node beyond."""
    K = np.concatenate([np.full(lens[m], min(64, lens[m])) for m in members])
    return int(np.where(K > 32, 2, 1).sum()), K


@pytest.mark.parametrize("cu", CUS)
def test_every_case_hits_its_target_exactly(cu):
    cases = lj.cases(cu)
    assert cases["edge_wide_max"]["target"] == 22 * cu and cases["edge_wide_max+1"]["target"] == 22 * cu + 1
    assert cases["nodeq_max"]["target"] == 8192 and cases["nodeq_max+1"]["target"] == 8193
    assert cases["quad_max"]["target"] == 64 * cu and cases["quad_max+1"]["target"] == 64 * cu + 1
    assert cases["chunked_min-1"]["target"] == 32767 and cases["chunked_min"]["target"] == 32768
    assert cases["nw4_max"]["target"] == 128 * cu and cases["nw4_max+1"]["target"] == 128 * cu + 1
    assert cases["two_halves"]["target"] == 2 * 32768 + 1 > 128 * cu          # eight waves on every supported part
    for name, case in cases.items():
        lens, members = lj.build_case(name, cu)
        nodes, tiles = lj.totals(lens, members)
        if case["kind"] == "halves":                                      # two builds interleaved: its own test below
            assert nodes == case["target"]
            continue
        n_tiles, K = _tiles_by_count(lens, members)
        assert tiles == n_tiles and nodes == K.shape[0]
        assert (nodes if case["kind"] == "nodes" else tiles) == case["target"], name
        assert lens[:8] == list(lj.LENGTHS) and len(lens) == 9 and lens[8] >= lj.MIN_FILL
        assert members.count(8) == 1                                      # one fill structure, once
        counts = [members.count(k) for k in range(8)]
        assert min(counts) >= 1 and max(counts) - min(counts) <= 1 and counts[1:] == [counts[1]] * 7
        # the order is mixed: no length sorted to one end, and both tile counts and both pairing kinds in any 64 members
        assert members != sorted(members)
        for a in range(0, len(members) - 64, 64):
            Ls = {lens[m] for m in members[a:a + 64]}
            assert Ls & {5, 12, 16} and Ls & {33, 46} and Ls & {64, 87, 130}, (name, a)
        assert lj.build_case(name, cu) == (lens, members)                 # the seed is fixed
    print(f"cu {cu}: " + ", ".join(f"{n} {c['target']} {c['kind']}" for n, c in cases.items()))


def test_two_halves_are_dealt_as_stated():
    lens, members = lj.build_case("two_halves", 256)
    nodes, _tiles = lj.totals(lens, members)
    assert nodes == 2 * 32768 + 1 and len(lens) == 10
    halves = [sum(lens[m] for m in members[p::2]) for p in range(2)]      # engine.Job.parts(2)
    assert halves == [32769, 32768] == list(lj.HALVES)
    for p in range(2):
        assert {lens[m] for m in members[p::2]} >= set(lj.LENGTHS)


@pytest.mark.parametrize("cu", CUS)
def test_last_tile_of_the_first_eight_wave_job_holds_one_node(cu):
    lens, members = lj.build_case("nw4_max+1", cu)
    off = lj.offsets(lens, members)
    n = int(off[-1])
    assert n == 128 * cu + 1 and (n + 31) // 32 == 4 * cu + 1 and n - 32 * ((n - 1) // 32) == 1
    last = lj.member_of(off, n - 1)
    assert last == len(members) - 1                                       # the last member owns that node
    lens4, members4 = lj.build_case("nw4_max", cu)
    assert lj.totals(lens4, members4)[0] % 32 == 0                        # the job before it has only full tiles


def test_chunk_size_restatement():
    assert lj.xcd_chunk_nodes(32767) == 32 * 128 and lj.xcd_chunk_nodes(32768) == 4096 and lj.xcd_chunk_nodes(32769) == 4352
    assert lj.xcd_chunk_nodes(65537) == 256 * 33 and lj.xcd_chunk_nodes(100) == 32 and lj.xcd_chunk_nodes(8193) == 1056
    for n in (8193, 32767, 32768, 32769, 38913, 65537):
        assert 8 * lj.xcd_chunk_nodes(n) >= n > 7 * lj.xcd_chunk_nodes(n) - 8 * 256


@pytest.mark.parametrize("cu", CUS)
def test_members_at_chunk_bounds_are_identified(cu):
    for name in lj.cases(cu):
        lens, members = lj.build_case(name, cu)
        off = lj.offsets(lens, members)
        n = int(off[-1])
        chunk = lj.xcd_chunk_nodes(n)
        found = lj.chunk_bound_members(off)
        assert [k for k, _b, _m, _s in found] == list(range(1, len(found) + 1)) and len(found) == (n - 1) // chunk
        assert len(found) == 7 or n <= 7 * chunk
        for k, b, m, straddles in found:
            assert b == k * chunk and off[m] <= b < off[m + 1]
            assert straddles == (off[m] <= b - 1)                         # nodes b - 1 and b belong to the same member
            # by brute force over the members
            brute = [i for i in range(len(members)) if off[i] <= b < off[i + 1]]
            assert brute == [m]
        if name in ("nw4_max+1", "chunked_min", "two_halves"):            # where the float64 check picks one
            assert any(s for _k, _b, _m, s in found), name


def test_node_placement_restatement():
    """node_place against node_kernel_h's own statement, workgroup by workgroup: every node is placed once."""
    for n, waves in ((32768, 4), (32769, 8), (65537, 8), (38913, 4)):
        chunk, per_wg = lj.xcd_chunk_nodes(n), 32 * waves
        grid = 8 * (chunk // per_wg)
        seen = np.zeros(n, dtype=np.int64)
        for blk in range(grid):
            wg_node0 = (blk % 8) * chunk + (blk // 8) * per_wg
            if wg_node0 >= n:
                continue
            for node in (wg_node0, min(wg_node0 + per_wg, n) - 1):
                c, wg, wave = lj.node_place(n, node, waves, True)
                assert (c, wg, wave) == (blk % 8, blk, (node - wg_node0) // 32)
            seen[wg_node0:min(wg_node0 + per_wg, n)] += 1
        assert (seen == 1).all()
    assert lj.node_place(8193, 8192, 4, False) == (None, 64, 0)


def test_expectations_follow_the_part():
    """What a case expects of the node update where its job is too small for node_kernel_h (parts below 128 CUs: between
    node_kernel_q and node_kernel_h lies node_kernel_w, up to 8 192 nodes), and the supported range."""
    small, mid, big = lj.cases(64), lj.cases(256), lj.cases(304)
    assert small["quad_max+1"]["expect"]["node_upd"] == ("w",) and small["quad_max+1"]["target"] == 4097
    assert small["nw4_max"]["expect"]["node_upd"] == ("w",) and small["nw4_max"]["target"] == 8192
    assert small["nw4_max+1"]["expect"]["node_upd"] == ("h8",) and small["nw4_max+1"]["target"] == 8193
    for c in (mid, big):
        assert c["quad_max+1"]["expect"]["node_upd"] == lj.H and c["nw4_max"]["expect"]["node_upd"] == ("h4",)
        assert c["nw4_max+1"]["expect"]["node_upd"] == ("h8",)
    assert lj.cases(127)["quad_max+1"]["expect"]["node_upd"] == ("w",)          # 8 129 nodes
    assert lj.cases(128)["quad_max+1"]["expect"]["node_upd"] == lj.H           # 8 193 nodes
    for c in (small, mid, big):
        assert c["quad_max"]["expect"]["node_upd"] == ("q",) and c["nodeq_max"]["expect"]["node_in"] == ("w",)
        assert c["two_halves"]["expect"]["node_upd"] == ("h8",) and c["two_halves"]["expect"]["chunked_upd"] == (True,)
    for cu in (lj.MIN_CU, lj.MAX_CU):                                           # buildable at both ends of the range
        for name, case in lj.cases(cu).items():
            nodes, tiles = lj.totals(*lj.build_case(name, cu))
            assert (tiles if case["kind"] == "edge_tiles" else nodes) == case["target"]
    for cu in (lj.MIN_CU - 1, lj.MAX_CU + 1):
        with pytest.raises(AssertionError):
            lj.cases(cu)


@pytest.mark.parametrize("cu", CUS)
def test_reference_groups_stay_small(cu):
    lens, members = lj.build_case("nw4_max+1", cu)
    groups = lj.ref_groups(lens, members, max_tiles=22 * cu)
    assert groups[0][0] == 0 and groups[-1][1] == len(members)
    assert all(a[1] == b[0] for a, b in zip(groups, groups[1:]))
    for a, b in groups:
        nodes, tiles = lj.totals(lens, members[a:b])
        assert 0 < nodes <= lj.REF_MAX_NODES <= 64 * cu and tiles <= 22 * cu
    assert len(groups) <= 2 * (128 * cu + 1) // lj.REF_MAX_NODES + 2       # tens of launches, not hundreds


def test_dispatch_record_binding_matches_the_header():
    """The names _lib.dispatch_read gives the record's words and kinds are the header's, in the header's order; the
    entry point copies no more words than asked for and always says how many it keeps."""
    import ctypes as C
    import os
    import re

    from codlad_amd import _lib
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "codlad_hip.h")).read()

    def names(prefix):
        found = sorted((int(v), n.lower()) for n, v in re.findall(rf"#define {prefix}([A-Z0-9_]+) (\d+)", header))
        assert [v for v, _n in found] == list(range(len(found)))
        return tuple(n for _v, n in found)

    assert names("CODLAD_EDGE_KIND_") == _lib.EDGE_KINDS
    assert names("CODLAD_NODE_KIND_") == _lib.NODE_KINDS
    words = names("CODLAD_DISPATCH_")
    assert words[-1] == "words" and words[:-1] == _lib.DISPATCH_WORDS
    lib = _lib.lib()
    out = (C.c_int32 * 3)(-7, -7, -7)
    assert lib.codlad_dispatch_read(out, 2) == len(_lib.DISPATCH_WORDS) and out[2] == -7 and out[0] >= 0 and out[1] >= 0
    assert lib.codlad_dispatch_read(None, 2) < 0 and b"bad arguments" in lib.codlad_last_error()
    assert set(_lib.dispatch_read()) == set(_lib.DISPATCH_WORDS)
