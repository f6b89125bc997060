"""Paired last tiles of the per-node edge kernels (CODLAD_OPT_EDGE_PAIR, codlad_amd/csrc/edge_args.h) and the XCD chunks
balanced by tile cost (codlad_workspace.xcd_bounds).

CPU: the tile accounting of codlad_edge_plan_host - the function the kernels' walk is planned with - on the flagship
job and against a walk written out again here.  GPU: switch on against switch off, bit for bit."""
import ctypes as C

import numpy as np
import pytest
import torch

from codlad_amd import _lib, synth

GRID = _lib.EDGE_GRID
GROUP = 32                   # granularity of the chunk bounds, nodes
GROUP_COST = GROUP * 4       # the most a 32-node group can cost, in half tiles (two tiles per node)


def job_K(lengths, n_samples_each):
    """Neighbour counts of a job's nodes, samples protein-major as the benchmark and pipeline.Config order them."""
    return np.concatenate([np.full(L * n_samples_each, min(64, L), dtype=np.int32) for L in lengths])


def cost2(K):
    return 2 if K <= 32 else (3 if K <= 48 else 4)


def eligible(K):
    return K <= 16 or 32 < K <= 48


def walk_tiles(K, bounds, grid, pair):
    """The walk of msg_kernel_h / upd_kernel_h written out: chunk b % 8 belongs to the workgroups of that residue class,
    a wave takes every (nb / 8 * nwaves)-th node of it; a two-tile eligible node followed by an eligible one shares its
    second tile with that node's last."""
    nb, nw = grid
    tiles = pairs = 0
    for b in range(nb):
        for w in range(nw):
            if nb % 8:
                first, end, stride = b * nw + w, len(K), nb * nw
            else:
                first, end, stride = int(bounds[b % 8]) + (b // 8) * nw + w, int(bounds[b % 8 + 1]), (nb // 8) * nw
            n = first
            while n < end:
                tiles += 2 if K[n] > 32 else 1
                if pair and n + stride < end and 32 < K[n] <= 48 and eligible(K[n + stride]):
                    n += stride
                    tiles += (2 if K[n] > 32 else 1) - 1
                    pairs += 1
                n += stride
    return tiles, pairs


def check_bounds(K, bounds, stats, grid=GRID, model_cost=False):
    """The balance that is held: the tiles the waves of an XCD really walk (a wave that meets an odd number of eligible
    nodes in a row runs one on its own: two tiles, not the cost model's 1.5).  A bound sits on the 32-node boundary
    nearest to its target, at most half a group's tiles away, so a chunk exceeds the mean by at most one group.
    model_cost: hold the same for the cost model of 1, 1.5 and 2 tiles a node as well."""
    n = len(K)
    assert bounds[0] == 0 and bounds[8] == n and all(bounds[x] <= bounds[x + 1] for x in range(8))
    assert all(int(bounds[x]) % GROUP == 0 for x in range(8))
    per_xcd = [sum(cost2(int(k)) for k in K[bounds[x]:bounds[x + 1]]) for x in range(8)]
    assert per_xcd == [int(v) for v in stats[4:12]]
    if model_cost:
        assert max(per_xcd) <= sum(per_xcd) / 8 + GROUP_COST, per_xcd
    if grid[0] % 8 == 0:
        walked = [int(v) for v in stats[12:20]]
        assert sum(walked) == int(stats[2])
        assert max(walked) <= sum(walked) / 8 + GROUP_COST / 2, walked
    return per_xcd


@pytest.mark.parametrize("halves", [1, 2])
def test_flagship_job_tile_accounting(halves):
    """cfg2: 35 400 nodes, 70 800 tiles per edge launch; with the L = 46 protein's second halves paired 68 500.  The job
    runs as two half-jobs of 17 700 nodes (engine.Job.parts deals the samples alternately): both are held."""
    cfg = synth.baseline_config("cfg2")
    per = cfg["n_frames"] * cfg["n_ensemble"]
    assert per % halves == 0
    K = job_K(cfg["lengths"], per // halves)
    assert len(K) * halves == 35400
    bounds, stats = _lib.edge_plan(K, pair=True)
    assert int(stats[0]) * halves == 70800
    assert int(stats[1]) * halves == 2 * 68500            # half tiles
    # the issue's figure, the cost model on the whole job; the half-jobs are held to the tiles walked (check_bounds)
    per_xcd = check_bounds(K, bounds, stats, model_cost=halves == 1)
    tiles, pairs = walk_tiles(K, bounds, GRID, True)
    assert (tiles, pairs) == (int(stats[2]), int(stats[3]))
    # the walk pairs what a wave meets in a row: a wave with an odd count of eligible nodes keeps one on its own
    n46 = int((K == 46).sum())
    assert n46 // 2 - GRID[0] * GRID[1] // 8 <= pairs <= n46 // 2
    assert tiles == int(stats[0]) - pairs
    print(f"cfg2 / {halves}: tiles {int(stats[0])} -> {tiles} as walked ({pairs} pairs; cost model {int(stats[1]) / 2}), "
          f"bounds {bounds.tolist()}, tiles walked per XCD {[int(v) for v in stats[12:20]]}")
    # the slowest XCD sets a launch's time: against the equal ranges, which give the first XCDs 2 240 two-tile nodes each
    assert max(int(v) for v in stats[12:20]) * halves <= 0.975 * 2 * max(np.diff(_lib.edge_plan(K, pair=False)[0])) * halves
    # switch off: the eight equal ranges, every node on its own
    b0, s0 = _lib.edge_plan(K, pair=False)
    chunk = -(-len(K) // GROUP // 8) * GROUP if len(K) < 32768 else -(-len(K) // 256 // 8) * 256
    assert b0.tolist() == [min(x * chunk, len(K)) for x in range(9)]
    assert int(s0[2]) == int(s0[0]) == int(stats[0]) and int(s0[3]) == 0


def test_other_configurations_keep_their_tile_count():
    """cfg3 has no eligible node, cfg4's share almost none: nothing to pair, and the balanced chunks still hold."""
    for name in ("cfg3", "cfg4share"):
        cfg = synth.baseline_config(name)
        lengths = cfg["lengths"] if name == "cfg3" else cfg["lengths"][::8]
        K = job_K(lengths, 1 if name == "cfg3" else 16)
        bounds, stats = _lib.edge_plan(K, pair=True)
        check_bounds(K, bounds, stats)
        if name == "cfg3":
            assert not any(eligible(int(k)) for k in K) and int(stats[2]) == int(stats[0]) and int(stats[3]) == 0


@pytest.mark.parametrize("grid", [(256, 8), (8, 8), (16, 8), (63, 8)])
def test_plan_matches_the_walk_on_ragged_jobs(grid):
    rng = np.random.default_rng(5)
    pool = [5, 14, 16, 17, 32, 33, 40, 46, 48, 49, 64, 87]
    for trial in range(6):
        lens = rng.choice(pool, size=int(rng.integers(3, 120)))
        K = np.concatenate([np.full(L, min(64, L), dtype=np.int32) for L in lens])
        for pair in (True, False):
            bounds, stats = _lib.edge_plan(K, pair=pair, grid=grid)
            tiles, pairs = walk_tiles(K, bounds, grid, pair)
            assert (tiles, pairs) == (int(stats[2]), int(stats[3])), (trial, pair)
            assert int(stats[0]) == int((K > 32).sum() + len(K))
            if pair:
                check_bounds(K, bounds, stats, grid)
            else:
                assert pairs == 0 and tiles == int(stats[0])


def test_option_and_workspace_field():
    import os
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "codlad_hip.h")) as f:
        header = f.read()
    assert "#define CODLAD_OPT_EDGE_PAIR 8\n" in header and "#define CODLAD_N_OPTIONS 9\n" in header
    assert _lib.OPT_EDGE_PAIR == 8
    _lib.set_option(_lib.OPT_EDGE_PAIR, 0)
    _lib.set_option(_lib.OPT_EDGE_PAIR, 1)
    assert _lib.lib().codlad_set_option(9, 0) != 0
    assert _lib.Workspace.xcd_bounds.offset == C.sizeof(_lib.Workspace) - C.sizeof(C.c_void_p)


# ---------------------------------------------------------------------------------------------------------------------
# GPU: switch on against switch off
# ---------------------------------------------------------------------------------------------------------------------
DEV = "cuda:0"
# lengths that give every kind of last tile: K = 5, 14, 16 (eligible, one tile), 17, 32 (one tile, not eligible), 33, 40, 46,
# 48 (eligible, two tiles), 49, 64 (two tiles, not eligible; 87: K = 64 with neighbours chosen among more)
LENS = [5, 14, 16, 17, 32, 33, 40, 46, 48, 49, 64, 87]
# sample order: runs of one length (a wave meets the same K again and again, even and odd counts), eligible next to
# ineligible, one-tile eligible after two-tile eligible, and the short samples a wave meets once
MEMBERS = ([7] * 5 + [3, 8, 0, 6, 1, 9, 5, 2, 10, 4, 11] + [8] * 3 + [5, 1, 7, 2, 6, 0, 8, 9, 7, 4, 6, 10, 5, 5, 3]
           + [6] * 4 + [11, 7, 1, 7, 2, 8, 0, 5] + [7] * 6)


def _tables(T):
    from codlad_amd.diffusion_and_flow.schedule import Tables, named_betas, space_timesteps
    return Tables(named_betas("linear", 1000), space_timesteps(1000, str(T)))


def _bits(t):
    return t.contiguous().view(torch.int32).clone()


def _run(den, job, x, eps, T):
    """Everything the switch could change, as bit patterns: logits and h_V of a forward, the edge state after the forward
    (encoder layer 2) and after single launches of the layer-0 and layer-1 edge updates, the neighbour sums of single
    layer-0 and layer-1 message launches, and samples on one stream and on the default / two streams."""
    lib = den.lib
    job.hE.zero_()                       # slots of edges beyond K are never written: the same in every run
    out = {"logits": _bits(den.forward(job, x, 600)), "hV": _bits(job.hV), "hE_enc2": _bits(job.hE)}
    mods = den.step_mods([600])
    st = job.structures
    for which, layer in ((1, 0), (1, 1), (0, 0), (0, 1)):
        rc = lib.codlad_bench_edge_launch(C.byref(den.weights.struct), _lib.ptr(job.node_info), job.n_nodes,
                                          _lib.ptr(st.E_idx), _lib.ptr(st.h_E0), _lib.ptr(mods), C.byref(job.ws), which,
                                          layer, _lib.stream_ptr(den.device))
        _lib.check(rc, "codlad_bench_edge_launch")
        torch.cuda.synchronize()
        out[f"{'hE' if which else 'S'}_launch_{layer}"] = _bits(job.hE if which else job.S[0])
    for streams in (1, None, 2):
        out[f"sample_streams_{streams}"] = _bits(den.sample(job, x, eps, _tables(T), streams=streams))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("precision", ["f16x3", "f16x4"])
@pytest.mark.parametrize("edge_cus", [8, 16, 0])
def test_paired_tiles_are_bit_identical(precision, edge_cus):
    """msg_kernel_h / upd_kernel_h with paired last tiles and balanced chunks against the same kernels with every node on
    its own (CODLAD_OPT_EDGE_PAIR = 0) and against the small-job tile kernels: torch.equal on every output, hoisted layer 0
    and not.  CODLAD_OPT_EDGE_TILE_MAX_NODES = 0 sends the job to the per-node kernels; CODLAD_OPT_EDGE_CUS = 8 / 16 makes a
    wave walk 20-40 / 10-20 nodes of this job, so that it meets pairs, leftovers and every neighbour combination; the full
    grid (0) gets five copies of the job, four to five nodes per wave."""
    from codlad_amd.engine import Denoiser
    sd = synth.denoiser_state_dict(1234)
    prots = [synth.make_protein(L, 900 + i, n_frames=1) for i, L in enumerate(LENS)]
    xyz = [torch.from_numpy(p["xyz_full"])[0, 1:-1] for p in prots]
    zz = [torch.from_numpy(p["z_full"])[1:-1] for p in prots]
    # the full grid (edge_cus 0) needs five times the job for a wave to meet several nodes; it then also runs as two
    # half-jobs on two streams by default
    members = MEMBERS if edge_cus else MEMBERS * 5
    n = sum(LENS[m] for m in members)
    x = synth.gaussian((n, 3), 47).to(DEV)
    T = 10
    eps = synth.gaussian((T, n, 3), 48).to(DEV)
    K = np.concatenate([np.full(LENS[m], min(64, LENS[m]), dtype=np.int32) for m in members])
    assert (n + 7) // 8 >= (edge_cus or 256)           # the persistent grid is full
    bounds, stats = _lib.edge_plan(K, pair=True, grid=(edge_cus or 256, 8))
    assert int(stats[3]) >= 40, "the job must give the waves pairs to form"
    print(f"edge_cus {edge_cus}: {int(stats[0])} tiles -> {int(stats[2])}, {int(stats[3])} pairs")
    res = {}
    try:
        _lib.set_option(_lib.OPT_EDGE_CUS, edge_cus)
        den = Denoiser(sd, DEV, precision=precision)
        for hoist in (True, False):
            job = den.make_job(den.prepare_structures(xyz, zz, hoist_layer0=hoist), members)
            assert job.xcd_bounds.tolist() == _lib.edge_plan(K, pair=True)[0].tolist()
            for tag, max_nodes, pair in (("paired", 0, 1), ("single", 0, 0), ("tile", 1 << 30, 1)):
                _lib.set_option(_lib.OPT_EDGE_TILE_MAX_NODES, max_nodes)
                _lib.set_option(_lib.OPT_EDGE_PAIR, pair)
                res[hoist, tag] = _run(den, job, x, eps, T)
    finally:
        _lib.set_option(_lib.OPT_EDGE_TILE_MAX_NODES, 1 << 30)
        _lib.set_option(_lib.OPT_EDGE_PAIR, 1)
        _lib.set_option(_lib.OPT_EDGE_CUS, 0)
    for hoist in (True, False):
        ref = res[hoist, "single"]
        assert bool(torch.isfinite(ref["logits"].view(torch.float32)).all())
        for tag in ("paired", "tile"):
            for key, want in ref.items():
                if tag == "tile" and key.startswith("S_launch"):
                    continue     # the tile kernels keep the message sums as partial sums per half (S planes 1-3)
                assert torch.equal(res[hoist, tag][key], want), (precision, edge_cus, hoist, tag, key)
