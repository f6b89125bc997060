"""Jobs that sit on either side of every size threshold of the denoiser's dispatch (tests/test_dispatch_thresholds.py,
GPU) and the CPU test that holds them to what they claim (tests/test_large_job_cases_host.py).  Nothing here touches a GPU.

A job is a list of short structures repeated many times, so the feature prepass stays small: LENGTHS holds one-tile nodes
(K = L <= 32) and two-tile nodes (K = min(64, L) > 32), last tiles that pair (L = 46: 14 columns; L = 12, 5, 16: at most
16; L = 33: one column) and last tiles that do not (L = 64, 87, 130: 32 columns).  One fill structure of the remainder
length makes the total exact, and the member order is shuffled with a fixed seed, so every chunk, workgroup and wave of a
persistent grid holds mixed lengths.  A node of a structure of L residues has min(64, L) neighbours, i.e. one non-empty
32-edge tile up to L = 32 and two beyond.

The thresholds are those of enqueue_forward / launch_edge_now / launch_node (codlad_amd/csrc/denoiser_forward.hip) and of
node_kernel_h's placement (edge_args.h); `cases(cu)` states per case only what THAT threshold decides, and the GPU test
reads the rest from the dispatch record (codlad_dispatch_read) instead of restating the rules.
"""
import numpy as np

LENGTHS = (5, 12, 16, 33, 46, 64, 87, 130)
ROUND_NODES = sum(LENGTHS)                                              # 393
SHUFFLE_SEED = 20241
STRUCT_SEED = 880                                                       # synth.make_protein(L, STRUCT_SEED + L)
CHUNKED_MIN = 32768                                                     # XCD_CHUNKED_NODE_KERNEL_MIN
NODEQ_MAX_NODES = 32 * 256                                              # CODLAD_OPT_NODEQ_MAX_TILES tiles of 32 nodes
MIN_FILL = 5                                                            # no fill structure shorter than the shortest member
REF_MAX_NODES = 1024                                                    # the reference jobs of the bit comparison


def node_tiles(L):
    """Non-empty 32-edge tiles of every node of a structure of L residues."""
    return 2 if min(64, L) > 32 else 1


def struct_tiles(L):
    return L * node_tiles(L)


ROUND_TILES = sum(struct_tiles(L) for L in LENGTHS)                     # 753


def xcd_chunk_nodes(n):
    """edge_args.h, restated: the node kernel's eight chunks (placement, not arithmetic)."""
    g = 256 if n >= CHUNKED_MIN else 32
    return g * ((-(-n // g) + 7) // 8)


def build(target, kind, seed=SHUFFLE_SEED):
    """-> (lens, members): the structures' lengths (LENGTHS, then the fill structure) and the job's members as indices
    into them, in job order.  kind "nodes": exactly `target` nodes; "edge_tiles": exactly `target` non-empty 32-edge
    tiles.  Every length of LENGTHS occurs equally often (plus, for an odd tile remainder, one more L = 5)."""
    assert kind in ("nodes", "edge_tiles")
    members = []
    if kind == "nodes":
        assert target >= ROUND_NODES + MIN_FILL
        rounds = (target - MIN_FILL) // ROUND_NODES
        fill = target - rounds * ROUND_NODES                            # MIN_FILL .. ROUND_NODES + MIN_FILL - 1
    else:
        # the fill has two tiles per node, so it takes an even remainder; an odd one gives five tiles to one more L = 5
        assert target >= ROUND_TILES + 71
        rounds = (target - 71) // ROUND_TILES
        rest = target - rounds * ROUND_TILES                            # 71 .. 823
        if rest % 2:
            members.append(LENGTHS.index(5))
            rest -= 5
        fill = rest // 2                                                # 33 .. 411
        assert fill > 32
    members += list(range(len(LENGTHS))) * rounds + [len(LENGTHS)]
    order = np.random.Generator(np.random.PCG64(seed)).permutation(len(members))
    return list(LENGTHS) + [fill], [members[i] for i in order]


def build_halves(first, second):
    """A job whose alternately dealt halves (Job.parts(2): members 0, 2, 4, ... and 1, 3, 5, ...) have exactly `first` and
    `second` nodes: two node-count builds interleaved.  -> (lens, members); two fill structures."""
    la, ma = build(first, "nodes", SHUFFLE_SEED + 1)
    lb, mb = build(second, "nodes", SHUFFLE_SEED + 2)
    assert len(ma) in (len(mb), len(mb) + 1)
    fill_b = len(la)
    mb = [fill_b if m == len(LENGTHS) else m for m in mb]
    members = [m for pair in zip(ma, mb) for m in pair] + ma[len(mb):]
    return la + [lb[-1]], members


def offsets(lens, members):
    """Node offsets of the members: int64 [len(members) + 1]."""
    return np.concatenate([[0], np.cumsum([lens[m] for m in members])]).astype(np.int64)


def totals(lens, members):
    """-> (nodes, non-empty 32-edge tiles)."""
    return sum(lens[m] for m in members), sum(struct_tiles(lens[m]) for m in members)


def member_of(off, node):
    """The member that holds `node`."""
    m = int(np.searchsorted(off, node, side="right")) - 1
    assert 0 <= m < len(off) - 1 and off[m] <= node < off[m + 1]
    return m


def chunk_bound_members(off):
    """Per inner chunk bound b = k x xcd_chunk_nodes(n) < n, k = 1 .. 7: (k, b, member holding node b, straddles), where
    straddles says that the member also holds node b - 1, i.e. lies on both sides of the bound."""
    n = int(off[-1])
    chunk = xcd_chunk_nodes(n)
    out = []
    for k in range(1, 8):
        b = k * chunk
        if b >= n:
            break
        m = member_of(off, b)
        out.append((k, b, m, bool(off[m] < b)))
    return out


def node_place(n_nodes, node, waves, chunked):
    """Where node_kernel_h with `waves` waves per workgroup puts `node` -> (chunk, workgroup index, wave): the
    restatement of its wg_node0 (node_stream_kernel.hip) that a mismatch report quotes."""
    per_wg = 32 * waves
    if not chunked:
        return None, node // per_wg, node % per_wg // 32
    chunk = xcd_chunk_nodes(n_nodes)
    c, r = divmod(node, chunk)
    return c, c + 8 * (r // per_wg), r % per_wg // 32


def ref_groups(lens, members, max_tiles, max_nodes=REF_MAX_NODES):
    """Consecutive members grouped into reference jobs of at most max_nodes nodes and max_tiles non-empty 32-edge tiles
    -> [(first member, end member)]."""
    groups, a, nodes, tiles = [], 0, 0, 0
    for i, m in enumerate(members):
        L, t = lens[m], struct_tiles(lens[m])
        assert L <= max_nodes and t <= max_tiles
        if nodes + L > max_nodes or tiles + t > max_tiles:
            groups.append((a, i))
            a, nodes, tiles = i, 0, 0
        nodes += L
        tiles += t
    groups.append((a, len(members)))
    return groups


H = ("h4", "h8")           # node_kernel_h, either wave count
MIN_CU, MAX_CU = 38, 511   # below: 22 x CU tiles are less than one round and a fill; above: 64 x CU reaches CHUNKED_MIN


def cases(cu):
    """name -> dict(target, kind, expect, what).  expect: words of the dispatch record (_lib.dispatch_read) -> the values
    this side of this threshold allows - only the words the threshold decides on a part with `cu` compute units, MIN_CU <= cu <=
    MAX_CU.  Between node_kernel_q (up to 64 x cu nodes) and node_kernel_h (beyond NODEQ_MAX_NODES) the node update of a
    part with fewer than 128 CUs passes through node_kernel_w, as the input node kernel does on every part: where a
    case's job is that small, `past_quad` says so."""
    assert MIN_CU <= cu <= MAX_CU, f"the cases are laid out for parts of {MIN_CU} .. {MAX_CU} compute units"
    c = {}

    def past_quad(n_nodes, stream):
        return "w" if n_nodes <= NODEQ_MAX_NODES else stream

    def add(name, target, kind, what, **expect):
        c[name] = dict(target=target, kind=kind, what=what,
                       expect={k: (v if isinstance(v, tuple) else (v,)) for k, v in expect.items()})

    add("edge_wide_max", 22 * cu, "edge_tiles", "the last job of msg_wide_kernel / upd_wide_kernel", edge="wide")
    add("edge_wide_max+1", 22 * cu + 1, "edge_tiles", "the first job of the per-node edge kernels", edge=("node", "node_upd1"))
    add("nodeq_max", NODEQ_MAX_NODES, "nodes", "the last job whose input node kernel is node_kernel_w", node_in="w")
    add("nodeq_max+1", NODEQ_MAX_NODES + 1, "nodes", "the first whose input node kernel is node_kernel_h", node_in=H)
    add("quad_max", 64 * cu, "nodes", "the last job whose node update is node_kernel_q", node_upd="q")
    add("quad_max+1", 64 * cu + 1, "nodes", "the first whose node update is not node_kernel_q", node_upd=past_quad(64 * cu + 1, H))
    add("chunked_min-1", CHUNKED_MIN - 1, "nodes", "the last job in plain workgroup order", chunked_upd=False)
    add("chunked_min", CHUNKED_MIN, "nodes", "the first with XCD-chunked node kernels", chunked_upd=True, chunked_in=True,
        node_upd=H, node_in=H)
    add("nw4_max", 128 * cu, "nodes", "the last job with four waves per node workgroup", node_upd=past_quad(128 * cu, "h4"))
    add("nw4_max+1", 128 * cu + 1, "nodes", "the first with eight; its last 32-node tile holds one node",
        node_upd=past_quad(128 * cu + 1, "h8"))
    add("two_halves", sum(HALVES), "halves", "both halves that `sample` deals are chunked; whole: eight waves, chunked",
        chunked_upd=True, chunked_in=True, node_upd="h8", node_in="h8", edge=("node", "node_upd1"))
    return c


HALVES = (CHUNKED_MIN + 1, CHUNKED_MIN)    # 2 x 32 768 + 1 nodes: both halves that `sample` deals are chunked


def build_case(name, cu):
    if name == "two_halves":
        return build_halves(*HALVES)
    case = cases(cu)[name]
    return build(case["target"], case["kind"])
