// Shared by the translation units that hold edge kernels: argument struct, LDS layout and the XCD-aware
// node placement.  (The small-job tile kernels live in their own translation unit, edge_tile_kernels.hip: with
// them in the same unit hipcc allocated the per-node kernels' registers differently and spilled in their inner
// loops - scratch 20 -> 88 and 24 -> 116 bytes, -9 % - although their source was unchanged.)
#pragma once
#include "common.h"
#include "host_util.h"     // for the launcher that ends every kernel unit

#define HD 128

// ---------------------------------------------------------------------------------------------
// Edge kernels: one wave = one node = up to 64 neighbour columns (two 32-column passes).
// ---------------------------------------------------------------------------------------------
struct EdgeArgs {
    const int4 *node_info;
    const int32_t *E_idx;  // [n_snodes][64]
    const float *hE_in;    // [rows][64][128]
    int in_by_src;         // 1: rows indexed by structure node (h_E0), 0: by sample node
    const float *E1;       // encoder layer 0 only (may be null): W1e @ h_E0 per structure edge, hoisted
    float *hE_out;         // edge update only
    const float *P, *Q;    // [n_nodes][128]: own-node term (+bias), neighbour term
    const float *W1, *W2, *W3;
    const void *W1h, *W2h, *W3h;  // split-fp16 copies (precision 1, 2)
    const float *b2, *b3;
    const float *mods3;    // edge update: shift3, scale3, gate3 (3 x 128)
    float *S;              // message: [n_nodes][128]
    int n_nodes;
    // split-fp16 modes (block exponents, common.h): GELU constants for the input of layer 2 (scale 2^E1) and of
    // layer 3 / the message epilogue (2^(E1+E2)); edge update: the residual enters layer 3's accumulator as
    // h_E * res_scale (= 2^(E1+E2+E3)) and the LayerNorm runs with eps * res_scale^2 (exactly equivalent).
    // b2 / b3 point at biases pre-scaled to match.
    GeluK gelu_a, gelu_b;
    float res_scale, ln_eps;
    // per-node kernels of large jobs (msg_kernel_h, upd_kernel_h; every other kernel ignores both):
    const int32_t *xcd_bounds;   // [9] node bounds of the eight XCD chunks, balanced by tile cost (null: uniform chunks)
    int pair;                    // 1: two nodes with short last tiles share one 32-edge tile (edge_pair_ok below)
};

// small jobs: the work dealt out per non-empty 32-edge tile {node, half} (edge_tile_kernels.hip, edge_wide_kernels.hip)
struct EdgeTileArgs : EdgeArgs {
    const int2 *tile_list;
    int n_tiles;
};

#define LDS_BLOCK_U4 4096   // one 64 KB packed block in 16-byte words

// XCD-aware node placement.  Workgroups are dealt round-robin over the 8 XCDs (blocks b and b + 8
// share one, MI355X_MICROARCH.md "Workgroup dispatch"), each with a private 4 MB L2.  The node list
// is cut into 8 contiguous chunks and chunk b % 8 is served by the workgroups of that residue
// class, in the node kernel and in both edge kernels alike: the P/Q rows the node kernel writes,
// the neighbour rows an edge tile gathers (neighbours are nodes of the same sample, i.e. of the
// same chunk) and the edge state written by one edge kernel and read by the next then stay within
// one XCD's L2 instead of being pulled into all eight.  Placement is a speed matter only.
// Chunk granularity: large jobs use 256 nodes (the largest node-kernel workgroup: 8 waves x 32), so
// that the node kernel can follow the same chunks; below 32 768 nodes that would leave whole XCDs
// without work (eight chunks of a multiple of 256 nodes), so chunks are cut to 32 nodes and the node
// kernel keeps its plain order - at that size everything fits in any L2 anyway.
constexpr int NODE_WG_TILE = 256;
constexpr int XCD_CHUNKED_NODE_KERNEL_MIN = 32768;
__host__ __device__ inline int xcd_chunk_nodes(int n_nodes) {
    const int g = n_nodes >= XCD_CHUNKED_NODE_KERNEL_MIN ? NODE_WG_TILE : 32;
    const int tiles = (n_nodes + g - 1) / g;
    return g * ((tiles + 7) / 8);
}

// Paired last tiles (CODLAD_OPT_EDGE_PAIR).  A node's last 32-edge tile holds K - 32 (K > 32) or K (K <= 32) valid columns;
// when that is at most 16 the node is ELIGIBLE, and the last tiles of two eligible nodes fit in one tile: columns 0..15
// belong to the first node, 16..31 to the second.  A wave pairs node n with the next node of its own walk, n + stride,
// when n has two tiles (its first tile gives the time to learn the next node's K before the decision is due) and both
// are eligible.  Columns are independent of each other in every contraction, GELU and LayerNorm, so the results are
// bit for bit those of the unpaired walk.  A node's cost in HALF tiles, as the chunk balance below counts it: an
// eligible two-tile node 3, any other two-tile node 4, a one-tile node 2.
__host__ __device__ inline bool edge_node_eligible(int K) { return K <= 16 || (K > 32 && K <= 48); }
__host__ __device__ inline bool edge_pair_ok(int K, int K_next) {
    return K > 32 && K <= 48 && edge_node_eligible(K_next);
}
__host__ __device__ inline int edge_node_cost2(int K) { return K <= 32 ? 2 : (K <= 48 ? 3 : 4); }
constexpr int XCD_BOUND_GRANULE = 32;     // the balanced chunk bounds are multiples of this many nodes

struct NodeSpan {
    int first, end, stride;
};
// nodes first, first + stride, ... < end for wave `wave` of workgroup b of nb.  bounds (host or device memory, may be
// null): the nine chunk bounds of EdgeArgs::xcd_bounds.
__host__ __device__ inline NodeSpan node_span_of(int n_nodes, int nwaves, int wave, int nb, int b, const int32_t *bounds) {
    if (nb % 8) return {b * nwaves + wave, n_nodes, nb * nwaves};
    int lo, hi;
    if (bounds) {
        lo = bounds[b % 8];
        hi = bounds[b % 8 + 1];
    } else {
        const int chunk = xcd_chunk_nodes(n_nodes);
        lo = (b % 8) * chunk;
        hi = lo + chunk;
    }
    if (lo > n_nodes) lo = n_nodes;
    if (hi > n_nodes) hi = n_nodes;
    return {lo + (b / 8) * nwaves + wave, hi, (nb / 8) * nwaves};
}
DEV NodeSpan wave_node_span(int n_nodes, int nwaves, int wave, const int32_t *bounds = nullptr) {
    return node_span_of(n_nodes, nwaves, wave, gridDim.x, blockIdx.x, bounds);
}

// Small wave-uniform vectors (the centre node's P row, biases, modulation) are NOT read with
// per-lane global loads: a 128-float vector costs 16 dwordx4 instructions per lane whatever the
// addresses, and eight of those per tile were half of the kernel's traffic through the texture
// addresser (tools/ablate_edge.py).  They sit in LDS instead and are read as broadcasts.
//   message LDS (16-byte words): [W1e 4096][W2 4096][consts][P slots NWAVES x 32]
//   update  LDS                : [W12 4096][W13 4096][W11e first UPD_W1_KS k-steps][consts][P slots]
// Three blocks do not fit in 160 KB, so the update kernel streams part of ONE block from L2.  That
// block is W11e, the first contraction of a tile: its fragment loads are issued before the tile's
// own rows are even requested and run eight groups ahead (the registers are free at that point),
// which hides the L2 latency that a streamed W13 - needed last, with three tiles live - could not.
constexpr int UPD_W1_KS = 3;                              // k-steps of W11e that fit in LDS
constexpr int EDGE_CONST_U4 = 4 * 32;                     // b2, b3, modulate A, modulate B
template <bool EDGE_UPDATE, int NWAVES>
constexpr int edge_lds_u4() {
    return 2 * LDS_BLOCK_U4 + (EDGE_UPDATE ? UPD_W1_KS * 512 : 0) + EDGE_CONST_U4 + NWAVES * 32;
}

