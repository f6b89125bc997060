// Split-fp16 node kernel of LARGE jobs (precision 1, 2), alone in its translation unit: hipcc's register allocation for a
// kernel depends on what shares its unit (edge_args.h).
#include "node_args.h"

// ---------------------------------------------------------------------------------------------
// Split-fp16 node kernel (precision 1, 2).  A workgroup of NW waves owns NW 32-node tiles; the up to 13
// weight blocks of the node update are streamed through a 2 x 64 KB LDS double buffer: block i+1
// is fetched from L2 into registers before the waves contract with block i and written to the
// other buffer after it, one barrier per block.  Every wave of the chip reads each block from L2
// once per workgroup instead of once per tile.
// ---------------------------------------------------------------------------------------------
template <bool MODE_UPD, int NW, int TERMS>
__global__ __launch_bounds__(NW * 64, (NW + 3) / 4) void node_kernel_h(NodeArgs a) {
    extern __shared__ __align__(16) u32x4 wl[];
    constexpr int NT = NW * 64;
    constexpr int PER_T = LDS_BLOCK_U4 / NT;              // 16-byte words per thread per block
    static_assert(LDS_BLOCK_U4 % NT == 0, "block must divide evenly over the workgroup");
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int h = lane >> 5, c = lane & 31;
    // large jobs: workgroup -> its 32*NW nodes inside chunk (blockIdx % 8), see wave_node_span (grid =
    // 8 x workgroups per chunk); small jobs: plain order
    const int wg_node0 = a.n_nodes >= XCD_CHUNKED_NODE_KERNEL_MIN
                             ? (blockIdx.x % 8) * xcd_chunk_nodes(a.n_nodes) + (blockIdx.x / 8) * (32 * NW)
                             : blockIdx.x * (32 * NW);
    if (wg_node0 >= a.n_nodes) return;                    // padding of the last chunk (whole workgroup)
    const int node = wg_node0 + wave * 32 + c;
    const bool valid = node < a.n_nodes;
    const int nc = valid ? node : a.n_nodes - 1;
    const int4 info = a.node_info[nc];
    const int n_blk = (MODE_UPD ? 9 : 0) + a.n_proj;

    int cur = 0;                                          // index of the block resident in wl[(cur&1)]
    // global -> LDS buffer (i & 1) without staging registers: global_load_lds_dwordx4 moves 16 bytes
    // per lane, one wave instruction = 1 KB landing contiguously at the (wave-uniform) LDS address.
    // The buffer being written is the one every wave left at the previous barrier.
    auto fetch = [&](int i) {
        const u32x4 *g = reinterpret_cast<const u32x4 *>(a.blk_h[i]);
        u32x4 *dst = wl + (i & 1) * LDS_BLOCK_U4;
#pragma unroll
        for (int q = 0; q < PER_T; ++q) {
            const int chunk = (q * NW + wave) * 64;
            __builtin_amdgcn_global_load_lds(g + chunk + lane,
                                             (__attribute__((address_space(3))) void *)(dst + chunk), 16, 0, 0);
        }
    };
    auto landed = [&]() { __builtin_amdgcn_s_waitcnt(0x0F70); };   // vmcnt(0): the LDS-direct loads are in
    // contraction with the current block while the next one streams in, then rotate the double buffer
    auto apply = [&](Tile &acc, const Tile &in, bool gelu_in) {
        const bool more = cur + 1 < n_blk;
        if (more) fetch(cur + 1);
        const u32x4 *w = wl + (cur & 1) * LDS_BLOCK_U4;
        if (gelu_in) gemm128_h_lds<TERMS, true>(acc, in, w, lane, a.gelu_ffn);
        else gemm128_h_lds<TERMS, false>(acc, in, w, lane, a.gelu_ffn);
        if (more) landed();
        __syncthreads();
        ++cur;
    };
    if (n_blk > 0) {
        fetch(0);
        landed();
    }
    // both modulations folded to one multiply-add each (tile_layernorm_affine), kept in LDS behind
    // the double buffer: A = gate (1 + scale), B = gate shift
    const float *modAB = reinterpret_cast<const float *>(wl + 2 * LDS_BLOCK_U4);
    if (MODE_UPD && tid < 64) {
        const float4 *m = reinterpret_cast<const float4 *>(a.mods) + 96 * (tid >> 5);
        const int i = tid & 31;
        const float4 s = m[i], c = m[32 + i], g = m[64 + i];
        float4 *cf = reinterpret_cast<float4 *>(wl + 2 * LDS_BLOCK_U4) + 64 * (tid >> 5);
        cf[i] = make_float4(g.x * (1.0f + c.x), g.y * (1.0f + c.y), g.z * (1.0f + c.z), g.w * (1.0f + c.w));
        cf[32 + i] = make_float4(g.x * s.x, g.y * s.y, g.z * s.z, g.w * s.w);
    }
    __syncthreads();

    Tile v;
    if (!MODE_UPD) {
        const XIn xi = x_in_load(a, nc);
        tile_load_row(v, a.x_in_b, h);
#pragma unroll
        for (int bo = 0; bo < 4; ++bo) x_in_block(v.b[bo], xi, a, bo, h);
    } else {
        Tile s, t;
        tile_load_row(s, a.S + (size_t)nc * HD, h);
        if (a.s_partials) {       // tile kernels: planes half + 2 h, added in msg_kernel_h's order (a0 + a1) + (b0 + b1)
            const size_t plane = (size_t)a.n_nodes * HD;
            tile_load_row(t, a.S + 2 * plane + (size_t)nc * HD, h);
            if (info.z > 32) {
                tile_add_row(s, a.S + plane + (size_t)nc * HD, h);
                tile_add_row(t, a.S + 3 * plane + (size_t)nc * HD, h);
            }
#pragma unroll
            for (int bo = 0; bo < 4; ++bo) s.b[bo] += t.b[bo];
        }
        tile_load_row(t, a.b3, h);
        // S is a sum over up to 64 neighbours and the only operand of the path that is not
        // normalised: contract W3 with S/64 (exact power-of-two scaling, undone below) so that the
        // fp16 halves keep 64x more headroom before 65504.  The same two multiplies take the block
        // exponents out: S arrives as 2^(E1+E2) S, the W3 block as 2^e3 W3 (a.b3 = 2^e3 b3).
        const float kf = (float)info.z * 0.015625f;
#pragma unroll
        for (int bo = 0; bo < 4; ++bo) {
            t.b[bo] *= kf;
            s.b[bo] *= a.s_scale;
        }
        apply(t, s, false);                                                   // W3 @ S
        tile_load_row(v, a.hV + (size_t)nc * HD, h);
#pragma unroll
        for (int bo = 0; bo < 4; ++bo)
#pragma unroll
            for (int r = 0; r < 16; ++r) v.b[bo][r] += (t.b[bo][r] * a.t_scale) / 30.0f;
        tile_layernorm_affine(v, 1e-6f, modAB, modAB + HD, h);
        tile_load_row(t, a.b_out, h);
#pragma unroll 1
        for (int ch = 0; ch < 4; ++ch) {
            tile_load_row(s, a.b_in + ch * HD, h);
            apply(s, v, false);                                               // W_in chunk
            apply(t, s, true);                                                // W_out chunk on GELU(hidden)
        }
#pragma unroll
        for (int bo = 0; bo < 4; ++bo) v.b[bo] += t.b[bo] * a.ffn_scale;      // exact: power-of-two scale, then the add
        tile_layernorm_affine(v, 1e-6f, modAB + 2 * HD, modAB + 3 * HD, h);
    }
    if (valid) {
        tile_store_row(v, a.hV + (size_t)node * HD, h);
        if (a.hVenc_out) tile_store_row(v, a.hVenc_out + (size_t)node * HD, h);
    }
#pragma unroll 1
    for (int p = 0; p < a.n_proj; ++p) {
        Tile in = v, out;
        const int fl = a.proj_flags[p];
        if (fl & 1) {
            if (a.venc_is_self) {
#pragma unroll
                for (int bo = 0; bo < 4; ++bo) in.b[bo] += v.b[bo];
            } else {
                tile_add_row(in, a.hVenc_in + (size_t)nc * HD, h);
            }
        }
        if (a.proj_b[p]) tile_load_row(out, a.proj_b[p], h);
        else tile_zero(out);
        if (fl & 2) tile_add_row(out, a.TS + (size_t)info.w * HD, h);
        apply(out, in, false);
        if (valid) tile_store_row(out, a.proj_out[p] + (size_t)node * HD, h);
    }
}

// NW = 4 or 8 waves (32-node tiles) per workgroup, one workgroup per CU (LDS): denoiser_forward.hip says which, and why.
template <int TERMS, int NW>
static void launch_node_hw(bool upd, const NodeArgs &na, hipStream_t st) {
    static bool attr_set = false;
    const size_t lds = 2 * 65536 + 4 * 512;
    if (!attr_set) {
        set_max_lds(reinterpret_cast<const void *>(node_kernel_h<true, NW, TERMS>), lds);
        set_max_lds(reinterpret_cast<const void *>(node_kernel_h<false, NW, TERMS>), lds);
        attr_set = true;
    }
    static_assert(NODE_WG_TILE % (32 * NW) == 0, "chunks hold whole workgroup tiles");
    const bool chunked = na.n_nodes >= XCD_CHUNKED_NODE_KERNEL_MIN;      // the kernel's own test for wg_node0
    const int wgs = chunked ? 8 * (xcd_chunk_nodes(na.n_nodes) / (32 * NW)) : (na.n_nodes + 32 * NW - 1) / (32 * NW);
    dim3 grid(wgs), block(NW * 64);
    dispatch_note(grid.x, NW, chunked);
    hipLaunchKernelGGL((upd ? node_kernel_h<true, NW, TERMS> : node_kernel_h<false, NW, TERMS>), grid, block, lds, st, na);
}

void launch_node_stream(int terms, int waves, bool upd, const NodeArgs &na, hipStream_t st) {
    if (terms == 3) return waves == 8 ? launch_node_hw<3, 8>(upd, na, st) : launch_node_hw<3, 4>(upd, na, st);
    return waves == 8 ? launch_node_hw<4, 8>(upd, na, st) : launch_node_hw<4, 4>(upd, na, st);
}
