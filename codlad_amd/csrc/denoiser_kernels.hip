// Per-step kernels of the mpnn_diffusion denoiser for gfx950 (SURVEY.md 8a rows 5-7 + row 2).
//
// Algebra used (results equal the reference's up to fp32 summation order):
//   W1 @ [h_V_i | h_E_ij | h_V_j] = W1a @ h_V_i + W1e @ h_E_ij + W1c @ h_V_j
//     -> the two node terms are projected once per node (P, Q) and gathered per edge, only
//        the h_E term is a per-edge contraction;
//   sum_k (W3 @ g_k + b3) = W3 @ (sum_k g_k) + K * b3
//     -> the third message layer runs once per node on the neighbour sum S.
// Per edge this leaves 2 (message) or 3 (edge update) 128x128 contractions, all on
// v_mfma_f32_32x32x2_f32 through the register chain of common.h.
#include "common.h"
#include <stdlib.h>
#include "../../include/codlad_hip.h"

#include "edge_args.h"
#include <vector>


template <bool EDGE_UPDATE>
__global__ __launch_bounds__(256, 2) void edge_kernel(EdgeArgs a) {
    const int lane = threadIdx.x & 63;
    const int n = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (n >= a.n_nodes) return;
    const int h = lane >> 5, c = lane & 31;
    const int4 info = a.node_info[n];
    const int src = info.x, base = info.y, K = info.z;
    const float *rows = a.hE_in + (size_t)(a.in_by_src ? src : n) * (64 * HD);
    const float *Prow = a.P + (size_t)n * HD;

    for (int half = 0; half < 2; ++half) {
        if (32 * half >= K) break;
        const int col = 32 * half + c;
        const bool valid = col < K;
        const int colc = valid ? col : 0;
        const int j = a.E_idx[(size_t)src * 64 + colc];

        Tile x, acc;
        tile_load_row(acc, Prow, h);
        tile_add_row(acc, a.Q + (size_t)(base + j) * HD, h);
        if (a.E1) {   // layer-1 edge term precomputed per structure (step- and member-invariant)
            tile_add_edge(acc, a.E1 + (size_t)src * EDGE_BLOCK, colc, h);
        } else {
            tile_load_edge(x, rows, colc, h);
            gemm128(acc, x, a.W1, lane);
        }
        const GeluK gk = gelu_consts(0);
        tile_gelu(acc, gk);
        tile_load_row(x, a.b2, h);
        gemm128(x, acc, a.W2, lane);
        tile_gelu(x, gk);

        if (!EDGE_UPDATE) {
            // S[n] = sum over the valid columns; each half reduces its 32 lanes, the second
            // half adds to what the first one stored (same wave, program order)
            float *Srow = a.S + (size_t)n * HD;
#pragma unroll
            for (int bo = 0; bo < 4; ++bo)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    x.b[bo][r] = half_wave_sum(valid ? x.b[bo][r] : 0.f);
                }
            if (c == 31) {
                if (half) tile_add_row(x, Srow, h);
                tile_store_row(x, Srow, h);
            }
        } else {
            tile_load_row(acc, a.b3, h);
            gemm128(acc, x, a.W3, lane);
            tile_add_edge(acc, rows, colc, h);  // residual: h_E + message
            tile_layernorm(acc, 1e-6f);
            tile_modulate(acc, a.mods3, a.mods3 + HD, a.mods3 + 2 * HD, h);
            if (valid) tile_store_edge(acc, a.hE_out + (size_t)n * EDGE_BLOCK, col, h);
        }
    }
}

#include "node_args.h"

template <bool MODE_UPD>
__global__ __launch_bounds__(64, 1) void node_kernel(NodeArgs a) {
    const int lane = threadIdx.x & 63;
    const int h = lane >> 5, c = lane & 31;
    const int node = blockIdx.x * 32 + c;
    const bool valid = node < a.n_nodes;
    const int nc = valid ? node : a.n_nodes - 1;
    const int4 info = a.node_info[nc];

    Tile v;
    if (!MODE_UPD) {
        const float x0 = a.x[nc * 3 + 0], x1 = a.x[nc * 3 + 1], x2 = a.x[nc * 3 + 2];
        const bool sc = a.in_dim == 6;
        const bool have_sc = sc && a.x_sc != nullptr;
        const float s0 = have_sc ? a.x_sc[nc * 3 + 0] : 0.f, s1 = have_sc ? a.x_sc[nc * 3 + 1] : 0.f,
                    s2 = have_sc ? a.x_sc[nc * 3 + 2] : 0.f;
        tile_load_row(v, a.x_in_b, h);
#pragma unroll
        for (int bo = 0; bo < 4; ++bo)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int f = 32 * bo + (r & 3) + 8 * (r >> 2) + 4 * h;
                const float *wr = a.x_in_w + f * a.in_dim;
                float acc = 0.f;
                if (sc) {   // input = cat(x_self_cond, x): weight columns 0-2 | 3-5
                    acc = fmaf(s2, wr[2], fmaf(s1, wr[1], s0 * wr[0]));
                    wr += 3;
                }
                v.b[bo][r] += fmaf(x2, wr[2], fmaf(x1, wr[1], fmaf(x0, wr[0], acc)));
            }
    } else {
        Tile s, t;
        tile_load_row(s, a.S + (size_t)nc * HD, h);
        tile_load_row(t, a.b3, h);
        const float kf = (float)info.z;
#pragma unroll
        for (int bo = 0; bo < 4; ++bo) t.b[bo] *= kf;
        gemm128(t, s, a.W3, lane);
        tile_load_row(v, a.hV + (size_t)nc * HD, h);
#pragma unroll
        for (int bo = 0; bo < 4; ++bo)
#pragma unroll
            for (int r = 0; r < 16; ++r) v.b[bo][r] += t.b[bo][r] / 30.0f;
        tile_layernorm(v, 1e-6f);
        tile_modulate(v, a.mods, a.mods + HD, a.mods + 2 * HD, h);
        // position-wise FFN 128 -> 512 -> 128 in four 128-wide hidden chunks
        tile_load_row(t, a.b_out, h);
#pragma unroll 1
        for (int ch = 0; ch < 4; ++ch) {
            tile_load_row(s, a.b_in + ch * HD, h);
            gemm128(s, v, a.Win[ch], lane);
            tile_gelu(s, gelu_consts(0));
            gemm128(t, s, a.Wout[ch], lane);
        }
#pragma unroll
        for (int bo = 0; bo < 4; ++bo) v.b[bo] += t.b[bo];
        tile_layernorm(v, 1e-6f);
        tile_modulate(v, a.mods + 3 * HD, a.mods + 4 * HD, a.mods + 5 * HD, h);
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
        gemm128(out, in, a.proj_w[p], lane);
        if (valid) tile_store_row(out, a.proj_out[p] + (size_t)node * HD, h);
    }
}

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
        const float x0 = a.x[nc * 3 + 0], x1 = a.x[nc * 3 + 1], x2 = a.x[nc * 3 + 2];
        const bool sc = a.in_dim == 6;
        const bool have_sc = sc && a.x_sc != nullptr;
        const float s0 = have_sc ? a.x_sc[nc * 3 + 0] : 0.f, s1 = have_sc ? a.x_sc[nc * 3 + 1] : 0.f,
                    s2 = have_sc ? a.x_sc[nc * 3 + 2] : 0.f;
        tile_load_row(v, a.x_in_b, h);
#pragma unroll
        for (int bo = 0; bo < 4; ++bo)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int f = 32 * bo + (r & 3) + 8 * (r >> 2) + 4 * h;
                const float *wr = a.x_in_w + f * a.in_dim;
                float acc = 0.f;
                if (sc) {   // input = cat(x_self_cond, x): weight columns 0-2 | 3-5
                    acc = fmaf(s2, wr[2], fmaf(s1, wr[1], s0 * wr[0]));
                    wr += 3;
                }
                v.b[bo][r] += fmaf(x2, wr[2], fmaf(x1, wr[1], fmaf(x0, wr[0], acc)));
            }
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

// ---------------------------------------------------------------------------------------------
// FinalLayer (latent_model.py:31-35) + ancestral DDPM update (gaussian_diffusion.py:303-367,446).
// One thread per node.
// ---------------------------------------------------------------------------------------------
struct FinalArgs {
    const float *hV;
    const float *mods;  // shift, scale (2 x 128)
    const float *out_w, *out_b;
    int n_nodes;
    float *logits;      // [n][6] or null
    float *x;           // in/out [n][3] (update mode)
    const float *noise; // [n][3]
    const float *coef;  // device [8]
    float *x_start;     // [n][3] or null: pred_xstart of this step (self-conditioning input of the next)
    int *status;        // sticky status word or null (CODLAD_STATUS_NONFINITE)
    int n_out;          // 6 (eps | variance logits, diffusion) or 3 (velocity, flow matching: logits mode only)
};

// 32 lanes per node (one 16-byte word of the row each: coalesced 512-byte row reads, the reductions are
// butterflies inside the half wave), 8 nodes per 256-thread block.
DEV float half_wave_allsum(float v) {
#pragma unroll
    for (int m = 16; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

// PIN: residue pinning fused into the update (codlad_sample_loop_pinned): at a node with pin_mask[n] != 0 the step's
// raw pred_xstart is replaced by pin_x0[n] before the clamp.  A template parameter, so that final_kernel<false> (the
// logits mode and the plain loop) is instruction for instruction the kernel it was before pinning existed; only its
// argument block grows by the two unused pointers.
// STEP: the update of the loop - CODLAD_STEP_DDPM (ddpm_step, mode from the table's column 7), CODLAD_STEP_DDIM or
// CODLAD_STEP_DDIM_REVERSE (ddim_step with the host's `mode` argument; the reverse step reads no noise).  The DDPM
// instantiations are instruction for instruction what they were before DDIM existed (they do not read `mode`, which
// follows the other arguments).
#define CODLAD_STEP_DDPM 0
#define CODLAD_STEP_DDIM 1
#define CODLAD_STEP_DDIM_REVERSE 2
template <bool PIN, int STEP = CODLAD_STEP_DDPM>
__global__ __launch_bounds__(256) void final_kernel(FinalArgs a, const float *pin_x0, const uint8_t *pin_mask, int mode) {
    const int l = threadIdx.x & 31;
    const int n = blockIdx.x * 8 + (threadIdx.x >> 5);
    const bool live = n < a.n_nodes;
    const int nc = live ? n : a.n_nodes - 1;           // whole half waves stay converged for the shuffles
    const float4 v = reinterpret_cast<const float4 *>(a.hV + (size_t)nc * HD)[l];
    const float mean = half_wave_allsum((v.x + v.y) + (v.z + v.w)) * (1.0f / 128.0f);
    const float d0 = v.x - mean, d1 = v.y - mean, d2 = v.z - mean, d3 = v.w - mean;
    const float var = half_wave_allsum((d0 * d0 + d1 * d1) + (d2 * d2 + d3 * d3));
    const float rstd = 1.0f / sqrtf(var * (1.0f / 128.0f) + 1e-6f);
    const float4 sh = reinterpret_cast<const float4 *>(a.mods)[l], sc = reinterpret_cast<const float4 *>(a.mods + HD)[l];
    const float m0 = (d0 * rstd) * (1.0f + sc.x) + sh.x, m1 = (d1 * rstd) * (1.0f + sc.y) + sh.y,
                m2 = (d2 * rstd) * (1.0f + sc.z) + sh.z, m3 = (d3 * rstd) * (1.0f + sc.w) + sh.w;
    float o[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        o[k] = 0.f;
        if (k < a.n_out) {
            const float4 w = reinterpret_cast<const float4 *>(a.out_w + k * HD)[l];
            o[k] = half_wave_allsum(fmaf(m3, w.w, fmaf(m2, w.z, fmaf(m1, w.y, m0 * w.x)))) + a.out_b[k];
        }
    }
    if (!live) return;
    if (a.status && l == 0) {
        // inf / NaN by exponent bits.  This file is built with -fno-honor-nans: the compiler folds x != x away and
        // even turns the bit test on a float's bits into |x| == inf (false for NaN), so the bits are laundered
        // through an empty asm and tested as the integers they then are.
        bool bad = false;
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            unsigned u = __float_as_uint(o[k]);
            asm volatile("" : "+v"(u));
            bad |= (u & 0x7f800000u) == 0x7f800000u;
        }
        if (bad) atomicOr(a.status, CODLAD_STATUS_NONFINITE);
    }
    if (a.logits) {
        if (l < a.n_out) {
            float mine = o[0];
#pragma unroll
            for (int k = 1; k < 6; ++k) mine = l == k ? o[k] : mine;
            a.logits[(size_t)n * a.n_out + l] = mine;
        }
        return;
    }
    if (l < 3) {                                        // lane k updates component k
        const float eps = l == 0 ? o[0] : (l == 1 ? o[1] : o[2]);
        const float vv = l == 0 ? o[3] : (l == 1 ? o[4] : o[5]);      // (zeros for a 3-row head: fixed-variance samplers)
        const size_t i = (size_t)n * 3 + l;
        const float *pin = PIN && pin_mask[n] ? pin_x0 + i : nullptr;
        if constexpr (STEP == CODLAD_STEP_DDPM)
            a.x[i] = ddpm_step(a.x[i], eps, vv, a.coef, a.noise[i], a.x_start ? a.x_start + i : nullptr, pin);
        else if constexpr (STEP == CODLAD_STEP_DDIM)
            a.x[i] = ddim_step<false>(a.x[i], eps, a.coef, mode, a.noise[i], a.x_start ? a.x_start + i : nullptr, pin);
        else
            a.x[i] = ddim_step<true>(a.x[i], eps, a.coef, mode, 0.f, a.x_start ? a.x_start + i : nullptr, pin);
    }
}

// stand-alone DDPM update on a model output [n][6]
struct DdpmCoef {
    float c[8];
};

__global__ void ddpm_kernel(const float *x, const float *out, const float *noise, DdpmCoef cf,
                            int n_nodes, float *x_out, float *x_start) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_nodes * 3) return;
    const int n = i / 3, k = i - 3 * n;
    // a fixed-variance sampler's model has no variance channels (gaussian_diffusion.py:321-334: model_output stays [.., C])
    const bool fixed = ((int)cf.c[7] & CODLAD_DDPM_FIXED_VAR) != 0;
    const float o = fixed ? out[n * 3 + k] : out[n * 6 + k], v = fixed ? 0.f : out[n * 6 + 3 + k];
    x_out[i] = ddpm_step(x[i], o, v, cf.c, noise[i], x_start ? x_start + i : nullptr);
}

// The DDPM update split in two around a caller's denoised_fn / cond_fn (codlad_ddpm_pred_xstart /
// codlad_ddpm_posterior_step): the pieces of ddpm_step, so that a pin applied between them rounds as the fused one.
__global__ void ddpm_pred_xstart_kernel(const float *x, const float *out, DdpmCoef cf, int n_nodes, float *x0_out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_nodes * 3) return;
    const int n = i / 3, k = i - 3 * n;
    const bool fixed = ((int)cf.c[7] & CODLAD_DDPM_FIXED_VAR) != 0;
    x0_out[i] = ddpm_raw_x0(x[i], fixed ? out[n * 3 + k] : out[n * 6 + k], cf.c);
}

__global__ void ddpm_posterior_kernel(const float *x, const float *x0, const float *out, const float *noise,
                                      const float *grad, DdpmCoef cf, float fixed_variance, int n_nodes, float *x_out,
                                      float *x_start) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_nodes * 3) return;
    const int n = i / 3, k = i - 3 * n;
    const bool fixed = ((int)cf.c[7] & CODLAD_DDPM_FIXED_VAR) != 0;
    const float logvar = ddpm_log_variance(fixed ? 0.f : out[n * 6 + 3 + k], cf.c);
    // the variance that scales the gradient: exp(model_log_variance) for the learned range, the table value for
    // fixed variance (gaussian_diffusion.py:318, 320-334)
    const float variance = fixed ? fixed_variance : expf(logvar);
    x_out[i] = ddpm_posterior(x[i], x0[i], logvar, cf.c, noise[i], x_start ? x_start + i : nullptr,
                              grad ? grad + i : nullptr, variance);
}

// The DDIM update after a caller's denoised_fn / cond_fn (codlad_ddim_step): its first half is ddpm_pred_xstart_kernel,
// whose raw pred_xstart is ddim_step's; this is ddim_update, so a pin applied between them rounds as the fused one.
template <bool REVERSE>
__global__ void ddim_update_kernel(const float *x, const float *x0, const float *noise, const float *grad, DdpmCoef cf,
                                   int mode, int n_nodes, float *x_out, float *x_start) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_nodes * 3) return;
    x_out[i] = ddim_update<REVERSE>(x[i], x0[i], cf.c, mode, REVERSE ? 0.f : noise[i], x_start ? x_start + i : nullptr,
                                    grad ? grad + i : nullptr);
}

// ---------------------------------------------------------------------------------------------
// Timestep embedding + all adaLN heads, one workgroup per timestep (row 3).
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void mods_kernel(codlad_denoiser_weights w, const int64_t *tv, const float *tf,
                                                  float *mods) {
    __shared__ float emb[256];
    __shared__ float hid[HD];
    __shared__ float sc[HD];
    const int tid = threadIdx.x;
    const float t = tv ? (float)tv[blockIdx.x] : tf[blockIdx.x];   // latent_model.py:66: t[:, None].float() * freqs
    {
        const int k = tid & 127;
        const float arg = t * w.freqs[k];
        emb[tid] = tid < 128 ? cosf(arg) : sinf(arg);
    }
    __syncthreads();
    if (tid < HD) {
        float acc = 0.f;
        const float *wr = w.t_w0 + tid * 256;
        for (int k = 0; k < 256; ++k) acc = fmaf(emb[k], wr[k], acc);
        acc += w.t_b0[tid];
        hid[tid] = acc / (1.0f + expf(-acc));
    }
    __syncthreads();
    if (tid < HD) {
        float acc = 0.f;
        const float *wr = w.t_w2 + tid * HD;
        for (int k = 0; k < HD; ++k) acc = fmaf(hid[k], wr[k], acc);
        acc += w.t_b2[tid];
        sc[tid] = acc / (1.0f + expf(-acc));  // SiLU(c) feeds every adaLN head
    }
    __syncthreads();
    float *out = mods + (size_t)blockIdx.x * CODLAD_MODS_PER_STEP;
    int off = 0;
    for (int hd = 0; hd < 7; ++hd) {
        const int rows = hd < 3 ? 9 * HD : (hd < 6 ? 6 * HD : 2 * HD);
        for (int r = tid; r < rows; r += 256) {
            const float *wr = w.ada_w[hd] + (size_t)r * HD;
            float acc = 0.f;
            for (int k = 0; k < HD; ++k) acc = fmaf(sc[k], wr[k], acc);
            out[off + r] = acc + w.ada_b[hd][r];
        }
        off += rows;
    }
}

// ---------------------------------------------------------------------------------------------
// host launchers
// ---------------------------------------------------------------------------------------------
static inline int mods_offset(int head) {  // enc0..2, dec0..2, final
    return head < 3 ? head * 9 * HD : (head < 6 ? 27 * HD + (head - 3) * 6 * HD : 45 * HD);
}

static int g_num_cu = 0;

int num_cu() {
    if (!g_num_cu) {
        int dev = 0, n = 0;
        if (hipGetDevice(&dev) != hipSuccess ||
            hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0)
            n = 256;
        g_num_cu = n;
    }
    return g_num_cu;
}

// precision: 0 = fp32 MFMA, 1 = f16x4, 2 = f16x3 (include/codlad_hip.h)
// Raising a kernel's dynamic-LDS limit can fail (e.g. a device with less LDS than gfx950's 160 KB); the
// launch that follows would then fail with a less telling error, so the failure is kept for
// codlad_check_launch to report.
static hipError_t g_attr_error = hipSuccess;
void set_max_lds(const void *fn, size_t bytes) {
    const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (e != hipSuccess && g_attr_error == hipSuccess) g_attr_error = e;
}
hipError_t codlad_take_attr_error() {
    const hipError_t e = g_attr_error;
    g_attr_error = hipSuccess;
    return e;
}

// edge_tile_kernels.hip, edge_msg_kernel.hip, edge_upd_kernel.hip
void launch_edge_tile(int terms, bool update, const EdgeArgs &ea, const int2 *tile_list, int n_tiles, hipStream_t st);
void launch_edge_wide(int terms, bool update, const EdgeArgs &ea, const int2 *tile_list, int n_tiles, hipStream_t st);   // edge_wide_kernels.hip
int edge_wide_max_tiles();
void launch_edge_msg(int terms, const EdgeArgs &ea, hipStream_t st);
void launch_edge_upd(int terms, const EdgeArgs &ea, hipStream_t st);
void launch_edge_upd1(int terms, const EdgeArgs &ea, hipStream_t st);     // edge_upd1_kernel.hip: one wave per SIMD
int edge_upd_variant();

template <int TERMS>
static void launch_edge_h(bool update, const EdgeArgs &ea, const int2 *tile_list, int n_tiles, hipStream_t st) {
    if (tile_list && n_tiles <= edge_wide_max_tiles()) return launch_edge_wide(TERMS, update, ea, tile_list, n_tiles, st);
    if (tile_list) return launch_edge_tile(TERMS, update, ea, tile_list, n_tiles, st);
    if (update) {
        // upd1_kernel_h gives every node two tiles: worth it while (nearly) every node has two (n_tiles counts the
        // non-empty ones; 0 = the caller gave no tile list, i.e. nothing is known about the job)
        const bool two_tiles_each = n_tiles > 0 && 20ll * n_tiles >= 19ll * 2 * ea.n_nodes;
        if ((edge_upd_variant() == 1 && two_tiles_each) || edge_upd_variant() == 2) launch_edge_upd1(TERMS, ea, st);   // 2: always (tests)
        else launch_edge_upd(TERMS, ea, st);
    } else launch_edge_msg(TERMS, ea, st);
}

static void launch_edge_now(bool update, const EdgeArgs &ea, int precision, hipStream_t st, const int2 *tile_list,
                            int n_tiles) {
    if (precision == 2) return launch_edge_h<3>(update, ea, tile_list, n_tiles, st);
    if (precision == 1) return launch_edge_h<4>(update, ea, tile_list, n_tiles, st);
    dim3 grid((ea.n_nodes + 3) / 4), block(256);
    if (update) hipLaunchKernelGGL(edge_kernel<true>, grid, block, 0, st, ea);
    else hipLaunchKernelGGL(edge_kernel<false>, grid, block, 0, st, ea);
}

// Measurement aid (codlad_probe_edge_launches): while on, every edge-kernel launch of a forward is bracketed by a pair
// of HIP events on its own stream, so bench.py can quote the dominant kernel's duration as it runs inside the job
// (between node kernels, at the job's clock) rather than in a back-to-back loop of its own.
#define PROBE_MAX 4096
static struct {
    bool on = false;
    int used = 0;
    hipEvent_t ev[PROBE_MAX][2] = {};
    bool made[PROBE_MAX] = {};
    int kind[PROBE_MAX] = {};
} g_probe;

static void launch_edge(bool update, const EdgeArgs &ea, int precision, hipStream_t st, const int2 *tile_list = nullptr,
                        int n_tiles = 0) {
    const int i = g_probe.used;
    bool rec = g_probe.on && i < PROBE_MAX;
    if (rec && !g_probe.made[i]) {
        rec = hipEventCreate(&g_probe.ev[i][0]) == hipSuccess && hipEventCreate(&g_probe.ev[i][1]) == hipSuccess;
        g_probe.made[i] = rec;
    }
    if (rec) (void)hipEventRecord(g_probe.ev[i][0], st);
    launch_edge_now(update, ea, precision, st, tile_list, n_tiles);
    if (rec) {
        (void)hipEventRecord(g_probe.ev[i][1], st);
        g_probe.kind[i] = (update ? 1 : 0) + (ea.E1 ? 2 : 0);
        g_probe.used = i + 1;
    }
}

extern "C" int codlad_probe_edge_launches(int enable) {
    g_probe.on = enable != 0;
    if (enable) g_probe.used = 0;
    return 0;
}

extern "C" int codlad_probe_read(int kind, double *total_ms) {
    CODLAD_REQUIRE(total_ms && kind >= 0 && kind < 4, "bad arguments");
    double sum = 0.0;
    int n = 0;
    for (int i = 0; i < g_probe.used; ++i) {
        if (g_probe.kind[i] != kind) continue;
        float ms = 0.f;
        hipError_t e = hipEventSynchronize(g_probe.ev[i][1]);
        if (e == hipSuccess) e = hipEventElapsedTime(&ms, g_probe.ev[i][0], g_probe.ev[i][1]);
        if (e != hipSuccess) { codlad_set_error("codlad_probe_read: %s", hipGetErrorString(e)); return -(int)e - 1000; }
        sum += ms;
        ++n;
    }
    *total_ms = sum;
    return n;
}

// NW waves (32-node tiles) per workgroup, one workgroup per CU (LDS).  Four waves give every SIMD one
// tile and the most workgroups; a job with more tiles than 4 x CUs would then need a second, mostly
// empty round, and eight waves (two per SIMD, which overlap in this latency-bound kernel; a few
// dozen spilled registers) finish in one and stream every weight block once per 256 nodes.
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
    const int wgs = na.n_nodes >= XCD_CHUNKED_NODE_KERNEL_MIN ? 8 * (xcd_chunk_nodes(na.n_nodes) / (32 * NW))
                                                              : (na.n_nodes + 32 * NW - 1) / (32 * NW);
    dim3 grid(wgs), block(NW * 64);
    if (upd) hipLaunchKernelGGL((node_kernel_h<true, NW, TERMS>), grid, block, lds, st, na);
    else hipLaunchKernelGGL((node_kernel_h<false, NW, TERMS>), grid, block, lds, st, na);
}

// Jobs of up to CODLAD_NODEQ_MAX_TILES 32-node tiles take the quarter kernel (one tile per 4-wave workgroup).
static int g_options[CODLAD_N_OPTIONS] = {-1, -1, -1, -1, -1, -1, -1, -1, -1};
static int option_or(int opt, const char *env, int dflt) {
    if (g_options[opt] < 0) {
        const char *e = getenv(env);
        g_options[opt] = e ? atoi(e) : dflt;
    }
    return g_options[opt];
}
extern "C" int codlad_set_option(int option, int value) {
    CODLAD_REQUIRE(option >= 0 && option < CODLAD_N_OPTIONS && value >= 0, "unknown option or negative value");
    g_options[option] = value;
    return 0;
}
static int edge_tile_max_nodes() { return option_or(CODLAD_OPT_EDGE_TILE_MAX_NODES, "CODLAD_EDGE_TILE_MAX_NODES", 1 << 30); }
static int nodeq_max_tiles() { return option_or(CODLAD_OPT_NODEQ_MAX_TILES, "CODLAD_NODEQ_MAX_TILES", 256); }
int dec_edge_variant() { return option_or(CODLAD_OPT_DEC_EDGE_VARIANT, "CODLAD_DEC_EDGE_VARIANT", 0); }
int tp_conv_variant() { return option_or(CODLAD_OPT_TP_CONV_VARIANT, "CODLAD_TP_CONV_VARIANT", 0); }
int edge_upd_variant() { return option_or(CODLAD_OPT_EDGE_UPD_VARIANT, "CODLAD_EDGE_UPD_VARIANT", 0); }
// measured (tools/small_job_latency.py --sweep, k x 87 residues): the four-wave tile kernels win or tie up to ~5 600 tiles
// (2 800 nodes; 87 nodes 375 -> 254 us per step, 1 914 nodes 764 -> 594), beyond that the per-node kernels' reuse wins
int edge_wide_max_tiles() { return option_or(CODLAD_OPT_EDGE_WIDE_MAX_TILES, "CODLAD_EDGE_WIDE_MAX_TILES", 22 * num_cu()); }
int edge_cus() {
    const int v = option_or(CODLAD_OPT_EDGE_CUS, "CODLAD_EDGE_CUS", 0);
    return v > 0 && v < num_cu() ? v : num_cu();
}
// paired last tiles and cost-balanced XCD chunks in msg_kernel_h / upd_kernel_h (edge_args.h); 0: every node on its own, uniform chunks
static int edge_pair() { return option_or(CODLAD_OPT_EDGE_PAIR, "CODLAD_EDGE_PAIR", 1) != 0; }
static void set_edge_walk(EdgeArgs &ea, const codlad_workspace *ws) {
    ea.pair = edge_pair();
    ea.xcd_bounds = ea.pair ? ws->xcd_bounds : nullptr;
}

// The tile accounting of the per-node edge kernels on the host: the chunk bounds the kernels walk by and what the walk
// costs, from the same helpers (edge_args.h) the kernels decide with.
// Tiles the waves of one XCD run on nodes lo .. hi - 1 (wave w: lo + w, lo + w + stride, ...), and the pairs they form.
static int64_t chunk_walk(const int32_t *K, int lo, int hi, int stride, bool pair, int64_t *pairs) {
    int64_t tiles = 0;
    for (int w = 0; w < stride; ++w)
        for (int n = lo + w; n < hi; n += stride) {
            tiles += K[n] > 32 ? 2 : 1;
            if (pair && n + stride < hi && edge_pair_ok(K[n], K[n + stride])) {
                n += stride;                     // the second node: its tiles, less the one the two share
                tiles += (K[n] > 32 ? 2 : 1) - 1;
                if (pairs) ++*pairs;
            }
        }
    return tiles;
}

extern "C" int codlad_edge_plan_host(const int32_t *K_host, int n_nodes, int n_workgroups, int waves_per_workgroup,
                                     int pair, int32_t *bounds_host, int64_t *stats_host) {
    CODLAD_REQUIRE(K_host && n_nodes > 0 && n_workgroups > 0 && waves_per_workgroup > 0, "bad arguments");
    int32_t bounds[9];
    const int G = XCD_BOUND_GRANULE, ng = (n_nodes + G - 1) / G;
    std::vector<int64_t> upto(ng + 1, 0);       // half tiles of the cost model up to each granule boundary
    int64_t plain = 0;
    for (int n = 0; n < n_nodes; ++n) {
        CODLAD_REQUIRE(K_host[n] >= 1 && K_host[n] <= 64, "K outside 1..64");
        plain += K_host[n] > 32 ? 2 : 1;
        upto[n / G + 1] += pair ? edge_node_cost2(K_host[n]) : (K_host[n] > 32 ? 4 : 2);
    }
    for (int g = 0; g < ng; ++g) upto[g + 1] += upto[g];
    const int64_t total = upto[ng];
    const bool chunked = n_workgroups % 8 == 0;
    const int stride = chunked ? n_workgroups / 8 * waves_per_workgroup : n_workgroups * waves_per_workgroup;
    auto node_of = [&](int g) { return g * G < n_nodes ? g * G : n_nodes; };
    if (pair) {
        // Bound x: the granule boundary where the tiles walked so far are nearest to x eighths of the total, so that a
        // chunk misses the mean by less than one granule.  What a chunk costs is what its waves walk: a wave pairs the
        // eligible nodes it meets in a row and an odd one out costs two tiles, not the 1.5 of the cost model, which
        // therefore only gives the first guess (and the whole answer for a grid that is not dealt over the XCDs).
        double target = total / 16.0;
        for (int pass = 0; pass < (chunked ? 3 : 1); ++pass) {
            bounds[0] = 0;
            int g = 0;
            int64_t done = 0;               // tiles of the chunks closed so far
            for (int x = 1; x < 8; ++x) {
                const int g0 = g;
                if (pass == 0) {
                    while (g < ng && 8 * upto[g + 1] <= total * x) ++g;          // upto[g] <= target < upto[g + 1]
                    if (g < ng && 8 * upto[g + 1] - total * x < total * x - 8 * upto[g]) ++g;
                } else {
                    auto f = [&](int gg) { return (double)(done + chunk_walk(K_host, node_of(g0), node_of(gg), stride, true, nullptr)); };
                    const double want = target * x;
                    while (g < ng && f(g) < want) ++g;
                    while (g > g0 && f(g - 1) >= want) --g;                     // f(g - 1) < want <= f(g)
                    if (g > g0 && want - f(g - 1) < f(g) - want) --g;
                }
                bounds[x] = node_of(g);
                if (chunked) done += chunk_walk(K_host, node_of(g0), node_of(g), stride, true, nullptr);
            }
            bounds[8] = n_nodes;
            if (chunked) target = (done + chunk_walk(K_host, bounds[7], n_nodes, stride, true, nullptr)) / 8.0;
        }
    } else {
        const int chunk = xcd_chunk_nodes(n_nodes);
        for (int x = 0; x <= 8; ++x) bounds[x] = (int64_t)x * chunk < n_nodes ? x * chunk : n_nodes;
    }
    if (bounds_host)
        for (int x = 0; x <= 8; ++x) bounds_host[x] = bounds[x];
    if (stats_host) {
        int64_t walk = 0, pairs = 0;
        for (int x = 0; x < 8; ++x) {
            const int lo = (bounds[x] + G - 1) / G, hi = (bounds[x + 1] + G - 1) / G;
            stats_host[4 + x] = upto[hi] - upto[lo];
            stats_host[12 + x] = chunked ? chunk_walk(K_host, bounds[x], bounds[x + 1], stride, pair != 0, &pairs) : 0;
            walk += stats_host[12 + x];
        }
        if (!chunked) walk = chunk_walk(K_host, 0, n_nodes, stride, pair != 0, &pairs);
        stats_host[0] = plain;
        stats_host[1] = total;
        stats_host[2] = walk;
        stats_host[3] = pairs;
    }
    return 0;
}

// node_wide_kernels.hip, node_quad_kernels.hip
void launch_node_wide(int terms, bool upd, const NodeArgs &na, hipStream_t st);
void launch_node_quad(int terms, const NodeArgs &na, hipStream_t st);
// measured: 87 nodes 202 -> 182 us per step, the cfg-3 shard 476 -> 448, all of cfg 3 (411 tiles, two rounds) 2 316 -> 2 281;
// cfg 2's half-jobs (553 tiles) lose 1.3 % against the streaming kernel, which reads every block once per 4-8 tiles
static int node_quad_max_tiles() { return option_or(CODLAD_OPT_NODE_QUAD_MAX_TILES, "CODLAD_NODE_QUAD_MAX_TILES", 2 * num_cu()); }

template <int TERMS>
static void launch_node_h(bool upd, const NodeArgs &na, hipStream_t st) {
    const int tiles = (na.n_nodes + 31) / 32;
    if (upd && tiles <= node_quad_max_tiles()) launch_node_quad(TERMS, na, st);
    else if (tiles <= nodeq_max_tiles()) launch_node_wide(TERMS, upd, na, st);
    else if (tiles > 4 * num_cu()) launch_node_hw<TERMS, 8>(upd, na, st);
    else launch_node_hw<TERMS, 4>(upd, na, st);
}

static void launch_node(bool upd, const NodeArgs &na, int precision, hipStream_t st) {
    if (precision == 2) return launch_node_h<3>(upd, na, st);
    if (precision == 1) return launch_node_h<4>(upd, na, st);
    dim3 grid((na.n_nodes + 31) / 32), block(64);
    if (upd) hipLaunchKernelGGL(node_kernel<true>, grid, block, 0, st, na);
    else hipLaunchKernelGGL(node_kernel<false>, grid, block, 0, st, na);
}

// Everything an edge / node launch needs that depends on the contraction mode: in the split-fp16 modes the
// biases are the pre-scaled copies and the block exponents become scale constants (include/codlad_hip.h).
static void set_msg_scales(EdgeArgs &ea, bool split, const float *b2, const float *b2h, int e1, int e2) {
    ea.b2 = split ? b2h : b2;
    ea.gelu_a = gelu_consts(split ? e1 : 0);
    ea.gelu_b = gelu_consts(split ? e1 + e2 : 0);
    ea.res_scale = 1.0f; ea.ln_eps = 1e-6f;
}
static void set_upd_scales(EdgeArgs &eu, bool split, const codlad_enc_layer &L, const codlad_enc_layer_h &Lh) {
    eu.b2 = split ? Lh.b12 : L.b12; eu.b3 = split ? Lh.b13 : L.b13;
    const int E2 = split ? Lh.e11 + Lh.e12 : 0, E3 = split ? E2 + Lh.e13 : 0;
    eu.gelu_a = gelu_consts(split ? Lh.e11 : 0);
    eu.gelu_b = gelu_consts(E2);
    eu.res_scale = pow2i(E3);
    eu.ln_eps = 1e-6f * pow2i(2 * E3);
}
// node update that follows a message kernel with accumulated exponent e_msg = e1 + e2
static void set_node_scales(NodeArgs &na, bool split, int e_msg, int e3, int e_in, int e_out) {
    na.s_scale = 0.015625f * pow2i(split ? -e_msg : 0);
    na.t_scale = 64.0f * pow2i(split ? -e3 : 0);
    na.ffn_scale = pow2i(split ? -(e_in + e_out) : 0);
    na.gelu_ffn = gelu_consts(split ? e_in : 0);
}

// One denoiser forward up to (not including) the final layer: leaves h_V in ws->hV.
static void enqueue_forward(const codlad_denoiser_weights *w, const int32_t *node_info,
                            int n_nodes, const int32_t *E_idx, const float *h_E0, const float *E1,
                            size_t n_snodes, const float *x, const float *x_self_cond, const float *mods_t,
                            const codlad_workspace *ws, hipStream_t st) {
    const int4 *ni = reinterpret_cast<const int4 *>(node_info);
    const size_t NS = (size_t)n_nodes * HD;
    float *PQ0 = ws->PQ, *PQ1 = ws->PQ + NS, *PQ2 = ws->PQ + 2 * NS, *PQ3 = ws->PQ + 3 * NS;
    const bool split = w->precision != 0;
    // small jobs: edge kernels per 32-edge tile, message sums per half (S[2][n_nodes][128])
    // (while every wave of the persistent grid gets at most one tile: beyond that the per-node order is as good)
    const bool tilewise = split && ws->tile_list && ws->n_tiles > 0 &&
                          (ws->n_tiles <= 8 * num_cu() || ws->n_tiles <= edge_wide_max_tiles()) &&
                          n_nodes <= edge_tile_max_nodes();
    const int2 *tile_list = tilewise ? reinterpret_cast<const int2 *>(ws->tile_list) : nullptr;

    // h_V = x_in(x); P/Q for encoder layer 0's message
    {
        NodeArgs na = {};
        na.node_info = ni; na.n_nodes = n_nodes;
        na.x = x; na.x_in_w = w->x_in_w; na.x_in_b = w->x_in_b; na.hV = ws->hV;
        na.x_sc = x_self_cond; na.in_dim = w->self_condition ? 6 : 3;
        na.n_proj = 2;
        na.proj_w[0] = w->enc[0].W1a; na.proj_b[0] = split ? w->enc_h[0].b1 : w->enc[0].b1; na.proj_out[0] = PQ0;
        na.proj_w[1] = w->enc[0].W1c; na.proj_b[1] = nullptr;      na.proj_out[1] = PQ1;
        na.blk_h[0] = w->enc_h[0].W1a; na.blk_h[1] = w->enc_h[0].W1c;
        set_node_scales(na, split, 0, 0, 0, 0);
        launch_node(false, na, w->precision, st);
    }
    for (int l = 0; l < 3; ++l) {
        const codlad_enc_layer &L = w->enc[l];
        const codlad_enc_layer_h &Lh = w->enc_h[l];
        const float *m = mods_t + mods_offset(l);
        EdgeArgs ea = {};
        ea.node_info = ni; ea.E_idx = E_idx; ea.n_nodes = n_nodes;
        ea.hE_in = l == 0 ? h_E0 : ws->hE; ea.in_by_src = l == 0;
        ea.P = PQ0; ea.Q = PQ1; ea.W1 = L.W1e; ea.W2 = L.W2; ea.S = ws->S;
        ea.W1h = Lh.W1e; ea.W2h = Lh.W2;
        set_msg_scales(ea, split, L.b2, Lh.b2, Lh.e1, Lh.e2);
        set_edge_walk(ea, ws);
        if (l == 0 && E1) ea.E1 = E1;
        launch_edge(false, ea, w->precision, st, tile_list, ws->n_tiles);

        NodeArgs na = {};
        na.node_info = ni; na.n_nodes = n_nodes; na.S = ws->S; na.hV = ws->hV;
        na.W3 = L.W3; na.b3 = split ? Lh.b3 : L.b3; na.mods = m;
        for (int c = 0; c < 4; ++c) { na.Win[c] = L.Win[c]; na.Wout[c] = L.Wout[c]; }
        na.b_in = split ? Lh.b_in : L.b_in; na.b_out = split ? Lh.b_out : L.b_out;
        set_node_scales(na, split, Lh.e1 + Lh.e2, Lh.e3, Lh.e_in, Lh.e_out);
        na.s_partials = tilewise;
        na.n_proj = 4;
        na.proj_w[0] = L.W11a; na.proj_b[0] = split ? Lh.b11 : L.b11; na.proj_out[0] = PQ2;   // edge update P
        na.proj_w[1] = L.W11c; na.proj_b[1] = nullptr;                 na.proj_out[1] = PQ3;   // edge update Q
        if (l < 2) {
            na.proj_w[2] = w->enc[l + 1].W1a; na.proj_b[2] = split ? w->enc_h[l + 1].b1 : w->enc[l + 1].b1; na.proj_out[2] = PQ0;
            na.proj_w[3] = w->enc[l + 1].W1c; na.proj_b[3] = nullptr;          na.proj_out[3] = PQ1;
        } else {
            // first decoder layer: h_Venc := this h_V, so its neighbour term sees 2*h_V
            na.proj_w[2] = w->dec[0].W1a; na.proj_b[2] = split ? w->dec_h[0].b1 : w->dec[0].b1; na.proj_out[2] = PQ0;
            na.proj_w[3] = w->dec[0].W1v; na.proj_b[3] = nullptr;      na.proj_out[3] = PQ1;
            na.proj_flags[3] = 3; na.TS = split ? w->dec_h[0].TS : w->dec[0].TS;
            na.hVenc_out = ws->hVenc; na.venc_is_self = 1;
        }
        {
            int k = 0;
            na.blk_h[k++] = Lh.W3;
            for (int c = 0; c < 4; ++c) { na.blk_h[k++] = Lh.Win[c]; na.blk_h[k++] = Lh.Wout[c]; }
            na.blk_h[k++] = Lh.W11a; na.blk_h[k++] = Lh.W11c;
            if (l < 2) { na.blk_h[k++] = w->enc_h[l + 1].W1a; na.blk_h[k++] = w->enc_h[l + 1].W1c; }
            else { na.blk_h[k++] = w->dec_h[0].W1a; na.blk_h[k++] = w->dec_h[0].W1v; }
        }
        launch_node(true, na, w->precision, st);

        EdgeArgs eu = {};
        eu.node_info = ni; eu.E_idx = E_idx; eu.n_nodes = n_nodes;
        eu.hE_in = l == 0 ? h_E0 : ws->hE; eu.in_by_src = l == 0; eu.hE_out = ws->hE;
        eu.P = PQ2; eu.Q = PQ3; eu.W1 = L.W11e; eu.W2 = L.W12; eu.W3 = L.W13;
        eu.mods3 = m + 6 * HD;
        eu.W1h = Lh.W11e; eu.W2h = Lh.W12; eu.W3h = Lh.W13;
        set_upd_scales(eu, split, L, Lh);
        set_edge_walk(eu, ws);
        if (l == 0 && E1) eu.E1 = E1 + n_snodes * 64 * HD;
        launch_edge(true, eu, w->precision, st, tile_list, ws->n_tiles);
    }
    for (int l = 0; l < 3; ++l) {
        const codlad_dec_layer &L = w->dec[l];
        const codlad_dec_layer_h &Lh = w->dec_h[l];
        EdgeArgs ea = {};
        ea.node_info = ni; ea.E_idx = E_idx; ea.n_nodes = n_nodes;
        ea.hE_in = ws->hE; ea.in_by_src = 0;
        ea.P = PQ0; ea.Q = PQ1; ea.W1 = L.W1e; ea.W2 = L.W2; ea.S = ws->S;
        ea.W1h = Lh.W1e; ea.W2h = Lh.W2;
        set_msg_scales(ea, split, L.b2, Lh.b2, Lh.e1, Lh.e2);
        set_edge_walk(ea, ws);
        launch_edge(false, ea, w->precision, st, tile_list, ws->n_tiles);

        NodeArgs na = {};
        na.node_info = ni; na.n_nodes = n_nodes; na.S = ws->S; na.hV = ws->hV; na.s_partials = tilewise;
        na.W3 = L.W3; na.b3 = split ? Lh.b3 : L.b3; na.mods = mods_t + mods_offset(3 + l);
        for (int c = 0; c < 4; ++c) { na.Win[c] = L.Win[c]; na.Wout[c] = L.Wout[c]; }
        na.b_in = split ? Lh.b_in : L.b_in; na.b_out = split ? Lh.b_out : L.b_out;
        set_node_scales(na, split, Lh.e1 + Lh.e2, Lh.e3, Lh.e_in, Lh.e_out);
        if (l < 2) {
            na.n_proj = 2;
            na.proj_w[0] = w->dec[l + 1].W1a; na.proj_b[0] = split ? w->dec_h[l + 1].b1 : w->dec[l + 1].b1; na.proj_out[0] = PQ0;
            na.proj_w[1] = w->dec[l + 1].W1v; na.proj_b[1] = nullptr;          na.proj_out[1] = PQ1;
            na.proj_flags[1] = 3; na.TS = split ? w->dec_h[l + 1].TS : w->dec[l + 1].TS; na.hVenc_in = ws->hVenc;
        }
        {
            int k = 0;
            na.blk_h[k++] = Lh.W3;
            for (int c = 0; c < 4; ++c) { na.blk_h[k++] = Lh.Win[c]; na.blk_h[k++] = Lh.Wout[c]; }
            if (l < 2) { na.blk_h[k++] = w->dec_h[l + 1].W1a; na.blk_h[k++] = w->dec_h[l + 1].W1v; }
        }
        launch_node(true, na, w->precision, st);
    }
}

static int check_ws(const codlad_workspace *ws) {
    return ws && ws->hV && ws->hVenc && ws->S && ws->PQ && ws->hE;
}

extern "C" int codlad_step_mods(const codlad_denoiser_weights *w, const int64_t *t_values, int n_t,
                                float *mods, void *stream) {
    CODLAD_REQUIRE(w && t_values && mods, "null pointer");
    CODLAD_REQUIRE(n_t > 0, "n_t must be positive");
    hipLaunchKernelGGL(mods_kernel, dim3(n_t), dim3(256), 0, (hipStream_t)stream, *w, t_values, (const float *)nullptr, mods);
    return codlad_check_launch("codlad_step_mods");
}

extern "C" int codlad_step_mods_f(const codlad_denoiser_weights *w, const float *t_values, int n_t, float *mods,
                                  void *stream) {
    CODLAD_REQUIRE(w && t_values && mods, "null pointer");
    CODLAD_REQUIRE(n_t > 0, "n_t must be positive");
    hipLaunchKernelGGL(mods_kernel, dim3(n_t), dim3(256), 0, (hipStream_t)stream, *w, (const int64_t *)nullptr, t_values, mods);
    return codlad_check_launch("codlad_step_mods_f");
}


extern "C" int codlad_denoiser_forward(const codlad_denoiser_weights *w, const int32_t *node_info,
                                       int n_nodes, const int32_t *E_idx, const float *h_E0,
                                       const float *E1, int n_snodes, const float *x,
                                       const float *x_self_cond, const float *mods_t, float *out,
                                       const codlad_workspace *ws, void *stream) {
    CODLAD_REQUIRE(w && node_info && E_idx && h_E0 && x && mods_t && out, "null pointer");
    CODLAD_REQUIRE(check_ws(ws), "incomplete workspace");
    CODLAD_REQUIRE(n_nodes > 0, "n_nodes must be positive");
    hipStream_t st = (hipStream_t)stream;
    CODLAD_REQUIRE(!x_self_cond || w->self_condition, "x_self_cond given to a model without self-conditioning");
    CODLAD_REQUIRE(w->out_dim == 6 || w->out_dim == 3, "out_dim must be 6 (diffusion) or 3 (flow matching)");
    enqueue_forward(w, node_info, n_nodes, E_idx, h_E0, E1, (size_t)n_snodes, x, x_self_cond, mods_t, ws, st);
    FinalArgs fa = {};
    fa.hV = ws->hV; fa.mods = mods_t + mods_offset(6); fa.out_w = w->out_w; fa.out_b = w->out_b;
    fa.n_nodes = n_nodes; fa.logits = out; fa.status = ws->status; fa.n_out = w->out_dim;
    hipLaunchKernelGGL(final_kernel<false>, dim3((n_nodes + 7) / 8), dim3(256), 0, st, fa, nullptr, nullptr, 0);
    return codlad_check_launch("codlad_denoiser_forward");
}

extern "C" int codlad_ddpm_update(const float *x, const float *model_out, const float *noise,
                                  const float *coef_host, int n_nodes, float *x_out, float *x_start_out,
                                  void *stream) {
    CODLAD_REQUIRE(x && model_out && noise && coef_host && x_out, "null pointer");
    CODLAD_REQUIRE(n_nodes > 0, "n_nodes must be positive");
    DdpmCoef cf;
    for (int k = 0; k < 8; ++k) cf.c[k] = coef_host[k];
    hipLaunchKernelGGL(ddpm_kernel, dim3((n_nodes * 3 + 255) / 256), dim3(256), 0,
                       (hipStream_t)stream, x, model_out, noise, cf, n_nodes, x_out, x_start_out);
    return codlad_check_launch("codlad_ddpm_update");
}

extern "C" int codlad_ddpm_pred_xstart(const float *x, const float *model_out, const float *coef_host, int n_nodes,
                                      float *pred_xstart, void *stream) {
    CODLAD_REQUIRE(x && model_out && coef_host && pred_xstart, "null pointer");
    CODLAD_REQUIRE(n_nodes > 0, "n_nodes must be positive");
    DdpmCoef cf;
    for (int k = 0; k < 8; ++k) cf.c[k] = coef_host[k];
    hipLaunchKernelGGL(ddpm_pred_xstart_kernel, dim3((n_nodes * 3 + 255) / 256), dim3(256), 0, (hipStream_t)stream, x,
                       model_out, cf, n_nodes, pred_xstart);
    return codlad_check_launch("codlad_ddpm_pred_xstart");
}

extern "C" int codlad_ddpm_posterior_step(const float *x, const float *pred_xstart, const float *model_out,
                                          const float *noise, const float *grad, const float *coef_host,
                                          float fixed_variance, int n_nodes, float *x_out, float *x_start_out,
                                          void *stream) {
    CODLAD_REQUIRE(x && pred_xstart && model_out && noise && coef_host && x_out, "null pointer");
    CODLAD_REQUIRE(n_nodes > 0, "n_nodes must be positive");
    DdpmCoef cf;
    for (int k = 0; k < 8; ++k) cf.c[k] = coef_host[k];
    hipLaunchKernelGGL(ddpm_posterior_kernel, dim3((n_nodes * 3 + 255) / 256), dim3(256), 0, (hipStream_t)stream, x,
                       pred_xstart, model_out, noise, grad, cf, fixed_variance, n_nodes, x_out, x_start_out);
    return codlad_check_launch("codlad_ddpm_posterior_step");
}

// the loop of codlad_sample_loop / codlad_sample_loop_pinned / codlad_ddim_loop (pin_x0 == NULL: no pinning).
// step: CODLAD_STEP_* of final_kernel; `mode` is read by the DDIM steps only.  The forward loops run i = T-1 .. 0 and
// consume noise entry k at step k; the reverse DDIM loop runs i = 0 .. T-1 and reads no noise.
static int sample_loop(const codlad_denoiser_weights *w, const int32_t *node_info, int n_nodes, const int32_t *E_idx,
                       const float *h_E0, const float *E1, int n_snodes, float *x, float *x_start, const float *noise,
                       const float *mods, const float *coef, int T, const float *pin_x0, const uint8_t *pin_mask,
                       const codlad_workspace *ws, void *stream, int step = CODLAD_STEP_DDPM, int mode = 0) {
    hipStream_t st = (hipStream_t)stream;
    // self-conditioning (gaussian_diffusion.py:530-547): step k reads the pred_xstart step k-1 wrote;
    // the first step gets none, which the model treats as zeros (latent_model.py:211)
    const bool sc = w->self_condition != 0;
    const bool reverse = step == CODLAD_STEP_DDIM_REVERSE;
    for (int k = 0; k < T; ++k) {
        const int i = reverse ? k : T - 1 - k;
        const float *mods_t = mods + (size_t)i * CODLAD_MODS_PER_STEP;
        enqueue_forward(w, node_info, n_nodes, E_idx, h_E0, E1, (size_t)n_snodes, x, sc && k > 0 ? x_start : nullptr,
                        mods_t, ws, st);
        FinalArgs fa = {};
        fa.hV = ws->hV; fa.mods = mods_t + mods_offset(6); fa.out_w = w->out_w; fa.out_b = w->out_b;
        fa.n_nodes = n_nodes; fa.x = x; fa.noise = reverse ? nullptr : noise + (size_t)k * n_nodes * 3;
        fa.coef = coef + (size_t)i * 8; fa.x_start = x_start; fa.status = ws->status; fa.n_out = w->out_dim;
        const dim3 grid((n_nodes + 7) / 8);
        if (step == CODLAD_STEP_DDIM) {
            if (pin_x0)
                hipLaunchKernelGGL((final_kernel<true, CODLAD_STEP_DDIM>), grid, dim3(256), 0, st, fa, pin_x0, pin_mask, mode);
            else
                hipLaunchKernelGGL((final_kernel<false, CODLAD_STEP_DDIM>), grid, dim3(256), 0, st, fa, nullptr, nullptr, mode);
        } else if (reverse) {
            if (pin_x0)
                hipLaunchKernelGGL((final_kernel<true, CODLAD_STEP_DDIM_REVERSE>), grid, dim3(256), 0, st, fa, pin_x0,
                                   pin_mask, mode);
            else
                hipLaunchKernelGGL((final_kernel<false, CODLAD_STEP_DDIM_REVERSE>), grid, dim3(256), 0, st, fa, nullptr,
                                   nullptr, mode);
        } else if (pin_x0) {
            hipLaunchKernelGGL(final_kernel<true>, dim3((n_nodes + 7) / 8), dim3(256), 0, st, fa, pin_x0, pin_mask, 0);
        } else {
            hipLaunchKernelGGL(final_kernel<false>, dim3((n_nodes + 7) / 8), dim3(256), 0, st, fa, nullptr, nullptr, 0);
        }
    }
    return 0;
}

#define SAMPLE_LOOP_REQUIRE()                                                                                          \
    CODLAD_REQUIRE(w && node_info && E_idx && h_E0 && x && noise && mods && coef, "null pointer");                     \
    CODLAD_REQUIRE(check_ws(ws), "incomplete workspace");                                                             \
    CODLAD_REQUIRE(n_nodes > 0 && T > 0, "n_nodes and T must be positive");                                           \
    CODLAD_REQUIRE(!w->self_condition || x_start, "a self-conditioned model needs the x_start buffer");               \
    CODLAD_REQUIRE(w->out_dim == 6 || w->out_dim == 3,                                                                \
                   "the DDPM loop needs a model with 6 outputs (mean | variance logits) or 3 (fixed-variance samplers)")

extern "C" int codlad_sample_loop(const codlad_denoiser_weights *w, const int32_t *node_info,
                                  int n_nodes, const int32_t *E_idx, const float *h_E0,
                                  const float *E1, int n_snodes, float *x, float *x_start,
                                  const float *noise, const float *mods, const float *coef, int T,
                                  const codlad_workspace *ws, void *stream) {
    SAMPLE_LOOP_REQUIRE();
    sample_loop(w, node_info, n_nodes, E_idx, h_E0, E1, n_snodes, x, x_start, noise, mods, coef, T, nullptr, nullptr, ws,
                stream);
    return codlad_check_launch("codlad_sample_loop");
}

extern "C" int codlad_sample_loop_pinned(const codlad_denoiser_weights *w, const int32_t *node_info,
                                         int n_nodes, const int32_t *E_idx, const float *h_E0,
                                         const float *E1, int n_snodes, float *x, float *x_start,
                                         const float *noise, const float *mods, const float *coef, int T,
                                         const float *pin_x0, const uint8_t *pin_mask,
                                         const codlad_workspace *ws, void *stream) {
    SAMPLE_LOOP_REQUIRE();
    CODLAD_REQUIRE(pin_x0 && pin_mask, "null pointer (pin_x0 / pin_mask)");
    sample_loop(w, node_info, n_nodes, E_idx, h_E0, E1, n_snodes, x, x_start, noise, mods, coef, T, pin_x0, pin_mask, ws,
                stream);
    return codlad_check_launch("codlad_sample_loop_pinned");
}
#undef SAMPLE_LOOP_REQUIRE

extern "C" int codlad_ddim_loop(const codlad_denoiser_weights *w, const int32_t *node_info, int n_nodes,
                                const int32_t *E_idx, const float *h_E0, const float *E1, int n_snodes, float *x,
                                float *x_start, const float *noise, const float *mods, const float *coef, int T, int mode,
                                int reverse, const float *pin_x0, const uint8_t *pin_mask, const codlad_workspace *ws,
                                void *stream) {
    CODLAD_REQUIRE(w && node_info && E_idx && h_E0 && x && mods && coef, "null pointer");
    CODLAD_REQUIRE(reverse || noise, "null pointer (noise: only the reverse loop runs without it)");
    CODLAD_REQUIRE(!pin_x0 == !pin_mask, "null pointer (pin_x0 and pin_mask come together)");
    CODLAD_REQUIRE(n_nodes > 0 && T > 0, "n_nodes and T must be positive");
    CODLAD_REQUIRE(mode >= 0 && mode <= (CODLAD_DDPM_START_X | CODLAD_DDPM_FIXED_VAR | CODLAD_DDPM_CLIP),
                   "unknown mode bits");
    CODLAD_REQUIRE(w->out_dim == ((mode & CODLAD_DDPM_FIXED_VAR) ? 3 : 6),
                   "mode and model disagree: a learned-range sampler needs a model with 6 outputs (mean | variance "
                   "logits), a fixed-variance one (mode bit 2) a model with 3");
    CODLAD_REQUIRE(!w->self_condition || x_start, "a self-conditioned model needs the x_start buffer");
    CODLAD_REQUIRE(check_ws(ws), "incomplete workspace");
    sample_loop(w, node_info, n_nodes, E_idx, h_E0, E1, n_snodes, x, x_start, noise, mods, coef, T, pin_x0, pin_mask, ws,
                stream, reverse ? CODLAD_STEP_DDIM_REVERSE : CODLAD_STEP_DDIM, mode);
    return codlad_check_launch("codlad_ddim_loop");
}

extern "C" int codlad_ddim_step(const float *x, const float *pred_xstart, const float *noise, const float *grad,
                                const float *coef_host, int reverse, int n_nodes, float *x_out, float *x_start_out,
                                void *stream) {
    CODLAD_REQUIRE(x && pred_xstart && coef_host && x_out, "null pointer");
    CODLAD_REQUIRE(reverse || noise, "null pointer (noise: only the reverse step runs without it)");
    CODLAD_REQUIRE(n_nodes > 0, "n_nodes must be positive");
    DdpmCoef cf;
    for (int k = 0; k < 8; ++k) cf.c[k] = coef_host[k];
    const int mode = (int)coef_host[7];
    const dim3 grid((n_nodes * 3 + 255) / 256);
    if (reverse)
        hipLaunchKernelGGL(ddim_update_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, x, pred_xstart, nullptr,
                           grad, cf, mode, n_nodes, x_out, x_start_out);
    else
        hipLaunchKernelGGL(ddim_update_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, x, pred_xstart, noise,
                           grad, cf, mode, n_nodes, x_out, x_start_out);
    return codlad_check_launch("codlad_ddim_step");
}

extern "C" int codlad_status_check(int32_t *status, void *stream) {
    CODLAD_REQUIRE(status, "null pointer");
    int32_t host = 0;
    hipStream_t st = (hipStream_t)stream;
    hipError_t e = hipMemcpyAsync(&host, status, sizeof(host), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e == hipSuccess && host) e = hipMemsetAsync(status, 0, sizeof(host), st);
    if (e != hipSuccess) {
        codlad_set_error("codlad_status_check: %s", hipGetErrorString(e));
        return (int)e;
    }
    if (host & CODLAD_STATUS_NONFINITE) {
        codlad_set_error("denoiser output is not finite: an input, a weight or - in the split-fp16 contraction "
                         "modes - an operand beyond the fp16 range (|x| > 65504) overflowed; rerun with precision f32 to tell them apart");
        return CODLAD_E_NONFINITE;
    }
    return 0;
}

// Hoisted layer-0 edge terms: W1e(enc 0) @ h_E0 and W11e(enc 0) @ h_E0 per structure edge.  h_E0
// depends on the CA trace only, so these two contractions are the same in every step and for every
// ensemble member of a frame; the layer-0 kernels then start from acc = P_i + Q_j + E1[edge].
struct Layer0Args {
    const int2 *snode_info;
    const float *hE0;
    const float *W_msg, *W_upd;      // fp32-packed
    const void *Wh_msg, *Wh_upd;     // split-fp16 packed
    float *E1;                       // [2][n_snodes][64][128]
    int n_snodes;
};

template <int TERMS>   // 0: fp32 MFMA, 3 / 4: split fp16
__global__ __launch_bounds__(256, 1) void layer0_kernel(Layer0Args a) {
    const int lane = threadIdx.x & 63, h = lane >> 5, c = lane & 31;
    const int m = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (m >= a.n_snodes) return;
    const int L = a.snode_info[m].y, K = L < 64 ? L : 64;
    for (int half = 0; half < 2; ++half) {
        if (32 * half >= K) break;
        const int col = 32 * half + c;
        const bool valid = col < K;
        const int colc = valid ? col : 0;
        Tile x;
        tile_load_edge(x, a.hE0 + (size_t)m * EDGE_BLOCK, colc, h);
#pragma unroll 1
        for (int which = 0; which < 2; ++which) {
            Tile acc;
            tile_zero(acc);
            if constexpr (TERMS != 0) gemm_h_glb<TERMS, 0, 8, false, true>(acc, x, which ? a.Wh_upd : a.Wh_msg, lane, gelu_consts(0));   // h_E0 as stored (pre-split)
            else gemm128(acc, x, which ? a.W_upd : a.W_msg, lane);
            if (valid) tile_store_edge(acc, a.E1 + ((size_t)which * a.n_snodes + m) * EDGE_BLOCK, col, h);
        }
    }
}

extern "C" int codlad_layer0_edge_terms(const codlad_denoiser_weights *w, const int32_t *snode_info,
                                        int n_snodes, const float *h_E0, float *E1, void *stream) {
    CODLAD_REQUIRE(w && snode_info && h_E0 && E1 && n_snodes > 0, "bad arguments");
    Layer0Args a = {};
    a.snode_info = reinterpret_cast<const int2 *>(snode_info); a.hE0 = h_E0; a.E1 = E1; a.n_snodes = n_snodes;
    a.W_msg = w->enc[0].W1e; a.W_upd = w->enc[0].W11e;
    a.Wh_msg = w->enc_h[0].W1e; a.Wh_upd = w->enc_h[0].W11e;
    dim3 grid((n_snodes + 3) / 4), block(256);
    if (w->precision == 2) hipLaunchKernelGGL(layer0_kernel<3>, grid, block, 0, (hipStream_t)stream, a);
    else if (w->precision == 1) hipLaunchKernelGGL(layer0_kernel<4>, grid, block, 0, (hipStream_t)stream, a);
    else hipLaunchKernelGGL(layer0_kernel<0>, grid, block, 0, (hipStream_t)stream, a);
    return codlad_check_launch("codlad_layer0_edge_terms");
}

// Single launch of one of the two edge kernels on encoder layer 0 (reads h_E0 and the P/Q left by
// a previous forward; idempotent) - lets bench.py time the dominant kernel with HIP events.
extern "C" int codlad_bench_edge_launch(const codlad_denoiser_weights *w, const int32_t *node_info,
                                        int n_nodes, const int32_t *E_idx, const float *h_E0,
                                        const float *mods_t, const codlad_workspace *ws, int which,
                                        int layer, void *stream) {
    CODLAD_REQUIRE(w && node_info && E_idx && h_E0 && mods_t, "null pointer");
    CODLAD_REQUIRE(check_ws(ws), "incomplete workspace");
    CODLAD_REQUIRE(n_nodes > 0 && (which == 0 || which == 1) && (layer == 0 || layer == 1), "bad arguments");
    const size_t NS = (size_t)n_nodes * HD;
    const codlad_enc_layer &L = w->enc[layer];
    EdgeArgs ea = {};
    ea.node_info = reinterpret_cast<const int4 *>(node_info); ea.E_idx = E_idx; ea.n_nodes = n_nodes;
    // layer 0 reads the shared structure-edge state, layer 1 the per-sample edge state (in place)
    ea.hE_in = layer == 0 ? h_E0 : ws->hE; ea.in_by_src = layer == 0;
    const codlad_enc_layer_h &Lh = w->enc_h[layer];
    const bool split = w->precision != 0;
    if (which == 0) {
        ea.P = ws->PQ; ea.Q = ws->PQ + NS; ea.W1 = L.W1e; ea.W2 = L.W2; ea.S = ws->S;
        ea.W1h = Lh.W1e; ea.W2h = Lh.W2;
        set_msg_scales(ea, split, L.b2, Lh.b2, Lh.e1, Lh.e2);
    } else {
        ea.hE_out = ws->hE; ea.P = ws->PQ + 2 * NS; ea.Q = ws->PQ + 3 * NS;
        ea.S = ws->S;      // unused by the edge update; the diagnostic -DU1_STAMP build of upd1_kernel_h reports through it
        ea.W1 = L.W11e; ea.W2 = L.W12; ea.W3 = L.W13;
        ea.mods3 = mods_t + 6 * HD;
        ea.W1h = Lh.W11e; ea.W2h = Lh.W12; ea.W3h = Lh.W13;
        set_upd_scales(ea, split, L, Lh);
    }
    set_edge_walk(ea, ws);
    launch_edge(which == 1, ea, w->precision, (hipStream_t)stream, nullptr, ws->n_tiles);
    return codlad_check_launch("codlad_bench_edge_launch");
}

// ---------------------------------------------------------------------------------------------
// self-test of the chain primitive
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void selftest_kernel(const float *Wp, const float *bias,
                                                      const float *X, int n_rows, int act, float *Y) {
    const int lane = threadIdx.x, h = lane >> 5, c = lane & 31;
    const int row = blockIdx.x * 32 + c;
    const int rc = row < n_rows ? row : n_rows - 1;
    Tile in, acc;
    tile_load_row(in, X + (size_t)rc * HD, h);
    tile_load_row(acc, bias, h);
    gemm128(acc, in, Wp, lane);
    if (act) tile_gelu(acc, gelu_consts(0));
    if (row < n_rows) tile_store_row(acc, Y + (size_t)row * HD, h);
}

template <int TERMS>
__global__ __launch_bounds__(64) void selftest_h_kernel(const void *Wh, const float *bias, const float *X,
                                                        int n_rows, int act, float *Y) {
    const int lane = threadIdx.x, h = lane >> 5, c = lane & 31;
    const int row = blockIdx.x * 32 + c;
    const int rc = row < n_rows ? row : n_rows - 1;
    Tile in, acc;
    tile_load_row(in, X + (size_t)rc * HD, h);
    tile_load_row(acc, bias, h);
    if (act) gemm_h_glb<TERMS, 0, 8, true>(acc, in, Wh, lane, gelu_consts(0));    // Y = W gelu(X) + b
    else gemm_h_glb<TERMS, 0, 8, false>(acc, in, Wh, lane, gelu_consts(0));       // Y = W X + b
    if (row < n_rows) tile_store_row(acc, Y + (size_t)row * HD, h);
}

extern "C" int codlad_selftest_gemm128_h(const void *W_split, const float *bias, const float *X, int n_rows,
                                         int act_in, int terms, float *Y, void *stream) {
    CODLAD_REQUIRE(W_split && bias && X && Y && n_rows > 0 && (terms == 3 || terms == 4), "bad arguments");
    dim3 grid((n_rows + 31) / 32), block(64);
    if (terms == 3) hipLaunchKernelGGL(selftest_h_kernel<3>, grid, block, 0, (hipStream_t)stream, W_split, bias, X, n_rows, act_in, Y);
    else hipLaunchKernelGGL(selftest_h_kernel<4>, grid, block, 0, (hipStream_t)stream, W_split, bias, X, n_rows, act_in, Y);
    return codlad_check_launch("codlad_selftest_gemm128_h");
}

extern "C" int codlad_selftest_gemm128(const float *W_packed, const float *bias, const float *X,
                                       int n_rows, int act, float *Y, void *stream) {
    CODLAD_REQUIRE(W_packed && bias && X && Y && n_rows > 0, "bad arguments");
    hipLaunchKernelGGL(selftest_kernel, dim3((n_rows + 31) / 32), dim3(64), 0, (hipStream_t)stream,
                       W_packed, bias, X, n_rows, act, Y);
    return codlad_check_launch("codlad_selftest_gemm128");
}
