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
// Here: the fp32 reference kernels (precision 0), the hoisted layer-0 edge terms and the self-test kernels of the chain
// primitive; the split-fp16 kernels of precision 1, 2 have units of their own (host_util.h lists them).
#include "node_args.h"

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
        const XIn xi = x_in_load(a, nc);
        tile_load_row(v, a.x_in_b, h);
#pragma unroll
        for (int bo = 0; bo < 4; ++bo) x_in_block(v.b[bo], xi, a, bo, h);
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

void launch_edge_f32(bool update, const EdgeArgs &ea, hipStream_t st) {
    dispatch_note((ea.n_nodes + 3) / 4);
    hipLaunchKernelGGL(update ? edge_kernel<true> : edge_kernel<false>, dim3((ea.n_nodes + 3) / 4), dim3(256), 0, st, ea);
}
void launch_node_f32(bool upd, const NodeArgs &na, hipStream_t st) {
    dispatch_note((na.n_nodes + 31) / 32);
    hipLaunchKernelGGL(upd ? node_kernel<true> : node_kernel<false>, dim3((na.n_nodes + 31) / 32), dim3(64), 0, st, na);
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
    hipLaunchKernelGGL(w->precision == 2 ? layer0_kernel<3> : (w->precision == 1 ? layer0_kernel<4> : layer0_kernel<0>), grid, block, 0,
                       (hipStream_t)stream, a);
    return codlad_check_launch("codlad_layer0_edge_terms");
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
    hipLaunchKernelGGL(terms == 3 ? selftest_h_kernel<3> : selftest_h_kernel<4>, grid, block, 0, (hipStream_t)stream, W_split, bias, X,
                       n_rows, act_in, Y);
    return codlad_check_launch("codlad_selftest_gemm128_h");
}

extern "C" int codlad_selftest_gemm128(const float *W_packed, const float *bias, const float *X,
                                       int n_rows, int act, float *Y, void *stream) {
    CODLAD_REQUIRE(W_packed && bias && X && Y && n_rows > 0, "bad arguments");
    hipLaunchKernelGGL(selftest_kernel, dim3((n_rows + 31) / 32), dim3(64), 0, (hipStream_t)stream,
                       W_packed, bias, X, n_rows, act, Y);
    return codlad_check_launch("codlad_selftest_gemm128");
}
