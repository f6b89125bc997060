// The denoiser's final layer (FinalLayer, latent_model.py:31-35) on the 32 lanes of a half wave: LayerNorm, adaLN
// modulation, Linear 128 -> n_out.  The one definition behind final_kernel (sampler_kernels.hip), loss_kernel
// (loss_kernels.hip) and ode_stage_kernel (ode_kernels.hip), which therefore give the same bits for the same hV.
// 32 lanes per node (one 16-byte word of the row each: coalesced 512-byte row reads, the reductions are butterflies
// inside the half wave), 8 nodes per 256-thread block.
#pragma once
#include "edge_args.h"     // HD, common.h, host_util.h

// What the head reads: the base of FinalArgs (sampler_args.h) and OdeStageArgs (ode_args.h).
struct HeadArgs {
    const float *hV;
    const float *mods;  // shift, scale (2 x 128)
    const float *out_w, *out_b;
    int n_nodes;
};

DEV float half_wave_allsum(float v) {
#pragma unroll
    for (int m = 16; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

// o[k] = row k of the head at node nc for k < min(N, n_out), 0 for the others.  Every lane of the half wave calls it
// and holds all of o.  Contraction is asked for here, so that units built with -ffp-contract=off round as final_kernel.
template <int N>
DEV void final_head(const HeadArgs &a, int n_out, int nc, int l, float (&o)[N]) {
#pragma clang fp contract(fast)
    const float4 v = reinterpret_cast<const float4 *>(a.hV + (size_t)nc * HD)[l];
    const float mean = half_wave_allsum((v.x + v.y) + (v.z + v.w)) * (1.0f / 128.0f);
    const float d0 = v.x - mean, d1 = v.y - mean, d2 = v.z - mean, d3 = v.w - mean;
    const float var = half_wave_allsum((d0 * d0 + d1 * d1) + (d2 * d2 + d3 * d3));
    const float rstd = 1.0f / sqrtf(var * (1.0f / 128.0f) + 1e-6f);
    const float4 sh = reinterpret_cast<const float4 *>(a.mods)[l], sc = reinterpret_cast<const float4 *>(a.mods + HD)[l];
    const float m0 = (d0 * rstd) * (1.0f + sc.x) + sh.x, m1 = (d1 * rstd) * (1.0f + sc.y) + sh.y,
                m2 = (d2 * rstd) * (1.0f + sc.z) + sh.z, m3 = (d3 * rstd) * (1.0f + sc.w) + sh.w;
#pragma unroll
    for (int k = 0; k < N; ++k) {
        o[k] = 0.f;
        if (k < n_out) {
            const float4 w = reinterpret_cast<const float4 *>(a.out_w + k * HD)[l];
            o[k] = half_wave_allsum(fmaf(m3, w.w, fmaf(m2, w.z, fmaf(m1, w.y, m0 * w.x)))) + a.out_b[k];
        }
    }
}

// inf / NaN by exponent bits.  The denoiser units are built with -fno-honor-nans: the compiler folds x != x away and
// even turns the bit test on a float's bits into |x| == inf (false for NaN), so the bits are laundered through an
// empty asm and tested as the integers they then are.
template <int N>
DEV bool any_nonfinite(const float (&o)[N]) {
    bool bad = false;
#pragma unroll
    for (int k = 0; k < N; ++k) {
        unsigned u = __float_as_uint(o[k]);
        asm volatile("" : "+v"(u));
        bad |= (u & 0x7f800000u) == 0x7f800000u;
    }
    return bad;
}

// lane k < n_out of node n's half wave picks o[k] and stores it: logits [n][n_out].  o[k] is read before the select, not
// inside it: a read that only the chosen lane performs becomes one indexed read, and the array then lives in LDS.
DEV void store_logits(float *logits, int n_out, int n, int l, const float (&o)[6]) {
    if (l < n_out) {
        float mine = o[0];
#pragma unroll
        for (int k = 1; k < 6; ++k) {
            const float ok = o[k];
            mine = l == k ? ok : mine;
        }
        logits[(size_t)n * n_out + l] = mine;
    }
}
