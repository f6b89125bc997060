// The fixed-order per-sample reduction of the loss kernels (loss_kernels.hip, flow_loss_kernels.hip): one 256-thread
// workgroup per sample, half wave w of the eight takes the sample's nodes w, w + 8, ... in order and lane k < 3 of it adds
// component k's value to its running sum; then (lane 0 + lane 1) + lane 2 per half wave, then half waves 0 .. 7 in order.
// The order depends on the sample's length alone: not on the grid, not on what else shares the job, and no floating-point
// atomic is involved.  Both units are built with -ffp-contract=off.
#pragma once
#include "common.h"

// Sum over the sample of per-lane running sums (lanes 0-2 of every half wave), in the fixed order of the header.
// part: LDS [NQ][8].  Every thread of the workgroup calls it; the totals are valid in thread 0.
template <int NQ>
DEV void sample_sum(float (&acc)[NQ], float (*part)[8]) {
    const int l = threadIdx.x & 31, hw = threadIdx.x >> 5;
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
        const int base = threadIdx.x & 32;
        const float s = (__shfl(acc[q], base, 64) + __shfl(acc[q], base + 1, 64)) + __shfl(acc[q], base + 2, 64);
        if (l == 0) part[q][hw] = s;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            float s = part[q][0];
            for (int w = 1; w < 8; ++w) s = s + part[q][w];
            acc[q] = s;
        }
    }
}
