// What the two SAXS pair kernels share (saxs_kernels.hip, saxs_hydration_kernels.hip): the partner read, the header's
// sine and the selection of sinc - the sequence of fp32 operations include/codlad_hip.h states for codlad_saxs_debye.
// Both files are compiled with -ffp-contract=off: one rounding per operation.
#pragma once
#include "../../include/codlad_hip.h"
#include "common.h"

namespace {
__device__ inline float lane_read(float v, int lane) {
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane));
}

// sin(x) for x >= 0, the header's sequence
__device__ inline float sin_cw(float x) {
    const float kf = __builtin_rintf(x * CODLAD_SAXS_INV_PI);
    const float y = ((x - kf * CODLAD_SAXS_P1) - kf * CODLAD_SAXS_P2) - kf * CODLAD_SAXS_P3;
    const float s = y * y;
    float p = CODLAD_SAXS_S11 * s + CODLAD_SAXS_S9;
    p = p * s + CODLAD_SAXS_S7;
    p = p * s + CODLAD_SAXS_S5;
    p = p * s + CODLAD_SAXS_S3;
    const float v = y + (y * s) * p;
    return __uint_as_float(__float_as_uint(v) ^ ((uint32_t)(int)kf << 31));
}

__device__ inline float sinc_term(float x, float sn, float inv_r, float inv_q) {
    const float far = (sn * inv_r) * inv_q;
    const float x2 = x * x;
    const float series = 1.0f - (x2 * CODLAD_SAXS_C6) * (1.0f - x2 * CODLAD_SAXS_C20);
    return x < CODLAD_SAXS_X_SMALL ? series : far;
}
}  // namespace
