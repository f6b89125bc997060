// Small-angle X-ray scattering of generated structures (codlad_saxs_debye; include/codlad_hip.h): the Debye sum
//   I[s][k] = sum_i f_i(k)^2 + 2 sum_{i<j} f_i(k) f_j(k) sinc(q_k r_ij)
// over all pairs of every structure of a call - no neighbour list, no cut-off, no atomics, each structure on its own.
//
// Three launches on the caller's stream (a fourth, one thread per k, when the ensemble mean is asked for):
//   finite_kernel     structure_math.h's: one workgroup per structure, is any coordinate NaN or +-inf
//   saxs_pair_kernel  one workgroup of four waves per (structure, pair of row blocks p and B - 1 - p: the triangle is
//                     evenly loaded).  Lane l owns atom i of the row block; a wave walks its partner tiles, 64 atoms a tile,
//                     one partner per lane in registers: the j loop is wave-uniform, partner j's coordinates and type come
//                     out of lane j by v_readlane into scalar registers, so ff[type_j][k] is a scalar load.  Q is walked in
//                     chunks of Q_CHUNK fp32 accumulators per lane; they are flushed to float64 after every tile.
//   saxs_sum_kernel   I[s][k] = the workgroups' partials in ascending order; NaN for a structure that is not finite.
// The sine is the header's sequence of fp32 operations (Cody-Waite reduction by pi, an odd polynomial, the sign from the
// parity), not the hardware instruction and not a library call: the float32 restatement of the tests performs the same
// operations.  -ffp-contract=off: one rounding per operation, in fp32 and in float64.
#include "common.h"
#include "reduce_math.h"
#include "saxs_math.h"
#include "structure_math.h"

namespace {
constexpr int WAVE = 64;
constexpr int WAVES = 4;
constexpr int THREADS = WAVE * WAVES;
constexpr int QC = CODLAD_SAXS_Q_CHUNK;

__global__ __launch_bounds__(THREADS) void saxs_pair_kernel(const float *xyz, int n, int n_blocks, int n_wg, const int32_t *type,
                                                            int n_types, const float *ff, const float *q, int n_q,
                                                            const uint8_t *finite, double *partial) {
    __shared__ double wave_part[WAVES][QC];
    const int s = blockIdx.x / n_wg, p = blockIdx.x % n_wg;
    if (!finite[s]) return;                                       // its partials are never read
    const int lane = threadIdx.x & (WAVE - 1), w = threadIdx.x / WAVE;
    const float *x = xyz + (size_t)s * n * 3;
    double *out = partial + ((size_t)s * n_wg + p) * n_q;
    for (int c0 = 0; c0 < n_q; c0 += QC) {
        const int kc = n_q - c0 < QC ? n_q - c0 : QC;            // uniform
        float qk[QC], iq[QC];
        double E[QC];
#pragma unroll
        for (int kk = 0; kk < QC; ++kk) {
            qk[kk] = q[c0 + (kk < kc ? kk : 0)];
            iq[kk] = 1.0f / qk[kk];
            E[kk] = 0.0;
        }
        for (int half = 0; half < 2; ++half) {
            const int rb = half ? n_blocks - 1 - p : p;
            if (half && rb == p) break;
            const int i = rb * WAVE + lane, ic = i < n ? i : n - 1;
            const float xi = x[3 * ic], yi = x[3 * ic + 1], zi = x[3 * ic + 2];
            double D[QC];
#pragma unroll
            for (int kk = 0; kk < QC; ++kk) D[kk] = 0.0;
            for (int t = rb + w; t < n_blocks; t += WAVES) {
                const int j0 = t * WAVE, cnt = n - j0 < WAVE ? n - j0 : WAVE;
                const int jc = j0 + lane < n ? j0 + lane : n - 1;
                const float xj = x[3 * jc], yj = x[3 * jc + 1], zj = x[3 * jc + 2];
                int tj = type[jc];
                tj = tj < 0 ? 0 : tj >= n_types ? n_types - 1 : tj;
                float acc[QC];
#pragma unroll
                for (int kk = 0; kk < QC; ++kk) acc[kk] = 0.f;
                for (int jj = 0; jj < cnt; ++jj) {
                    const float dx = lane_read(xj, jj) - xi, dy = lane_read(yj, jj) - yi, dz = lane_read(zj, jj) - zi;
                    const float *frow = ff + (size_t)__builtin_amdgcn_readlane(tj, jj) * n_q + c0;    // uniform
                    const float r = sqrtf((dx * dx + dy * dy) + dz * dz);
                    const float inv_r = 1.0f / r;
                    const bool pair = j0 + jj > i;
#pragma unroll
                    for (int kk = 0; kk < QC; ++kk) {
                        if (kk < kc) {
                            const float xx = qk[kk] * r;
                            const float term = frow[kk] * sinc_term(xx, sin_cw(xx), inv_r, iq[kk]);
                            acc[kk] += pair ? term : 0.f;
                        }
                    }
                }
#pragma unroll
                for (int kk = 0; kk < QC; ++kk) D[kk] += (double)acc[kk];
            }
            int ti = type[ic];
            ti = ti < 0 ? 0 : ti >= n_types ? n_types - 1 : ti;
#pragma unroll
            for (int kk = 0; kk < QC; ++kk) {
                const double fi = i < n && kk < kc ? (double)ff[(size_t)ti * n_q + c0 + (kk < kc ? kk : 0)] : 0.0;
                const double self = w == 0 ? fi * fi : 0.0;
                E[kk] += 2.0 * (fi * D[kk]) + self;
            }
        }
#pragma unroll
        for (int kk = 0; kk < QC; ++kk) {
            const double e = wave_sum(E[kk]);
            if (lane == 0) wave_part[w][kk] = e;
        }
        __syncthreads();
        if ((int)threadIdx.x < kc) {
            const int kk = threadIdx.x;
            out[c0 + kk] = ((wave_part[0][kk] + wave_part[1][kk]) + wave_part[2][kk]) + wave_part[3][kk];
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(THREADS) void saxs_sum_kernel(const double *partial, int n_wg, int n_q, int n_struct,
                                                           const uint8_t *finite, double *I) {
    const int64_t e = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    if (e >= (int64_t)n_struct * n_q) return;
    const int s = (int)(e / n_q), k = (int)(e % n_q);
    double sum = nan64();
    if (finite[s]) {
        sum = 0.0;
        const double *part = partial + (size_t)s * n_wg * n_q + k;
        for (int p = 0; p < n_wg; ++p) sum += part[(size_t)p * n_q];
    }
    I[e] = sum;
}

// one thread per k: the finite structures' rows in ascending s
__global__ __launch_bounds__(THREADS) void saxs_mean_kernel(const double *I, const uint8_t *finite, int n_struct, int n_q,
                                                            double *mean) {
    const int k = blockIdx.x * THREADS + threadIdx.x;
    if (k >= n_q) return;
    double sum = 0.0;
    int count = 0;
    for (int s = 0; s < n_struct; ++s)
        if (finite[s]) sum += I[(size_t)s * n_q + k], ++count;
    mean[k] = count ? sum / (double)count : nan64();
}
}  // namespace

extern "C" int codlad_saxs_debye(const float *xyz, int n_struct, int n_atoms, const int32_t *type, int n_types, const float *ff,
                                 const float *q, int n_q, double *partial, double *I, double *mean, uint8_t *finite,
                                 void *stream) {
    CODLAD_REQUIRE(xyz && type && ff && q && partial && I && finite, "null pointer");
    CODLAD_REQUIRE(n_struct > 0 && n_atoms > 0, "bad counts");
    CODLAD_REQUIRE(n_q >= 1 && n_q <= CODLAD_SAXS_MAX_Q, "n_q outside 1 .. 512");
    CODLAD_REQUIRE(n_types >= 1 && n_types <= CODLAD_SAXS_MAX_TYPES, "n_types outside 1 .. 32");
    const int64_t blocks = ((int64_t)n_atoms + WAVE - 1) / WAVE, n_wg = (blocks + 1) / 2;
    CODLAD_REQUIRE(n_wg * n_struct < (int64_t)1 << 31 && (int64_t)n_atoms * 3 < (int64_t)1 << 31,
                   "too many workgroups for one launch");
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(finite_kernel<THREADS>, dim3((unsigned)n_struct), dim3(THREADS), 0, st, xyz, n_atoms * 3, finite);
    int rc = codlad_check_launch("codlad_saxs_debye");
    if (rc) return rc;
    hipLaunchKernelGGL(saxs_pair_kernel, dim3((unsigned)(n_wg * n_struct)), dim3(THREADS), 0, st, xyz, n_atoms, (int)blocks,
                       (int)n_wg, type, n_types, ff, q, n_q, finite, partial);
    rc = codlad_check_launch("codlad_saxs_debye");
    if (rc) return rc;
    const unsigned sum_blocks = (unsigned)(((int64_t)n_struct * n_q + THREADS - 1) / THREADS);
    hipLaunchKernelGGL(saxs_sum_kernel, dim3(sum_blocks), dim3(THREADS), 0, st, partial, (int)n_wg, n_q, n_struct, finite, I);
    rc = codlad_check_launch("codlad_saxs_debye");
    if (rc || !mean) return rc;
    hipLaunchKernelGGL(saxs_mean_kernel, dim3((unsigned)((n_q + THREADS - 1) / THREADS)), dim3(THREADS), 0, st, I, finite, n_struct,
                       n_q, mean);
    return codlad_check_launch("codlad_saxs_debye");
}
