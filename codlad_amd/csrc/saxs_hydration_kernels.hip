// SAXS with a hydration shell and a fitted contrast (codlad_saxs_partials, codlad_saxs_hydration_fit; include/codlad_hip.h).
// An atom's amplitude is F_i = t_i + (1 - G) d_i + c2 f_w s_i: t the in-solvent form factor, d the displaced solvent, s
// the exposed fraction of the atom.  The pair walk accumulates the six partial profiles
//   P_ab[s][k] = sum_i a_i b_i + sum_{i<j} (a_i b_j + b_i a_j) sinc(q_k r_ij),  ab = tt, td, dd, ts, ds, ss
// once; any (c1, c2) is then a float64 combination of six short curves.
//
// codlad_saxs_partials, three launches (a fourth when the mean is asked for):
//   finite_kernel      one workgroup per structure: is any coordinate or weight NaN or +-inf
//   saxs_part_kernel   the decomposition of saxs_pair_kernel (saxs_kernels.hip): one workgroup of four waves per (structure,
//                      pair of row blocks p and B - 1 - p), partner j out of lane j by v_readlane so that the rows of both
//                      tables are scalar loads.  ONE sinc per (i, j, k) feeds three fp32 tile accumulators (t_j, d_j, s_j
//                      times sinc), flushed to float64 after every tile; the row atom's t_i, d_i, s_i combine them in
//                      float64.  The tt component performs the operations of saxs_pair_kernel: it carries its bits.
//   saxs_part_sum      P[s][c][k] = the workgroups' partials in ascending p; NaN for a structure that is not finite
// codlad_saxs_hydration_fit: one workgroup per curve set, a thread per grid point (strided); +, * and / in float64 only.
// -ffp-contract=off: one rounding per operation, in fp32 and in float64.
#include "common.h"
#include "reduce_math.h"
#include "saxs_math.h"
#include "structure_math.h"

namespace {
constexpr int WAVE = 64;
constexpr int WAVES = 4;
constexpr int THREADS = WAVE * WAVES;
constexpr int QC = CODLAD_SAXS_HYD_Q_CHUNK;
constexpr int NP = CODLAD_SAXS_HYD_PARTIALS;
static_assert(NP == 6 && NP * QC <= THREADS, "one thread writes one (partial, k) of a chunk");

__global__ __launch_bounds__(THREADS) void finite_kernel(const float *xyz, const float *weight, int n, uint8_t *finite) {
    const float *x = xyz + (size_t)blockIdx.x * n * 3, *wt = weight + (size_t)blockIdx.x * n;
    int bad = 0;
    for (int k = threadIdx.x; k < 3 * n; k += THREADS) bad |= non_finite(x[k]);
    for (int k = threadIdx.x; k < n; k += THREADS) bad |= non_finite(wt[k]);
    bad = __syncthreads_or(bad);
    if (threadIdx.x == 0) finite[blockIdx.x] = bad ? 0 : 1;
}

__global__ __launch_bounds__(THREADS) void saxs_part_kernel(const float *xyz, int n, int n_blocks, int n_wg, const int32_t *type,
                                                            int n_types, const float *ff_t, const float *ff_d,
                                                            const float *weight, const float *q, int n_q, const uint8_t *finite,
                                                            double *partial) {
    __shared__ double wave_part[WAVES][NP][QC];
    const int s = blockIdx.x / n_wg, p = blockIdx.x % n_wg;
    if (!finite[s]) return;                                       // its partials are never read
    const int lane = threadIdx.x & (WAVE - 1), w = threadIdx.x / WAVE;
    const float *x = xyz + (size_t)s * n * 3, *wt = weight + (size_t)s * n;
    double *out = partial + ((size_t)s * n_wg + p) * NP * n_q;
    for (int c0 = 0; c0 < n_q; c0 += QC) {
        const int kc = n_q - c0 < QC ? n_q - c0 : QC;            // uniform
        float qk[QC], iq[QC];
        double E[NP][QC];
#pragma unroll
        for (int kk = 0; kk < QC; ++kk) {
            qk[kk] = q[c0 + (kk < kc ? kk : 0)];
            iq[kk] = 1.0f / qk[kk];
#pragma unroll
            for (int c = 0; c < NP; ++c) E[c][kk] = 0.0;
        }
        for (int half = 0; half < 2; ++half) {
            const int rb = half ? n_blocks - 1 - p : p;
            if (half && rb == p) break;
            const int i = rb * WAVE + lane, ic = i < n ? i : n - 1;
            const float xi = x[3 * ic], yi = x[3 * ic + 1], zi = x[3 * ic + 2];
            double DT[QC], DD[QC], DS[QC];
#pragma unroll
            for (int kk = 0; kk < QC; ++kk) DT[kk] = 0.0, DD[kk] = 0.0, DS[kk] = 0.0;
            for (int t = rb + w; t < n_blocks; t += WAVES) {
                const int j0 = t * WAVE, cnt = n - j0 < WAVE ? n - j0 : WAVE;
                const int jc = j0 + lane < n ? j0 + lane : n - 1;
                const float xj = x[3 * jc], yj = x[3 * jc + 1], zj = x[3 * jc + 2], sj = wt[jc];
                int tj = type[jc];
                tj = tj < 0 ? 0 : tj >= n_types ? n_types - 1 : tj;
                float at[QC], ad[QC], aw[QC];
#pragma unroll
                for (int kk = 0; kk < QC; ++kk) at[kk] = 0.f, ad[kk] = 0.f, aw[kk] = 0.f;
                for (int jj = 0; jj < cnt; ++jj) {
                    const float dx = lane_read(xj, jj) - xi, dy = lane_read(yj, jj) - yi, dz = lane_read(zj, jj) - zi;
                    const size_t row = (size_t)__builtin_amdgcn_readlane(tj, jj) * n_q + c0;          // uniform
                    const float *trow = ff_t + row, *drow = ff_d + row;
                    const float sw = lane_read(sj, jj);
                    const float r = sqrtf((dx * dx + dy * dy) + dz * dz);
                    const float inv_r = 1.0f / r;
                    const bool pair = j0 + jj > i;
#pragma unroll
                    for (int kk = 0; kk < QC; ++kk) {
                        if (kk < kc) {
                            const float xx = qk[kk] * r;
                            const float sinc = sinc_term(xx, sin_cw(xx), inv_r, iq[kk]);
                            const float tt = trow[kk] * sinc, td = drow[kk] * sinc, ts = sw * sinc;
                            at[kk] += pair ? tt : 0.f;
                            ad[kk] += pair ? td : 0.f;
                            aw[kk] += pair ? ts : 0.f;
                        }
                    }
                }
#pragma unroll
                for (int kk = 0; kk < QC; ++kk) DT[kk] += (double)at[kk], DD[kk] += (double)ad[kk], DS[kk] += (double)aw[kk];
            }
            int ti = type[ic];
            ti = ti < 0 ? 0 : ti >= n_types ? n_types - 1 : ti;
            const double si = i < n ? (double)wt[ic] : 0.0;
#pragma unroll
            for (int kk = 0; kk < QC; ++kk) {
                const bool live = i < n && kk < kc;
                const size_t at_k = (size_t)ti * n_q + c0 + (kk < kc ? kk : 0);
                const double fi = live ? (double)ff_t[at_k] : 0.0, di = live ? (double)ff_d[at_k] : 0.0;
                const double sk = kk < kc ? si : 0.0;
                E[0][kk] += 2.0 * (fi * DT[kk]) + (w == 0 ? fi * fi : 0.0);      // the self terms are wave 0's
                E[1][kk] += (fi * DD[kk] + di * DT[kk]) + (w == 0 ? fi * di : 0.0);
                E[2][kk] += 2.0 * (di * DD[kk]) + (w == 0 ? di * di : 0.0);
                E[3][kk] += (fi * DS[kk] + sk * DT[kk]) + (w == 0 ? fi * sk : 0.0);
                E[4][kk] += (di * DS[kk] + sk * DD[kk]) + (w == 0 ? di * sk : 0.0);
                E[5][kk] += 2.0 * (sk * DS[kk]) + (w == 0 ? sk * sk : 0.0);
            }
        }
#pragma unroll
        for (int c = 0; c < NP; ++c) {
#pragma unroll
            for (int kk = 0; kk < QC; ++kk) {
                const double e = wave_sum(E[c][kk]);
                if (lane == 0) wave_part[w][c][kk] = e;
            }
        }
        __syncthreads();
        if ((int)threadIdx.x < NP * QC) {
            const int c = threadIdx.x / QC, kk = threadIdx.x % QC;
            if (kk < kc)
                out[(size_t)c * n_q + c0 + kk] = ((wave_part[0][c][kk] + wave_part[1][c][kk]) + wave_part[2][c][kk]) + wave_part[3][c][kk];
        }
        __syncthreads();
    }
}

// e = (s, c, k): the workgroups' partials in ascending p
__global__ __launch_bounds__(THREADS) void saxs_part_sum(const double *partial, int n_wg, int n_q, int n_struct,
                                                         const uint8_t *finite, double *P) {
    const int64_t e = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    const int64_t row = (int64_t)NP * n_q;
    if (e >= (int64_t)n_struct * row) return;
    const int s = (int)(e / row);
    const int64_t ck = e % row;
    double sum = nan64();
    if (finite[s]) {
        sum = 0.0;
        const double *part = partial + (size_t)s * n_wg * row + ck;
        for (int p = 0; p < n_wg; ++p) sum += part[(size_t)p * row];
    }
    P[e] = sum;
}

// one thread per (c, k): the finite structures' rows in ascending s
__global__ __launch_bounds__(THREADS) void saxs_part_mean(const double *P, const uint8_t *finite, int n_struct, int n_q,
                                                          double *mean) {
    const int ck = blockIdx.x * THREADS + threadIdx.x;
    const int row = NP * n_q;
    if (ck >= row) return;
    double sum = 0.0;
    int count = 0;
    for (int s = 0; s < n_struct; ++s)
        if (finite[s]) sum += P[(size_t)s * row + ck], ++count;
    mean[ck] = count ? sum / (double)count : nan64();
}

// I(q_k; c1, c2) of one curve set, the header's order; g = G[c1][k]
__device__ inline double hyd_combine(const double *P, int n_q, int k, double g, double fw, double c2) {
    const double u = 1.0 - g, w = c2 * fw;
    double I = P[k] + (2.0 * u) * P[n_q + k];
    I = I + (u * u) * P[2 * n_q + k];
    I = I + (2.0 * w) * P[3 * n_q + k];
    I = I + ((2.0 * w) * u) * P[4 * n_q + k];
    return I + (w * w) * P[5 * n_q + k];
}

__global__ __launch_bounds__(THREADS) void saxs_combine_kernel(const double *P, int n_q, const double *fw, const double *G,
                                                               int n_grid, const double *c2, int n_c2, double *I_grid) {
    const double *Pb = P + (size_t)blockIdx.x * NP * n_q;
    double *out = I_grid + (size_t)blockIdx.x * n_grid * n_q;
    for (int e = threadIdx.x; e < n_grid * n_q; e += THREADS) {
        const int g = e / n_q, k = e % n_q;
        out[e] = hyd_combine(Pb, n_q, k, G[(size_t)(g / n_c2) * n_q + k], fw[k], c2[g % n_c2]);
    }
}

// does candidate (ca, ia) beat (cb, ib)?  An index of -1 is "none yet"; a NaN or +inf chi2 is never a candidate
__device__ inline bool beats(double ca, int ia, double cb, int ib) {
    return ia >= 0 && (ib < 0 || ca < cb || (ca == cb && ia < ib));
}

__global__ __launch_bounds__(THREADS) void saxs_fit_kernel(const double *P, int n_q, const double *fw, const double *G,
                                                           int n_grid, const double *c2, int n_c2, const double *I_exp,
                                                           const double *sigma, double *scale, double *chi2, int32_t *best,
                                                           double *I_best) {
    __shared__ double best_chi[THREADS];
    __shared__ int best_idx[THREADS];
    const int b = blockIdx.x, tid = threadIdx.x;
    const double *Pb = P + (size_t)b * NP * n_q;
    double mine = __longlong_as_double(0x7ff0000000000000ll);     // +inf
    int mine_at = -1;
    for (int g = tid; g < n_grid; g += THREADS) {
        const double *Gr = G + (size_t)(g / n_c2) * n_q;
        const double cc = c2[g % n_c2];
        double num = 0.0, den = 0.0;
        for (int k = 0; k < n_q; ++k) {
            const double I = hyd_combine(Pb, n_q, k, Gr[k], fw[k], cc), wk = 1.0 / (sigma[k] * sigma[k]);
            num += (I_exp[k] * I) * wk;
            den += (I * I) * wk;
        }
        const double sc = num / den;
        double sum = 0.0;
        for (int k = 0; k < n_q; ++k) {
            const double r = (sc * hyd_combine(Pb, n_q, k, Gr[k], fw[k], cc) - I_exp[k]) / sigma[k];
            sum += r * r;
        }
        const double x2 = sum / (double)(n_q - 1);
        scale[(size_t)b * n_grid + g] = sc;
        chi2[(size_t)b * n_grid + g] = x2;
        if (x2 < mine) mine = x2, mine_at = g;                    // ascending g: the lowest index of a tie stays
    }
    best_chi[tid] = mine;
    best_idx[tid] = mine_at;
    __syncthreads();
    for (int st = THREADS / 2; st > 0; st >>= 1) {
        if (tid < st && beats(best_chi[tid + st], best_idx[tid + st], best_chi[tid], best_idx[tid])) {
            best_chi[tid] = best_chi[tid + st];
            best_idx[tid] = best_idx[tid + st];
        }
        __syncthreads();
    }
    const int at = best_idx[0];
    if (tid == 0) best[b] = at;
    for (int k = tid; k < n_q; k += THREADS)
        I_best[(size_t)b * n_q + k] = at < 0 ? nan64() : hyd_combine(Pb, n_q, k, G[(size_t)(at / n_c2) * n_q + k], fw[k], c2[at % n_c2]);
}
}  // namespace

extern "C" int codlad_saxs_partials(const float *xyz, int n_struct, int n_atoms, const int32_t *type, int n_types, const float *ff_t,
                                    const float *ff_d, const float *weight, const float *q, int n_q, double *partial, double *P,
                                    double *mean_P, uint8_t *finite, void *stream) {
    CODLAD_REQUIRE(xyz && type && ff_t && ff_d && weight && q && partial && P && finite, "null pointer");
    CODLAD_REQUIRE(n_struct > 0 && n_atoms > 0, "bad counts");
    CODLAD_REQUIRE(n_q >= 1 && n_q <= CODLAD_SAXS_MAX_Q, "n_q outside 1 .. 512");
    CODLAD_REQUIRE(n_types >= 1 && n_types <= CODLAD_SAXS_MAX_TYPES, "n_types outside 1 .. 32");
    const int64_t blocks = ((int64_t)n_atoms + WAVE - 1) / WAVE, n_wg = (blocks + 1) / 2;
    CODLAD_REQUIRE(n_wg * n_struct < (int64_t)1 << 31 && (int64_t)n_atoms * 3 < (int64_t)1 << 31,
                   "too many workgroups for one launch");
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(finite_kernel, dim3((unsigned)n_struct), dim3(THREADS), 0, st, xyz, weight, n_atoms, finite);
    int rc = codlad_check_launch("codlad_saxs_partials");
    if (rc) return rc;
    hipLaunchKernelGGL(saxs_part_kernel, dim3((unsigned)(n_wg * n_struct)), dim3(THREADS), 0, st, xyz, n_atoms, (int)blocks,
                       (int)n_wg, type, n_types, ff_t, ff_d, weight, q, n_q, finite, partial);
    rc = codlad_check_launch("codlad_saxs_partials");
    if (rc) return rc;
    const int64_t row = (int64_t)NP * n_q;
    const unsigned sum_blocks = (unsigned)((n_struct * row + THREADS - 1) / THREADS);
    hipLaunchKernelGGL(saxs_part_sum, dim3(sum_blocks), dim3(THREADS), 0, st, partial, (int)n_wg, n_q, n_struct, finite, P);
    rc = codlad_check_launch("codlad_saxs_partials");
    if (rc || !mean_P) return rc;
    hipLaunchKernelGGL(saxs_part_mean, dim3((unsigned)((row + THREADS - 1) / THREADS)), dim3(THREADS), 0, st, P, finite, n_struct,
                       n_q, mean_P);
    return codlad_check_launch("codlad_saxs_partials");
}

extern "C" int codlad_saxs_hydration_fit(const double *P, int n_batch, int n_q, const double *f_w, const double *G, int n_c1,
                                         const double *c2, int n_c2, const double *I_exp, const double *sigma, double *I_grid,
                                         double *scale, double *chi2, int32_t *best, double *I_best, void *stream) {
    CODLAD_REQUIRE(P && f_w && G && c2, "null pointer");
    CODLAD_REQUIRE(n_batch > 0 && n_c1 > 0 && n_c2 > 0, "bad counts");
    CODLAD_REQUIRE(n_q >= 1 && n_q <= CODLAD_SAXS_MAX_Q, "n_q outside 1 .. 512");
    CODLAD_REQUIRE((int64_t)n_c1 * n_c2 <= CODLAD_SAXS_HYD_MAX_GRID, "more than CODLAD_SAXS_HYD_MAX_GRID grid points");
    CODLAD_REQUIRE(!I_exp == !sigma, "I_exp and sigma come together");
    const int n_grid = n_c1 * n_c2;
    hipStream_t st = (hipStream_t)stream;
    if (!I_exp) {
        CODLAD_REQUIRE(I_grid, "null pointer");
        hipLaunchKernelGGL(saxs_combine_kernel, dim3((unsigned)n_batch), dim3(THREADS), 0, st, P, n_q, f_w, G, n_grid, c2, n_c2, I_grid);
        return codlad_check_launch("codlad_saxs_hydration_fit");
    }
    CODLAD_REQUIRE(scale && chi2 && best && I_best, "null pointer");
    CODLAD_REQUIRE(n_q >= 2, "a fit needs two q values or more");
    hipLaunchKernelGGL(saxs_fit_kernel, dim3((unsigned)n_batch), dim3(THREADS), 0, st, P, n_q, f_w, G, n_grid, c2, n_c2, I_exp, sigma,
                       scale, chi2, best, I_best);
    return codlad_check_launch("codlad_saxs_hydration_fit");
}
