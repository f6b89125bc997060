// Typed pair-distance histograms of generated structures (codlad_pair_hist, codlad_pair_hist_profile;
// include/codlad_hip.h): per structure and per class of atom types (a <= b) the integer number of atom pairs per distance
// bin - one sqrt and one integer LDS add per pair, no q - and what follows from the counts in float64: P(r), its I(0) and
// second moment, and I(q) on any q grid from a host-tabulated sinc.
//
// codlad_pair_hist, three launches on the caller's stream:
//   finite_kernel     structure_math.h's: one workgroup per structure, is any coordinate NaN or +-inf
//   fill_kernel       H, over = 0 (-1 for a structure that is not finite), d_bin = -1: the call writes every element
//   pair_hist_kernel  one workgroup of four waves per (structure, item).  The atoms are walked in the caller's order by
//                     type, so an item has ONE class: the histogram in LDS is n_bins ints.  Lane l owns row position
//                     row0 + l; wave w takes the column tiles w, w + 4, .. of the item's column range, 64 positions a tile,
//                     one partner per lane in registers, the j loop wave-uniform with the partner out of lane j by
//                     v_readlane (saxs_pair_kernel's walk).  Per pair the header's fp32 sequence and an LDS atomic add on
//                     int; pairs beyond the last bin are counted per lane in a register.  The non-zero bins go to H by
//                     integer atomic adds, the highest of them to d_bin by an integer atomic max.
// Integer adds commute: no result depends on the order in which workgroups or lanes arrive.  No floating-point atomics.
// codlad_pair_hist_profile: plain float64 loops, every sum in the header's one order.  -ffp-contract=off: one rounding per
// operation, in fp32 and in float64.
#include "common.h"
#include "reduce_math.h"
#include "saxs_math.h"
#include "structure_math.h"

namespace {
constexpr int WAVE = CODLAD_PAIR_HIST_ROWS;
constexpr int WAVES = 4;
constexpr int THREADS = WAVE * WAVES;
constexpr int ITEM = CODLAD_PAIR_HIST_ITEM_WORDS;
constexpr int FILL_BLOCKS = 2048;

__global__ __launch_bounds__(THREADS) void fill_kernel(const uint8_t *finite, int n_struct, int64_t per_h, int n_class,
                                                       int32_t *H, int32_t *over, int32_t *d_bin) {
    const int64_t stride = (int64_t)gridDim.x * THREADS, first = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    for (int64_t e = first; e < per_h * n_struct; e += stride) H[e] = finite[e / per_h] ? 0 : -1;
    for (int64_t e = first; e < (int64_t)n_class * n_struct; e += stride) over[e] = finite[e / n_class] ? 0 : -1;
    for (int64_t e = first; e < n_struct; e += stride) d_bin[e] = -1;
}

__global__ __launch_bounds__(THREADS) void pair_hist_kernel(const float *xyz, int n, const int32_t *order,
                                                            const int32_t *type_start, int n_types, float inv_dr, int n_bins,
                                                            const int32_t *items, int n_items, const uint8_t *finite,
                                                            int32_t *H, int32_t *over, int32_t *d_bin) {
    __shared__ int hist[CODLAD_PAIR_HIST_MAX_BINS];
    const int s = blockIdx.x / n_items;
    if (!finite[s]) return;                                       // its rows are fill_kernel's -1
    const int32_t *item = items + (size_t)(blockIdx.x % n_items) * ITEM;
    // every word of the tables into its range: a wrong table counts wrongly, inside the buffers
    const int a = clampi(item[0], 0, n_types - 1), b = clampi(item[1], a, n_types - 1);
    const int a0 = clampi(type_start[a], 0, n), a1 = clampi(type_start[a + 1], a0, n);
    const int b0 = clampi(type_start[b], 0, n), b1 = clampi(type_start[b + 1], b0, n);
    const int row0 = clampi(item[2], a0, a1);
    const int c0 = clampi(item[3], b0, b1), c1 = clampi(item[4], c0, b1);
    if (row0 >= a1 || c0 >= c1) return;                           // uniform: no pair
    const int n_class = n_types * (n_types + 1) / 2, c = CODLAD_PAIR_HIST_CLASS(a, b, n_types);
    for (int k = threadIdx.x; k < n_bins; k += THREADS) hist[k] = 0;
    __syncthreads();

    const int lane = threadIdx.x & (WAVE - 1), w = threadIdx.x / WAVE;
    const float *x = xyz + (size_t)s * n * 3;
    const int ip = row0 + lane;
    const bool row = ip < a1;
    const int ia = clampi(order[row ? ip : a1 - 1], 0, n - 1);
    const float xi = x[3 * ia], yi = x[3 * ia + 1], zi = x[3 * ia + 2];
    const float bins_f = (float)n_bins;
    const bool tri = a == b;
    int ov = 0;
    for (int j0 = c0 + w * WAVE; j0 < c1; j0 += WAVE * WAVES) {
        const int cnt = c1 - j0 < WAVE ? c1 - j0 : WAVE;
        const int ja = clampi(order[j0 + lane < c1 ? j0 + lane : c1 - 1], 0, n - 1);
        const float xj = x[3 * ja], yj = x[3 * ja + 1], zj = x[3 * ja + 2];
        for (int jj = 0; jj < cnt; ++jj) {
            const float dx = lane_read(xj, jj) - xi, dy = lane_read(yj, jj) - yi, dz = lane_read(zj, jj) - zi;
            const float r = sqrtf((dx * dx + dy * dy) + dz * dz);
            const float t = r * inv_dr;
            if (row && (!tri || j0 + jj > ip)) {
                if (t < bins_f) atomicAdd(&hist[(int)t], 1);
                else ++ov;
            }
        }
    }
    ov = wave_sum(ov);
    if (lane == 0 && ov) atomicAdd(&over[(size_t)s * n_class + c], ov);
    __syncthreads();
    int32_t *out = H + ((size_t)s * n_class + c) * n_bins;
    int top = -1;
    for (int k = threadIdx.x; k < n_bins; k += THREADS) {
        const int v = hist[k];
        if (v) atomicAdd(&out[k], v), top = k;
    }
#pragma unroll
    for (int st = WAVE / 2; st > 0; st >>= 1) {
        const int o = __shfl_xor(top, st);
        top = o > top ? o : top;
    }
    if (lane == 0 && top >= 0) atomicMax(&d_bin[s], top);
}

// ------------------------------------------------------------------------------------------------ from the counts --
// class c -> (a, b): rows a ascending, b ascending within a
__device__ inline void class_types(int c, int n_types, int &a, int &b) {
    a = 0;
    while (c >= n_types - a) c -= n_types - a, ++a;
    b = a + c;
}

// one thread per structure
__global__ __launch_bounds__(THREADS) void complete_kernel(const int32_t *over, const uint8_t *finite, int n_struct,
                                                           int n_class, uint8_t *complete) {
    const int s = blockIdx.x * THREADS + threadIdx.x;
    if (s >= n_struct) return;
    int ok = finite[s] ? 1 : 0;
    for (int c = 0; c < n_class; ++c) ok &= over[(size_t)s * n_class + c] == 0;
    complete[s] = (uint8_t)ok;
}

// one workgroup per (structure, class), a thread per k: the bins ascending up to the structure's d_bin
__global__ __launch_bounds__(WAVE) void profile_class_kernel(const int32_t *H, const int32_t *d_bin, const uint8_t *complete,
                                                             int n_class, int n_bins, const double *sinc_table, int n_q,
                                                             double *partial) {
    const int s = blockIdx.x / n_class;
    if (!complete[s]) return;                                     // its partials are never read
    const int32_t *h = H + (size_t)blockIdx.x * n_bins;
    const int last = clampi(d_bin[s], -1, n_bins - 1);
    for (int k = threadIdx.x; k < n_q; k += WAVE) {
        double sum = 0.0;
        for (int bin = 0; bin <= last; ++bin) sum += (double)h[bin] * sinc_table[(size_t)bin * n_q + k];
        partial[(size_t)blockIdx.x * n_q + k] = sum;
    }
}

// one thread per (structure, k): the classes ascending
__global__ __launch_bounds__(THREADS) void profile_sum_kernel(const double *partial, const uint8_t *complete, int n_struct,
                                                              int n_types, const int32_t *count, const double *ff, int n_q,
                                                              double *I) {
    const int64_t e = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    if (e >= (int64_t)n_struct * n_q) return;
    const int s = (int)(e / n_q), k = (int)(e % n_q);
    double out = nan64();
    if (complete[s]) {
        const int n_class = n_types * (n_types + 1) / 2;
        double self = 0.0, cross = 0.0;
        for (int a = 0; a < n_types; ++a) {
            const double f = ff[(size_t)a * n_q + k];
            self += (double)count[a] * (f * f);
        }
        const double *part = partial + (size_t)s * n_class * n_q + k;
        int c = 0;
        for (int a = 0; a < n_types; ++a)
            for (int b = a; b < n_types; ++b, ++c)
                cross += (ff[(size_t)a * n_q + k] * ff[(size_t)b * n_q + k]) * part[(size_t)c * n_q];
        out = self + 2.0 * cross;
    }
    I[e] = out;
}

// one thread per (structure, bin): the classes ascending
__global__ __launch_bounds__(THREADS) void pr_kernel(const int32_t *H, const int32_t *d_bin, const uint8_t *finite, int n_struct,
                                                     int n_types, int n_bins, const double *w, double *P) {
    const int64_t e = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    if (e >= (int64_t)n_struct * n_bins) return;
    const int s = (int)(e / n_bins), bin = (int)(e % n_bins);
    double out = nan64();
    if (finite[s]) {
        out = 0.0;
        if (bin <= d_bin[s]) {
            const int n_class = n_types * (n_types + 1) / 2;
            const int32_t *h = H + (size_t)s * n_class * n_bins + bin;
            int c = 0;
            for (int a = 0; a < n_types; ++a)
                for (int b = a; b < n_types; ++b, ++c) out += (w[a] * w[b]) * (double)h[(size_t)c * n_bins];
        }
    }
    P[e] = out;
}

// one thread per structure: the bins ascending up to d_bin
__global__ __launch_bounds__(THREADS) void pr_moments_kernel(const double *P, const int32_t *d_bin, const uint8_t *finite,
                                                             int n_struct, int n_types, int n_bins, const int32_t *count,
                                                             const double *w, const double *r2, double *I0, double *m2) {
    const int s = blockIdx.x * THREADS + threadIdx.x;
    if (s >= n_struct) return;
    double i0 = nan64(), mom = nan64();
    if (finite[s]) {
        const int last = clampi(d_bin[s], -1, n_bins - 1);
        const double *p = P + (size_t)s * n_bins;
        double self = 0.0, sum = 0.0;
        mom = 0.0;
        for (int a = 0; a < n_types; ++a) self += (double)count[a] * (w[a] * w[a]);
        for (int bin = 0; bin <= last; ++bin) sum += p[bin], mom += r2[bin] * p[bin];
        i0 = self + 2.0 * sum;
    }
    I0[s] = i0;
    m2[s] = mom;
}

// one thread per column: the complete structures' rows in ascending s
__global__ __launch_bounds__(THREADS) void hist_mean_kernel(const double *rows, const uint8_t *complete, int n_struct,
                                                            int n_cols, double *mean) {
    const int k = blockIdx.x * THREADS + threadIdx.x;
    if (k >= n_cols) return;
    double sum = 0.0;
    int count = 0;
    for (int s = 0; s < n_struct; ++s)
        if (complete[s]) sum += rows[(size_t)s * n_cols + k], ++count;
    mean[k] = count ? sum / (double)count : nan64();
}

unsigned blocks_of(int64_t threads) { return (unsigned)((threads + THREADS - 1) / THREADS); }
}  // namespace

extern "C" int codlad_pair_hist(const float *xyz, int n_struct, int n_atoms, const int32_t *order, const int32_t *type_start,
                                int n_types, float inv_dr, int n_bins, const int32_t *items, int n_items, int32_t *H,
                                int32_t *over, int32_t *d_bin, uint8_t *finite, void *stream) {
    CODLAD_REQUIRE(xyz && order && type_start && items && H && over && d_bin && finite, "null pointer");
    CODLAD_REQUIRE(n_struct > 0 && n_atoms > 0 && n_items > 0, "bad counts");
    CODLAD_REQUIRE(n_bins >= 1 && n_bins <= CODLAD_PAIR_HIST_MAX_BINS, "n_bins outside 1 .. 4096");
    CODLAD_REQUIRE(n_atoms <= CODLAD_PAIR_HIST_MAX_ATOMS, "n_atoms above 65535");
    CODLAD_REQUIRE(n_types >= 1 && n_types <= CODLAD_SAXS_MAX_TYPES, "n_types outside 1 .. 32");
    CODLAD_REQUIRE(inv_dr > 0.f && inv_dr <= 3.402823466e38f, "inv_dr is not a positive finite number");
    CODLAD_REQUIRE((int64_t)n_struct * n_items < (int64_t)1 << 31, "too many workgroups for one launch");
    const int n_class = n_types * (n_types + 1) / 2;
    const int64_t per_h = (int64_t)n_class * n_bins;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(finite_kernel<THREADS>, dim3((unsigned)n_struct), dim3(THREADS), 0, st, xyz, n_atoms * 3, finite);
    int rc = codlad_check_launch("codlad_pair_hist");
    if (rc) return rc;
    const int64_t fill = (per_h * n_struct + THREADS - 1) / THREADS;
    hipLaunchKernelGGL(fill_kernel, dim3((unsigned)(fill < FILL_BLOCKS ? fill : FILL_BLOCKS)), dim3(THREADS), 0, st, finite,
                       n_struct, per_h, n_class, H, over, d_bin);
    rc = codlad_check_launch("codlad_pair_hist");
    if (rc) return rc;
    hipLaunchKernelGGL(pair_hist_kernel, dim3((unsigned)((int64_t)n_struct * n_items)), dim3(THREADS), 0, st, xyz, n_atoms,
                       order, type_start, n_types, inv_dr, n_bins, items, n_items, finite, H, over, d_bin);
    return codlad_check_launch("codlad_pair_hist");
}

extern "C" int codlad_pair_hist_profile(const int32_t *H, const int32_t *over, const int32_t *d_bin, const uint8_t *finite,
                                        int n_struct, int n_types, int n_bins, const int32_t *count, const double *ff,
                                        const double *sinc_table, int n_q, double *partial, double *I, double *mean_I,
                                        const double *w, const double *r2, double *P, double *I0, double *m2, double *mean_P,
                                        uint8_t *complete, void *stream) {
    CODLAD_REQUIRE(H && over && d_bin && finite && count && complete, "null pointer");
    CODLAD_REQUIRE(I || P, "neither I nor P is asked for");
    CODLAD_REQUIRE(!I || (ff && sinc_table && partial), "null pointer (profile)");
    CODLAD_REQUIRE(!P || (w && r2 && I0 && m2), "null pointer (pair distribution)");
    CODLAD_REQUIRE((I || !mean_I) && (P || !mean_P), "a mean without its rows");
    CODLAD_REQUIRE(n_struct > 0 && n_bins > 0 && (!I || n_q > 0), "bad counts");
    CODLAD_REQUIRE(n_bins <= CODLAD_PAIR_HIST_MAX_BINS, "n_bins above 4096");
    CODLAD_REQUIRE(n_types >= 1 && n_types <= CODLAD_SAXS_MAX_TYPES, "n_types outside 1 .. 32");
    CODLAD_REQUIRE(!I || n_q <= CODLAD_SAXS_MAX_Q, "n_q above 512");
    const int n_class = n_types * (n_types + 1) / 2;
    CODLAD_REQUIRE((int64_t)n_struct * n_class < (int64_t)1 << 31, "too many workgroups for one launch");
    hipStream_t st = (hipStream_t)stream;
    const char *what = "codlad_pair_hist_profile";
    hipLaunchKernelGGL(complete_kernel, dim3(blocks_of(n_struct)), dim3(THREADS), 0, st, over, finite, n_struct, n_class, complete);
    int rc = codlad_check_launch(what);
    if (rc) return rc;
    if (I) {
        hipLaunchKernelGGL(profile_class_kernel, dim3((unsigned)(n_struct * n_class)), dim3(WAVE), 0, st, H, d_bin, complete,
                           n_class, n_bins, sinc_table, n_q, partial);
        if ((rc = codlad_check_launch(what))) return rc;
        hipLaunchKernelGGL(profile_sum_kernel, dim3(blocks_of((int64_t)n_struct * n_q)), dim3(THREADS), 0, st, partial, complete,
                           n_struct, n_types, count, ff, n_q, I);
        if ((rc = codlad_check_launch(what))) return rc;
        if (mean_I) {
            hipLaunchKernelGGL(hist_mean_kernel, dim3(blocks_of(n_q)), dim3(THREADS), 0, st, I, complete, n_struct, n_q, mean_I);
            if ((rc = codlad_check_launch(what))) return rc;
        }
    }
    if (P) {
        hipLaunchKernelGGL(pr_kernel, dim3(blocks_of((int64_t)n_struct * n_bins)), dim3(THREADS), 0, st, H, d_bin, finite, n_struct,
                           n_types, n_bins, w, P);
        if ((rc = codlad_check_launch(what))) return rc;
        hipLaunchKernelGGL(pr_moments_kernel, dim3(blocks_of(n_struct)), dim3(THREADS), 0, st, P, d_bin, finite, n_struct, n_types,
                           n_bins, count, w, r2, I0, m2);
        if ((rc = codlad_check_launch(what))) return rc;
        if (mean_P) {
            hipLaunchKernelGGL(hist_mean_kernel, dim3(blocks_of(n_bins)), dim3(THREADS), 0, st, P, complete, n_struct, n_bins, mean_P);
            if ((rc = codlad_check_launch(what))) return rc;
        }
    }
    return 0;
}
