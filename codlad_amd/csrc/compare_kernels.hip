// Comparing two ensembles (codlad_dist_hist, codlad_column_hist, codlad_hist_divergence; include/codlad_hip.h): integer
// count tables over the STRUCTURES of a pool - per atom pair the histogram of its distance, per column of a table of
// per-structure values the histogram of the column - and the float64 divergences of two such tables, row by row.
//
// codlad_dist_hist, three launches on the caller's stream:
//   compare_fill_kernel     H = 0, n_counted = 0: the call writes every element
//   compare_finite_kernel   one wave per structure: finite[s] over the SELECTED atoms, n_counted by an integer atomic add
//   dist_hist_kernel        one workgroup of 256 lanes per (tile of TI x TJ selection positions, chunk of structures).  The
//                           histograms of the tile's PT = TI * TJ pairs live in LDS as hist[column][pair]: lane l of a
//                           32-lane group touches bank l whatever its column is, so the adds never conflict.  PT is the
//                           largest of 256, 128, 64, 32 whose table fits (256 up to 54 bins, 32 at 256 bins); the 256 / PT
//                           lane groups of a pair take the structures of a batch in turn.  The coordinates of the tile's
//                           TI + TJ atoms for a batch of 16 structures are staged through LDS once (component-major, the
//                           next batch already on its way in registers) and reused by every pair.  Per pair the header's
//                           fp32 sequence and an LDS add on int; the non-zero counts go to H by integer atomic adds.
// codlad_column_hist: the same shape over a table of doubles - a workgroup owns 32 columns (a 256-byte run of every row)
// and a chunk of the structures, hist[column of H][column of values] in LDS.
// Integer adds commute: no count depends on the order in which lanes, workgroups or chunks arrive, on the number of
// chunks, or on where a structure stands in the pool.  No floating-point atomics anywhere.
// codlad_hist_divergence: one wave per row; the lanes compute the terms of 64 columns, lane 0 adds them in ascending k.
// -ffp-contract=off: one rounding per operation, in fp32 and in float64.
#include "common.h"
#include "reduce_math.h"
#include "structure_math.h"

namespace {
constexpr int WAVE = 64;
constexpr int THREADS = 256;
constexpr int BATCH = 16;                              // structures staged at a time
constexpr int MAX_TILE_ATOMS = 32;                     // TI + TJ of the largest tile
constexpr int HIST_LDS_BYTES = 56 * 1024;              // of the pair histograms; the staged coordinates take 6 KB more
constexpr int COL_TILE = 32;                           // columns of values per workgroup
constexpr int COL_ROWS = THREADS / COL_TILE;           // structures in flight per workgroup
constexpr int TARGET_GROUPS = 1024;                    // workgroups that fill the device: 4 per compute unit
constexpr int FILL_BLOCKS = 2048;

// NaN or +-inf by the exponent bits, structure_math.h's non_finite for a double (another body than reduce_math.h's fin64)
__device__ inline bool non_finite64(double v) {
    return ((unsigned long long)__double_as_longlong(v) & 0x7ff0000000000000ull) == 0x7ff0000000000000ull;
}

__global__ __launch_bounds__(THREADS) void compare_fill_kernel(int32_t *H, int64_t n, int32_t *extra, int n_extra) {
    const int64_t stride = (int64_t)gridDim.x * THREADS, first = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    for (int64_t e = first; e < n; e += stride) H[e] = 0;
    for (int64_t e = first; e < n_extra; e += stride) extra[e] = 0;
}

// one wave per structure, the selected atoms only
__global__ __launch_bounds__(WAVE) void compare_finite_kernel(const float *x, int n_atoms, const int32_t *sel, int m,
                                                              uint8_t *finite, int32_t *n_counted) {
    const float *xs = x + (size_t)blockIdx.x * n_atoms * 3;
    int bad = 0;
    for (int k = threadIdx.x; k < m; k += WAVE) {
        const int a = sel ? clampi(sel[k], 0, n_atoms - 1) : k;
        bad |= non_finite(xs[3 * a]) | non_finite(xs[3 * a + 1]) | non_finite(xs[3 * a + 2]);
    }
    bad = __syncthreads_or(bad);
    if (threadIdx.x == 0) {
        finite[blockIdx.x] = bad ? 0 : 1;
        if (!bad) atomicAdd(n_counted, 1);
    }
}

// grid (row tiles * column tiles, chunks); dynamic LDS: PT * cols ints, then 3 * BATCH * MAX_TILE_ATOMS floats, then BATCH ints
__global__ __launch_bounds__(THREADS) void dist_hist_kernel(const float *x, int N, int n_atoms, const int32_t *sel, int m,
                                                            float inv_dr, int n_bins, int ti_log, int tj_log, int n_tj,
                                                            const uint8_t *finite, int32_t *H) {
    extern __shared__ int lds[];
    const int TI = 1 << ti_log, TJ = 1 << tj_log, PT = TI * TJ, A = TI + TJ, cols = n_bins + 2;
    const int r0 = (int)(blockIdx.x / n_tj) * TI, c0 = (int)(blockIdx.x % n_tj) * TJ;
    if (c0 + TJ - 1 <= r0) return;                                // uniform: no pair i < j in this tile
    int *hist = lds;
    float *cx = reinterpret_cast<float *>(lds + PT * cols), *cy = cx + BATCH * MAX_TILE_ATOMS, *cz = cy + BATCH * MAX_TILE_ATOMS;
    int *ok = reinterpret_cast<int *>(cz + BATCH * MAX_TILE_ATOMS);
    for (int e = threadIdx.x; e < PT * cols; e += THREADS) hist[e] = 0;

    // what this lane stages: items e = lane, lane + 256 of a batch's BATCH * A (structure, atom) slots (A <= 32: two at most)
    int st_s[2], st_a[2];
    bool st_on[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        const int e = threadIdx.x + u * THREADS;
        st_on[u] = e < BATCH * A;
        st_s[u] = e / A;
        const int k = e % A, pos = k < TI ? r0 + k : c0 + (k - TI);
        const int pc = pos < m ? pos : m - 1;                     // a position past the selection is staged and never counted
        st_a[u] = sel ? clampi(sel[pc], 0, n_atoms - 1) : pc;
    }
    const int pl = threadIdx.x & (PT - 1), g = threadIdx.x / PT, G = THREADS / PT;
    const int ti = pl >> tj_log, tj = pl & (TJ - 1);
    const int ip = r0 + ti, jp = c0 + tj;
    const bool pair = ip < jp && jp < m;
    const float bins_f = (float)n_bins;
    const int n_batches = (N + BATCH - 1) / BATCH;

    float rx[2], ry[2], rz[2];
    int rok = 0;
    auto fetch = [&](int b) {
        const int s0 = b * BATCH;
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            rx[u] = ry[u] = rz[u] = 0.f;
            const int s = s0 + st_s[u];
            if (st_on[u] && s < N) {
                const float *p = x + ((size_t)s * n_atoms + st_a[u]) * 3;
                rx[u] = p[0], ry[u] = p[1], rz[u] = p[2];
            }
        }
        rok = threadIdx.x < BATCH && s0 + (int)threadIdx.x < N ? finite[s0 + threadIdx.x] : 0;
    };
    int b = blockIdx.y;
    if (b < n_batches) fetch(b);
    for (; b < n_batches; b += gridDim.y) {
        __syncthreads();                                          // the batch before is counted (first: hist is zero)
#pragma unroll
        for (int u = 0; u < 2; ++u)
            if (st_on[u]) {
                const int at = st_s[u] * MAX_TILE_ATOMS + (threadIdx.x + u * THREADS) % A;
                cx[at] = rx[u], cy[at] = ry[u], cz[at] = rz[u];
            }
        if (threadIdx.x < BATCH) ok[threadIdx.x] = rok;
        __syncthreads();
        if (b + (int)gridDim.y < n_batches) fetch(b + gridDim.y);   // in flight under the pairs below
        if (pair) {
            for (int sl = g; sl < BATCH; sl += G) {
                if (!ok[sl]) continue;                            // past the pool, or not finite: it takes no part
                const int at = sl * MAX_TILE_ATOMS;
                const float dx = cx[at + TI + tj] - cx[at + ti], dy = cy[at + TI + tj] - cy[at + ti],
                            dz = cz[at + TI + tj] - cz[at + ti];
                const float r = sqrtf((dx * dx + dy * dy) + dz * dz);
                const float t = r * inv_dr;
                const int col = t < bins_f ? 1 + (int)t : n_bins + 1;
                atomicAdd(&hist[col * PT + pl], 1);
            }
        }
    }
    __syncthreads();
    for (int e = threadIdx.x; e < PT * cols; e += THREADS) {
        const int v = hist[e];
        if (!v) continue;                                         // a pair outside the triangle never counted
        const int q = e & (PT - 1), col = e / PT;
        const int i = r0 + (q >> tj_log), j = c0 + (q & (TJ - 1));
        atomicAdd(&H[(size_t)CODLAD_DIST_HIST_PAIR(i, j, m) * cols + col], v);
    }
}

// grid (blocks of 32 columns, chunks of structures); LDS: (cols + 1) * 32 ints, the last row the valid counts
__global__ __launch_bounds__(THREADS) void column_hist_kernel(const double *values, int N, int C, double lo, double inv_width,
                                                              int n_bins, int periodic, int32_t *H, int32_t *n_valid) {
    extern __shared__ int lds[];
    const int cols = n_bins + 2;
    for (int e = threadIdx.x; e < (cols + 1) * COL_TILE; e += THREADS) lds[e] = 0;
    __syncthreads();
    const int cl = threadIdx.x & (COL_TILE - 1), c = blockIdx.x * COL_TILE + cl;
    if (c < C) {
        for (int s = blockIdx.y * COL_ROWS + threadIdx.x / COL_TILE; s < N; s += gridDim.y * COL_ROWS) {
            const double v = values[(size_t)s * C + c];
            if (non_finite64(v)) continue;
            const double t = (v - lo) * inv_width;
            int col;
            if (periodic) {
                if (!(fabs(t) < 2147483648.0)) continue;          // outside the admissible range: invalid
                int64_t k = (int64_t)floor(t) % n_bins;
                if (k < 0) k += n_bins;
                col = 1 + (int)k;
            } else {
                col = t < 0.0 ? 0 : floor(t) >= (double)n_bins ? n_bins + 1 : 1 + (int)floor(t);
            }
            atomicAdd(&lds[col * COL_TILE + cl], 1);
            atomicAdd(&lds[cols * COL_TILE + cl], 1);
        }
    }
    __syncthreads();
    for (int e = threadIdx.x; e < (cols + 1) * COL_TILE; e += THREADS) {
        const int v = lds[e], col = e / COL_TILE, cc = blockIdx.x * COL_TILE + (e & (COL_TILE - 1));
        if (!v || cc >= C) continue;
        if (col < cols) atomicAdd(&H[(size_t)cc * cols + col], v);
        else atomicAdd(&n_valid[cc], v);
    }
}

// one wave per row
__global__ __launch_bounds__(WAVE) void hist_divergence_kernel(const int32_t *HA, const int32_t *HB, int cols, double *js,
                                                               double *tv, double *w1) {
    __shared__ double term[WAVE], gap[WAVE], ps[WAVE], qs[WAVE];
    const int32_t *a = HA + (size_t)blockIdx.x * cols, *b = HB + (size_t)blockIdx.x * cols;
    long long nA = 0, nB = 0;
    int neg = 0;
    for (int k = threadIdx.x; k < cols; k += WAVE) nA += a[k], nB += b[k], neg |= (a[k] < 0) | (b[k] < 0);
    nA = wave_sum(nA), nB = wave_sum(nB);
    neg = __syncthreads_or(neg);
    if (neg || nA == 0 || nB == 0) {                              // uniform
        if (threadIdx.x == 0) js[blockIdx.x] = tv[blockIdx.x] = w1[blockIdx.x] = nan64();
        return;
    }
    const double dA = (double)nA, dB = (double)nB;
    double sj = 0.0, sv = 0.0, sw = 0.0, cA = 0.0, cB = 0.0;      // lane 0's
    for (int k0 = 0; k0 < cols; k0 += WAVE) {
        const int k = k0 + threadIdx.x;
        if (k < cols) {
            const double p = (double)a[k] / dA, q = (double)b[k] / dB, mid = 0.5 * (p + q);
            const double tp = a[k] > 0 ? p * log2(p / mid) : 0.0, tq = b[k] > 0 ? q * log2(q / mid) : 0.0;
            term[threadIdx.x] = tp + tq, gap[threadIdx.x] = fabs(p - q), ps[threadIdx.x] = p, qs[threadIdx.x] = q;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            const int cnt = cols - k0 < WAVE ? cols - k0 : WAVE;
            for (int l = 0; l < cnt; ++l) {
                sj += term[l], sv += gap[l];
                cA += ps[l], cB += qs[l];
                if (k0 + l < cols - 1) sw += fabs(cA - cB);
            }
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) js[blockIdx.x] = 0.5 * sj, tv[blockIdx.x] = 0.5 * sv, w1[blockIdx.x] = sw;
}

// the tile of a histogram width: the largest PT = 2^(ti + tj) of 256, 128, 64, 32 whose table fits HIST_LDS_BYTES
void tile_of(int n_bins, int &ti_log, int &tj_log) {
    const int room = HIST_LDS_BYTES / 4 / (n_bins + 2);
    if (room >= 256) ti_log = 4, tj_log = 4;
    else if (room >= 128) ti_log = 3, tj_log = 4;
    else if (room >= 64) ti_log = 3, tj_log = 3;
    else ti_log = 2, tj_log = 3;
}

bool positive_finite(double v) { return v > 0.0 && v <= 1.7976931348623157e308; }
unsigned fill_blocks(int64_t n) {
    const int64_t need = (n + THREADS - 1) / THREADS;
    return (unsigned)(need < 1 ? 1 : need < FILL_BLOCKS ? need : FILL_BLOCKS);
}
}  // namespace

extern "C" long long codlad_dist_hist_bytes(int m, int n_bins) {
    CODLAD_REQUIRE(m >= 2 && m <= CODLAD_DIST_HIST_MAX_SEL, "m outside 2 .. 2048");
    CODLAD_REQUIRE(n_bins >= 1 && n_bins <= CODLAD_COMPARE_MAX_BINS, "n_bins outside 1 .. 256");
    const long long words = (long long)m * (m - 1) / 2 * (n_bins + 2);
    CODLAD_REQUIRE(words < 1ll << 31, "P * (n_bins + 2) reaches 2^31");
    return 4 * words;
}

extern "C" long long codlad_column_hist_bytes(int C, int n_bins) {
    CODLAD_REQUIRE(C >= 1 && C <= CODLAD_COMPARE_MAX_ROWS, "C outside 1 .. 1048576");
    CODLAD_REQUIRE(n_bins >= 1 && n_bins <= CODLAD_COMPARE_MAX_BINS, "n_bins outside 1 .. 256");
    return 4ll * C * (n_bins + 2);
}

extern "C" int codlad_dist_hist(const float *x, int N, int n_atoms, const int32_t *sel, int n_sel, float inv_dr, int n_bins,
                                int32_t *H, uint8_t *finite, int32_t *n_counted, void *stream) {
    CODLAD_REQUIRE(x && H && finite && n_counted, "null pointer");
    CODLAD_REQUIRE(N >= 1 && N <= CODLAD_COMPARE_MAX_ROWS, "N outside 1 .. 1048576");
    CODLAD_REQUIRE(n_atoms >= 1 && n_sel >= 0, "bad counts");
    CODLAD_REQUIRE((sel != nullptr) == (n_sel > 0), "sel and n_sel disagree");
    const int m = sel ? n_sel : n_atoms;
    CODLAD_REQUIRE(m >= 2 && m <= CODLAD_DIST_HIST_MAX_SEL, "m outside 2 .. 2048");
    CODLAD_REQUIRE(n_bins >= 1 && n_bins <= CODLAD_COMPARE_MAX_BINS, "n_bins outside 1 .. 256");
    CODLAD_REQUIRE(inv_dr > 0.f && inv_dr <= 3.402823466e38f, "inv_dr is not a positive finite number");
    const int64_t words = (int64_t)m * (m - 1) / 2 * (n_bins + 2);
    CODLAD_REQUIRE(words < (int64_t)1 << 31, "P * (n_bins + 2) reaches 2^31");
    const char *what = "codlad_dist_hist";
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(compare_fill_kernel, dim3(fill_blocks(words)), dim3(THREADS), 0, st, H, words, n_counted, 1);
    int rc = codlad_check_launch(what);
    if (rc) return rc;
    hipLaunchKernelGGL(compare_finite_kernel, dim3((unsigned)N), dim3(WAVE), 0, st, x, n_atoms, sel, m, finite, n_counted);
    if ((rc = codlad_check_launch(what))) return rc;
    int ti_log, tj_log;
    tile_of(n_bins, ti_log, tj_log);
    const int TI = 1 << ti_log, TJ = 1 << tj_log, n_ti = (m + TI - 1) / TI, n_tj = (m + TJ - 1) / TJ;
    // when the triangle has few tiles the structures are cut into chunks that fill the device (counts do not depend on it)
    const int64_t tiles = ((int64_t)n_ti * n_tj + 1) / 2;
    const int batches = (N + BATCH - 1) / BATCH;
    int64_t chunks = (TARGET_GROUPS + tiles - 1) / tiles;
    chunks = chunks < 1 ? 1 : chunks > batches ? batches : chunks;
    const size_t lds = (size_t)(TI * TJ) * (n_bins + 2) * 4 + 3 * BATCH * MAX_TILE_ATOMS * 4 + BATCH * 4;
    hipLaunchKernelGGL(dist_hist_kernel, dim3((unsigned)(n_ti * n_tj), (unsigned)chunks), dim3(THREADS), lds, st, x, N, n_atoms,
                       sel, m, inv_dr, n_bins, ti_log, tj_log, n_tj, finite, H);
    return codlad_check_launch(what);
}

extern "C" int codlad_column_hist(const double *values, int N, int C, double lo, double inv_width, int n_bins, int periodic,
                                  int32_t *H, int32_t *n_valid, void *stream) {
    CODLAD_REQUIRE(values && H && n_valid, "null pointer");
    CODLAD_REQUIRE(N >= 1 && N <= CODLAD_COMPARE_MAX_ROWS, "N outside 1 .. 1048576");
    CODLAD_REQUIRE(C >= 1 && C <= CODLAD_COMPARE_MAX_ROWS, "C outside 1 .. 1048576");
    CODLAD_REQUIRE(n_bins >= 1 && n_bins <= CODLAD_COMPARE_MAX_BINS, "n_bins outside 1 .. 256");
    CODLAD_REQUIRE(lo >= -1.7976931348623157e308 && lo <= 1.7976931348623157e308, "lo is not finite");
    CODLAD_REQUIRE(positive_finite(inv_width), "inv_width is not a positive finite number");
    CODLAD_REQUIRE(periodic == 0 || periodic == 1, "periodic is neither 0 nor 1");
    const char *what = "codlad_column_hist";
    hipStream_t st = (hipStream_t)stream;
    const int64_t words = (int64_t)C * (n_bins + 2);
    hipLaunchKernelGGL(compare_fill_kernel, dim3(fill_blocks(words)), dim3(THREADS), 0, st, H, words, n_valid, C);
    int rc = codlad_check_launch(what);
    if (rc) return rc;
    const int blocks = (C + COL_TILE - 1) / COL_TILE, rounds = (N + COL_ROWS - 1) / COL_ROWS;
    int chunks = (TARGET_GROUPS + blocks - 1) / blocks;
    chunks = chunks < 1 ? 1 : chunks > rounds ? rounds : chunks;
    hipLaunchKernelGGL(column_hist_kernel, dim3((unsigned)blocks, (unsigned)chunks), dim3(THREADS),
                       (size_t)(n_bins + 3) * COL_TILE * 4, st, values, N, C, lo, inv_width, n_bins, periodic, H, n_valid);
    return codlad_check_launch(what);
}

extern "C" int codlad_hist_divergence(const int32_t *HA, const int32_t *HB, int rows, int cols, double *js, double *tv,
                                      double *w1, void *stream) {
    CODLAD_REQUIRE(HA && HB && js && tv && w1, "null pointer");
    CODLAD_REQUIRE(cols >= 2 && cols <= CODLAD_DIVERGENCE_MAX_COLS, "cols outside 2 .. 4098");
    CODLAD_REQUIRE(rows >= 1 && (int64_t)rows * cols < (int64_t)1 << 31, "rows outside 1 .. (2^31 - 1) / cols");
    hipLaunchKernelGGL(hist_divergence_kernel, dim3((unsigned)rows), dim3(WAVE), 0, (hipStream_t)stream, HA, HB, cols, js, tv, w1);
    return codlad_check_launch("codlad_hist_divergence");
}
