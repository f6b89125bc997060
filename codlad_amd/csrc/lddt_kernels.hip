// lDDT of generated structures against the true frames (codlad_lddt, include/codlad_hip.h): per atom the number of
// partners within `cutoff` on the reference and, per threshold, the number of those whose distance the model keeps;
// per residue and per structure the integer sums of those and the scores made from them.  An all-pairs pass per structure
// over the FULL SQUARE of selected atoms: every per-atom row has one writer, and no floating-point value is ever summed.
//
// Atoms are addressed by their POSITION p in the selection (sel[p] = the atom; no selection: p itself).
//
// pair_kernel: one workgroup = one structure x one block of ROWS row positions; a thread owns one row position - its
// reference and model coordinates and its residue in registers - and walks the columns, which are staged through LDS in
// tiles of COLS positions as two float4: {reference x, y, z, residue} and {model x, y, z, -}.  All lanes read the same LDS
// address (a broadcast), so any number of atoms works with 16 KiB of LDS.  The model tile is read, and the two roots are
// taken, only for the pairs that pass the inclusion test.
//
// The inclusion test is d_ref < cutoff with d_ref = sqrtf(d2).  sqrtf is correctly rounded and monotonic, so there is one
// float c2 - the smallest with sqrtf(c2) >= cutoff, found on the host by a few nextafterf steps from cutoff * cutoff - with
//   sqrtf(d2) < cutoff  <=>  d2 < c2        for every d2 that is a number (for a NaN both are false)
// and the kernel compares d2: the same decision bit for bit, without the root for the pairs that fail.
//
// Symmetric side chains: a position's model coordinates are read through one of three maps - PLAIN (itself), SWAP_ALL
// (its swap partner) or CHOSEN (its partner iff swapped[s][residue] is set) - chosen per launch for the rows and for the
// columns.  Same-residue pairs are never counted (seq_sep >= 1), so every partner of a row lies outside its residue: rows
// SWAP_ALL against columns PLAIN scores every residue swapped against an unswapped rest, all residues at once.  Only atoms
// that the swap moves can change a residue's sum, so the decision launch walks the list of moved positions only - about
// a tenth of the rows, which would leave most of the device idle behind a handful of workgroups that each walk every
// column.  So it is cut by column tile and by naming as well: a workgroup takes one block of moved rows, ONE column tile
// and one of PLAIN / SWAP_ALL, and adds each row's sum over the thresholds to its residue's entry of a table the call
// zeroes first - integer atomics, order-independent.  decide_kernel compares the two entries.  The final launch is CHOSEN /
// CHOSEN over all rows and writes the reported counts, one writer each.
//
// finite_kernel marks the structures whose selected model or reference coordinates hold a NaN or +-inf; reduce_kernel
// sums per residue (a CSR of positions by residue, one thread per residue, index order) and per structure (an integer tree
// in LDS), divides once in float64, and gives such a structure -1 in every count and NaN in every score.
//
// Every index a table supplies is clamped before it is used: a wrong table gives wrong counts, never an access out of
// bounds.  Compiled with -ffp-contract=off: distances are structure_math.h's dist2, as geometry_kernels.hip's.
#include <cmath>

#include "common.h"
#include "host_util.h"
#include "structure_math.h"

namespace {
constexpr int ROWS = 128;        // row positions per workgroup = threads per workgroup
constexpr int COLS = 512;        // positions per LDS column tile (two float4 each: 16 KiB)
constexpr int RED = 256;         // threads of the per-structure kernels
constexpr int MAX_T = CODLAD_LDDT_MAX_THRESHOLDS;
enum { PLAIN = 0, SWAP_ALL = 1, CHOSEN = 2 };

struct Thr { float t[MAX_T]; };
struct Tables {
    const int32_t *sel;          // [m] or null
    const int32_t *res;          // [m] the residue of a position
    const int32_t *partner;      // [m] the swap partner of a position (itself: none), null without symmetry
    const uint8_t *swapped;      // [S][R]
    int n, m, R;
};

__device__ inline int atom_of(const Tables &tb, int p) { return tb.sel ? clampi(tb.sel[p], 0, tb.n - 1) : p; }
__device__ inline int residue_of(const Tables &tb, int p) { return clampi(tb.res[p], 0, tb.R - 1); }
// the position whose MODEL coordinates position p (of residue r, structure s) reads
__device__ inline int model_pos(const Tables &tb, int mode, int s, int p, int r) {
    if (mode == PLAIN || !tb.partner) return p;
    if (mode == CHOSEN && !tb.swapped[(size_t)s * tb.R + r]) return p;
    return clampi(tb.partner[p], 0, tb.m - 1);
}

// DECIDE: blockIdx.x = ((s * row_blocks + rb) * tiles + column tile) * 2 + naming, sums to dec [S][R][2]; otherwise
// blockIdx.x = s * row_blocks + rb, every column, counts to atom_total / atom_pres
template <int TN, bool DECIDE>
__global__ __launch_bounds__(ROWS) void pair_kernel(const float *xyz, const float *ref, const int32_t *ref_index, int n_ref,
                                                    Tables tb, const int32_t *rows, int n_rows, int row_blocks, int row_mode,
                                                    int col_mode, float c2, Thr thr, int n_thr, int seq_sep,
                                                    int32_t *atom_total, int32_t *atom_pres, unsigned long long *dec) {
    __shared__ float4 tile_r[COLS];
    __shared__ float4 tile_m[COLS];
    int wg = blockIdx.x, c_lo = 0, c_hi = tb.m;
    if (DECIDE) {
        const int tiles = (tb.m + COLS - 1) / COLS;
        row_mode = (wg & 1) ? SWAP_ALL : PLAIN;
        wg >>= 1;
        c_lo = (wg % tiles) * COLS, c_hi = min(c_lo + COLS, tb.m);
        wg /= tiles;
    }
    const int s = wg / row_blocks, rb = wg % row_blocks;
    const float *xm = xyz + (size_t)s * tb.n * 3;
    const float *xr = ref + (size_t)clampi(ref_index[s], 0, n_ref - 1) * tb.n * 3;
    const int q = rb * ROWS + (int)threadIdx.x;
    const bool have = q < n_rows;
    int p = 0, ri = 0;
    float rx = 0.f, ry = 0.f, rz = 0.f, mx = 0.f, my = 0.f, mz = 0.f;
    if (have) {
        p = rows ? clampi(rows[q], 0, tb.m - 1) : q;
        ri = residue_of(tb, p);
        const int a = atom_of(tb, p), am = atom_of(tb, model_pos(tb, row_mode, s, p, ri));
        rx = xr[3 * a], ry = xr[3 * a + 1], rz = xr[3 * a + 2];
        mx = xm[3 * am], my = xm[3 * am + 1], mz = xm[3 * am + 2];
    }
    int total = 0;
    int pres[TN];
#pragma unroll
    for (int k = 0; k < TN; ++k) pres[k] = 0;

    for (int c0 = c_lo; c0 < c_hi; c0 += COLS) {
        const int width = min(COLS, c_hi - c0);
        __syncthreads();                                  // the previous tile has been read
        for (int k = threadIdx.x; k < width; k += ROWS) {
            const int j = c0 + k, rj = residue_of(tb, j);
            const int a = atom_of(tb, j), am = atom_of(tb, model_pos(tb, col_mode, s, j, rj));
            tile_r[k] = make_float4(xr[3 * a], xr[3 * a + 1], xr[3 * a + 2], __int_as_float(rj));
            tile_m[k] = make_float4(xm[3 * am], xm[3 * am + 1], xm[3 * am + 2], 0.f);
        }
        __syncthreads();
        if (!have) continue;
        for (int k = 0; k < width; ++k) {
            const float4 a = tile_r[k];
            const float d2 = dist2(rx, ry, rz, a.x, a.y, a.z);
            // a position is no partner of itself: it is of its own residue and seq_sep >= 1
            if (d2 < c2 && abs(ri - __float_as_int(a.w)) >= seq_sep) {
                const float4 b = tile_m[k];
                const float d_ref = sqrtf(d2), d_mod = sqrtf(dist2(mx, my, mz, b.x, b.y, b.z));
                const float diff = fabsf(d_mod - d_ref);
                ++total;
#pragma unroll
                for (int t = 0; t < TN; ++t) pres[t] += diff < thr.t[t];
            }
        }
    }
    if (!have) return;
    if (DECIDE) {
        int kept = 0;                                     // the padding thresholds have counted nothing
#pragma unroll
        for (int t = 0; t < TN; ++t) kept += pres[t];
        if (kept) atomicAdd(dec + ((size_t)s * tb.R + ri) * 2 + (row_mode == SWAP_ALL), (unsigned long long)kept);
    } else {
        const size_t at = (size_t)s * tb.m + p;
        atom_total[at] = total;
#pragma unroll
        for (int t = 0; t < TN; ++t)
            if (t < n_thr) atom_pres[at * n_thr + t] = pres[t];
    }
}

// finite[s] and the zeroed row of `swapped`: one workgroup per structure
__global__ __launch_bounds__(RED) void finite_kernel(const float *xyz, const float *ref, const int32_t *ref_index, int n_ref,
                                                     Tables tb, uint8_t *finite, uint8_t *swapped) {
    __shared__ int bad_any;
    const int s = blockIdx.x;
    const float *xm = xyz + (size_t)s * tb.n * 3;
    const float *xr = ref + (size_t)clampi(ref_index[s], 0, n_ref - 1) * tb.n * 3;
    if (threadIdx.x == 0) bad_any = 0;
    __syncthreads();
    bool bad = false;
    for (int p = threadIdx.x; p < tb.m; p += RED) {
        const int a = atom_of(tb, p);
        for (int c = 0; c < 3; ++c) bad |= non_finite(xm[3 * a + c]) || non_finite(xr[3 * a + c]);
    }
    if (bad) bad_any = 1;                                 // every writer writes the same value
    for (int r = threadIdx.x; r < tb.R; r += RED) swapped[(size_t)s * tb.R + r] = 0;
    __syncthreads();
    if (threadIdx.x == 0) finite[s] = bad_any ? 0 : 1;
}

// swapped[s][r] = the residue's moved atoms keep strictly more distances when read through the swap: dec [S][R][2] holds
// their sums over positions and thresholds, [0] in their own naming and [1] exchanged
__global__ __launch_bounds__(RED) void decide_kernel(const unsigned long long *dec, int R, const uint8_t *finite,
                                                     uint8_t *swapped) {
    const int s = blockIdx.x;
    if (!finite[s]) return;                               // finite_kernel left the row at 0
    for (int r = threadIdx.x; r < R; r += RED) {
        const size_t at = ((size_t)s * R + r) * 2;
        swapped[(size_t)s * R + r] = dec[at + 1] > dec[at];
    }
}

// per residue and per structure: the integer sums and the scores; a structure that is not finite gets -1 and NaN
__global__ __launch_bounds__(RED) void reduce_kernel(Tables tb, const int32_t *res_ptr, const int32_t *res_pos, int n_thr,
                                                     const uint8_t *finite, int32_t *atom_total, int32_t *atom_pres,
                                                     int32_t *res_total, int32_t *res_pres, double *res_score,
                                                     long long *counts, double *score) {
    __shared__ long long red[RED];
    const int s = blockIdx.x, T = n_thr;
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    if (!finite[s]) {
        for (size_t p = threadIdx.x; p < (size_t)tb.m; p += RED) atom_total[(size_t)s * tb.m + p] = -1;
        for (size_t e = threadIdx.x; e < (size_t)tb.m * T; e += RED) atom_pres[(size_t)s * tb.m * T + e] = -1;
        for (int r = threadIdx.x; r < tb.R; r += RED) {
            res_total[(size_t)s * tb.R + r] = -1;
            res_score[(size_t)s * tb.R + r] = nan;
            for (int t = 0; t < T; ++t) res_pres[((size_t)s * tb.R + r) * T + t] = -1;
        }
        if ((int)threadIdx.x <= T) counts[(size_t)s * (T + 1) + threadIdx.x] = -1;
        if (threadIdx.x == 0) score[s] = nan;
        return;
    }
    long long part[MAX_T + 1];
#pragma unroll
    for (int t = 0; t <= MAX_T; ++t) part[t] = 0;
    for (int r = threadIdx.x; r < tb.R; r += RED) {
        long long sum[MAX_T + 1];
#pragma unroll
        for (int t = 0; t <= MAX_T; ++t) sum[t] = 0;
        const int lo = clampi(res_ptr[r], 0, tb.m), hi = clampi(res_ptr[r + 1], 0, tb.m);
        for (int e = lo; e < hi; ++e) {
            const int p = res_pos[e];
            if ((unsigned)p >= (unsigned)tb.m) continue;
            const size_t at = (size_t)s * tb.m + p;
            sum[0] += atom_total[at];
#pragma unroll
            for (int t = 0; t < MAX_T; ++t)
                if (t < T) sum[t + 1] += atom_pres[at * T + t];
        }
        long long kept = 0;
#pragma unroll
        for (int t = 0; t < MAX_T; ++t)
            if (t < T) {
                res_pres[((size_t)s * tb.R + r) * T + t] = (int32_t)sum[t + 1];      // <= m (m - 1) < 2^31
                kept += sum[t + 1];
            }
        res_total[(size_t)s * tb.R + r] = (int32_t)sum[0];
        res_score[(size_t)s * tb.R + r] = sum[0] ? (double)kept / (double)((long long)T * sum[0]) : nan;
#pragma unroll
        for (int t = 0; t <= MAX_T; ++t) part[t] += sum[t];
    }
    long long all[MAX_T + 1];
#pragma unroll
    for (int t = 0; t <= MAX_T; ++t) {
        __syncthreads();
        red[threadIdx.x] = part[t];
        __syncthreads();
        for (int st = RED / 2; st > 0; st >>= 1) {
            if ((int)threadIdx.x < st) red[threadIdx.x] += red[threadIdx.x + st];
            __syncthreads();
        }
        all[t] = red[0];
    }
    if (threadIdx.x == 0) {
        long long kept = 0;
#pragma unroll
        for (int t = 0; t <= MAX_T; ++t)
            if (t <= T) {
                counts[(size_t)s * (T + 1) + t] = all[t];
                if (t) kept += all[t];
            }
        score[s] = all[0] ? (double)kept / (double)((long long)T * all[0]) : nan;
    }
}

// the smallest float whose correctly rounded root is >= cutoff: sqrtf(d2) < cutoff <=> d2 < it
float inclusion_bound(float cutoff) {
    float x = cutoff * cutoff;
    while (sqrtf(x) >= cutoff) {
        const float y = nextafterf(x, 0.f);
        if (!(sqrtf(y) >= cutoff)) break;
        x = y;
    }
    while (sqrtf(x) < cutoff) x = nextafterf(x, INFINITY);
    return x;
}

template <bool DECIDE>
void launch_pairs(int T, dim3 grid, hipStream_t st, const float *xyz, const float *ref, const int32_t *ref_index, int n_ref,
                  const Tables &tb, const int32_t *rows, int n_rows, int row_blocks, int mode, float c2, const Thr &thr,
                  int seq_sep, int32_t *atom_total, int32_t *atom_pres, unsigned long long *dec) {
    if (T <= 4)
        hipLaunchKernelGGL((pair_kernel<4, DECIDE>), grid, dim3(ROWS), 0, st, xyz, ref, ref_index, n_ref, tb, rows, n_rows,
                           row_blocks, mode, mode, c2, thr, T, seq_sep, atom_total, atom_pres, dec);
    else
        hipLaunchKernelGGL((pair_kernel<MAX_T, DECIDE>), grid, dim3(ROWS), 0, st, xyz, ref, ref_index, n_ref, tb, rows, n_rows,
                           row_blocks, mode, mode, c2, thr, T, seq_sep, atom_total, atom_pres, dec);
}
}  // namespace

extern "C" int codlad_lddt(const float *xyz, int n_struct, const float *ref, int n_ref, const int32_t *ref_index, int n_atoms,
                           const int32_t *sel, int n_sel, const int32_t *res, int n_res, const int32_t *res_ptr,
                           const int32_t *res_pos, const int32_t *partner, const int32_t *moved, int n_moved, float cutoff,
                           const float *thresholds, int n_thresholds, int seq_sep, int32_t *atom_total,
                           int32_t *atom_preserved, int32_t *residue_total, int32_t *residue_preserved,
                           double *residue_score, long long *counts, double *score, uint8_t *swapped, uint8_t *finite,
                           long long *scratch, void *stream) {
    CODLAD_REQUIRE(xyz && ref && ref_index && res && res_ptr && res_pos && thresholds, "null input pointer");
    CODLAD_REQUIRE(atom_total && atom_preserved && residue_total && residue_preserved && residue_score && counts && score &&
                   swapped && finite, "null output pointer");
    CODLAD_REQUIRE(n_struct > 0 && n_ref > 0 && n_atoms > 0 && n_res > 0, "bad counts");
    CODLAD_REQUIRE(n_atoms <= CODLAD_LDDT_MAX_ATOMS, "more than CODLAD_LDDT_MAX_ATOMS atoms (46340): a residue's count would pass 2^31");
    CODLAD_REQUIRE(sel ? (n_sel > 0 && n_sel <= n_atoms) : n_sel == 0, "sel and n_sel disagree");
    CODLAD_REQUIRE(n_thresholds >= 1 && n_thresholds <= MAX_T, "n_thresholds outside 1 .. CODLAD_LDDT_MAX_THRESHOLDS (8)");
    CODLAD_REQUIRE(std::isfinite(cutoff) && cutoff > 0.f, "cutoff is not a positive finite number");
    Thr thr;
    for (int t = 0; t < MAX_T; ++t) {
        thr.t[t] = t < n_thresholds ? thresholds[t] : 0.f;          // |x| < 0 never holds: the padding counts nothing
        CODLAD_REQUIRE(t >= n_thresholds || (std::isfinite(thr.t[t]) && thr.t[t] > 0.f), "a threshold is not a positive finite number");
    }
    CODLAD_REQUIRE(seq_sep >= 1, "seq_sep must be >= 1");
    CODLAD_REQUIRE(n_moved >= 0 && (n_moved == 0 || (partner && moved && scratch)),
                   "symmetric atoms need partner, moved and scratch");
    const int m = sel ? n_sel : n_atoms;
    CODLAD_REQUIRE(n_moved <= m, "more moved positions than positions");
    const int64_t row_blocks = ((int64_t)m + ROWS - 1) / ROWS;
    const int64_t moved_blocks = ((int64_t)n_moved + ROWS - 1) / ROWS, tiles = ((int64_t)m + COLS - 1) / COLS;
    CODLAD_REQUIRE(row_blocks * n_struct < (int64_t)1 << 31 && 2 * tiles * moved_blocks * n_struct < (int64_t)1 << 31,
                   "too many workgroups for one launch");
    hipStream_t st = (hipStream_t)stream;
    const float c2 = inclusion_bound(cutoff);
    const int T = n_thresholds;
    Tables tb = {sel, res, n_moved ? partner : nullptr, swapped, n_atoms, m, n_res};
    hipLaunchKernelGGL(finite_kernel, dim3((unsigned)n_struct), dim3(RED), 0, st, xyz, ref, ref_index, n_ref, tb, finite, swapped);
    if (n_moved) {
        unsigned long long *dec = reinterpret_cast<unsigned long long *>(scratch);
        const hipError_t e = hipMemsetAsync(dec, 0, sizeof(unsigned long long) * 2 * (size_t)n_res * (size_t)n_struct, st);
        if (e != hipSuccess) return codlad_hip_failed("codlad_lddt", e);
        launch_pairs<true>(T, dim3((unsigned)(2 * tiles * moved_blocks * n_struct)), st, xyz, ref, ref_index, n_ref, tb, moved,
                           n_moved, (int)moved_blocks, PLAIN, c2, thr, seq_sep, nullptr, nullptr, dec);
        hipLaunchKernelGGL(decide_kernel, dim3((unsigned)n_struct), dim3(RED), 0, st, dec, n_res, finite, swapped);
    }
    const int mode = n_moved ? CHOSEN : PLAIN;
    launch_pairs<false>(T, dim3((unsigned)(row_blocks * n_struct)), st, xyz, ref, ref_index, n_ref, tb, nullptr, m,
                        (int)row_blocks, mode, c2, thr, seq_sep, atom_total, atom_preserved, nullptr);
    hipLaunchKernelGGL(reduce_kernel, dim3((unsigned)n_struct), dim3(RED), 0, st, tb, res_ptr, res_pos, T, finite, atom_total,
                       atom_preserved, residue_total, residue_preserved, residue_score, counts, score);
    return codlad_check_launch("codlad_lddt");
}
