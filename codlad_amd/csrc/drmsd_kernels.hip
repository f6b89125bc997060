// Superposition-free distance RMSD (include/codlad_hip.h, codlad_drmsd_matrix and codlad_drmsd_pairs): the structural
// distance of two conformations of a disordered chain, msd_ij = sum_p (d_p(i) - d_p(j))^2 / P over the P pairs of chain
// positions k < l, l - k >= min_sep, with d_p the fp32 pair distance (pair_hist_kernels.hip's sequence).
//
// The matrix is the Gram form msd_ij = max(G_i + G_j - 2 C_ij, 0) / P, C = D D^T over the vectors D of pair distances,
// one float64 matrix product on v_mfma_f64_16x16x4_f64 (cluster_kernels.hip's 64 x 64 block, wave tiles, bitmap and
// one-writer discipline).  What is new is the operand: element (structure, p) is d_p(structure), made inside the kernel
// from the coordinates and never stored as a table.
//   finite_kernel   a wave per structure: finite[i] = no NaN and no infinity among its selected atoms.
//   gram_kernel     workgroup (J, I, slab) of 8 waves owns the pairs of the structure blocks I and J (64 + 64 structures).
//                   The pair triangle is walked in windows of 16 x 16 chain positions (rows k, columns l), row of
//                   windows by row of windows: the 16 row atoms of the 128 structures are staged in LDS once per row of
//                   windows, thread (structure s = t & 127, quarter q = t >> 7) keeps the window's column atoms 4 q .. 4 q + 3
//                   of its structure in registers.  Two window rows (32 slots) at a time the threads write their 8
//                   distances as fp32 into the panel [slot][structure] in LDS; the MFMA operand (row lane & 15, k lane
//                   >> 4) is read from it and converted to float64 on the read, which is exact.  A slot that is no pair
//                   and every slot of a structure that is not finite or not there is an exact zero; window rows and
//                   windows without a pair are skipped (zeros add nothing to a sum that starts at +0).
//                   NORM: blocks (I, I), the four diagonal wave tiles only, the diagonal of the product -> G.
//                   Split (grid z = slabs): the workgroup writes its slab's partial block, in register layout, to the
//                   scratch; finish_kernel adds the partials in ascending slab order and runs the same tail.  Unsplit: the
//                   workgroup runs the slabs in ascending order, each from zero into `acc`, and adds them to `tot` in
//                   that order - the same additions.
//   tail            per lane, the pairs (row q + 4 reg of tile ti, column lr of tile tj): msd, the table (one pool: the
//                   element and its mirror from the same lane), the decision through __ballot into 16-bit segments.
// The products d_p(i) d_p(j) are exact in float64 (24 x 24 bits) and commute, so C_ij = C_ji to the bit whatever the
// MFMA's order inside a K step, and C_ii' = C_ii = C_i'i' for two structures with the same distance vector: exactly 0.
// No atomics, no scratch memory, no spills.  As built for gfx950 (kernel-resource-usage): gram_kernel 73 / 74 / 74 VGPRs
// (norm, one pool, two pools), no AGPRs, 43.2 KiB of LDS (24.2 KiB staged row atoms, 18 KiB panel, 1 KiB bitmap segments):
// the LDS allows three workgroups a compute unit - 6 waves per SIMD - so other workgroups' MFMAs run under this one's
// barriers and distance arithmetic; finish_kernel 44 VGPRs, pairs_kernel 43, 8 waves per SIMD.  Measured
// (profiles/drmsd_cost.txt): 37 TFLOP/s of executed MFMA work at (16 384, 129), operand generation included.  Not
// built, so not measured: float64 panels (36 KiB: two workgroups a compute unit, no conversion on the operand read);
// 16 x 16 windows with BOTH atom sets in LDS (48 KiB + panels) do not fit 64 KiB.
//
// codlad_drmsd_pairs: pairs_kernel, the direct sum in float64 for a list of pairs, a workgroup per pair; its order is in
// the header.
#include "common.h"
#include "host_util.h"
#include "reduce_math.h"
#include "structure_math.h"

namespace {
constexpr int MAX_N = CODLAD_CLUSTER_MAX_N;
constexpr int MAX_SEL = CODLAD_DRMSD_MAX_SEL;
constexpr int BLK = 64;                     // structures of a block = bits of a word
constexpr int WIN = CODLAD_DRMSD_WINDOW;    // chain positions of a window's side
constexpr int SLAB = CODLAD_DRMSD_SLAB_TILES;
constexpr int NW = 8, TJ = 2;               // waves of a workgroup, wave tiles of a wave
constexpr int MT = NW * 64;
constexpr int KC = 2 * WIN;                 // slots of a panel: two window rows, 8 MFMA steps
constexpr int PROW = 2 * BLK + 16;          // floats of a slot of the panel: the four k of an operand on other banks
constexpr int RROW = 2 * BLK + 1;           // floats of an (atom, component) of the staged rows
constexpr int PART = BLK * BLK;             // doubles of a partial block
static_assert(WIN == 16 && MT == 4 * 2 * BLK && NW * TJ == 16, "a thread per (structure, quarter of the window's columns)");

enum { MODE_NORM = 0, MODE_ONE = 1, MODE_CROSS = 2 };

struct Prm {
    const float *x, *y;                     // the pool of the row blocks and of the column blocks (one pool: the same)
    const uint8_t *fx, *fy;
    const double *gx, *gy;
    const int32_t *sel;
    int Na, Nb, n_atoms, m, min_sep, T, n_tiles, n_slabs, split, squared, W;
    double P, cut2;
    double *out;
    unsigned long long *bits;
    double *gdst;                           // NORM: G [N_pad], or with split the partials [slab][g_stride]
    int g_stride;
    double *part;                           // split: [block][slab][PART]
};

__device__ __forceinline__ int row_of(const int32_t *sel, int k, int n_atoms) { return sel ? clampi(sel[k], 0, n_atoms - 1) : k; }

__global__ __launch_bounds__(256) void finite_kernel(const float *x, int N, int n_atoms, const int32_t *sel, int m, uint8_t *finite) {
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (i >= N) return;                                              // uniform in the wave
    const float *xs = x + (size_t)i * n_atoms * 3;
    int bad = 0;
    for (int k = lane; k < m; k += 64) {
        const size_t a = row_of(sel, k, n_atoms);
        bad |= non_finite(xs[3 * a]) | non_finite(xs[3 * a + 1]) | non_finite(xs[3 * a + 2]);
    }
    bad = wave_sum(bad);
    if (lane == 0) finite[i] = bad ? 0 : 1;
}

// the block of the upper triangle of nb x nb blocks, row by row
__device__ __host__ inline long long tri_block(int I, int J, int nb) { return (long long)I * nb - (long long)I * (I - 1) / 2 + (J - I); }

__device__ __forceinline__ double pick(const double4_t &v, int reg) { return reg == 0 ? v.x : reg == 1 ? v.y : reg == 2 ? v.z : v.w; }

// The pairs (row lk + 4 reg of wave tile ti, column lr of wave tile tj0 + u) of this lane from their C.
template <int MODE> __device__ __forceinline__ void tail(const Prm &p, int I, int J, const double4_t (&c)[TJ]) {
    __shared__ unsigned short rowseg[BLK][4], colseg[BLK][4];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int ti = wave / (4 / TJ), tj0 = (wave % (4 / TJ)) * TJ;
    const int lr = lane & 15, lk = lane >> 4;
#pragma unroll
    for (int u = 0; u < TJ; ++u) {
        const int tj = tj0 + u, gj = J * BLK + tj * 16 + lr;
        const bool on = MODE == MODE_CROSS || I != J || tj >= ti;    // uniform in the wave
        const bool in_j = gj < p.Nb;
        const bool fj = in_j && p.fy[gj] != 0;
        const double Gj = in_j ? p.gy[gj] : 0.0;
        unsigned colbits = 0;
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            const int gi = I * BLK + ti * 16 + lk + 4 * reg;
            const bool valid = on && gi < p.Na && in_j;
            const bool upper = MODE == MODE_CROSS || gi < gj, diag = MODE != MODE_CROSS && gi == gj;
            const bool fin = valid && fj && p.fx[gi] != 0;
            double msd = nan64();
            if (fin && upper) {
                const double v = (p.gx[gi] + Gj) - 2.0 * pick(c[u], reg);
                msd = (v < 0.0 ? 0.0 : v) / p.P;                     // a NaN stays
            } else if (fin && diag) {
                msd = 0.0;
            }
            if (p.out && valid && (upper || diag)) {
                const double v = p.squared ? msd : sqrt(msd);
                p.out[(size_t)gi * p.Nb + gj] = v;
                if (MODE != MODE_CROSS && upper) p.out[(size_t)gj * p.Nb + gi] = v;
            }
            if (MODE == MODE_ONE) {
                const bool dec = fin && (upper ? msd <= p.cut2 : diag);
                const unsigned long long b = __ballot(dec);
                if (lane < 4) rowseg[ti * 16 + 4 * reg + lane][tj] = (unsigned short)((b >> (16 * lane)) & 0xffffull);
#pragma unroll
                for (int q = 0; q < 4; ++q) colbits |= (unsigned)((b >> (16 * q + lr)) & 1ull) << (4 * reg + q);
            }
        }
        if (MODE == MODE_ONE && lane < 16) colseg[tj * 16 + lane][ti] = (unsigned short)colbits;
    }
    if (MODE != MODE_ONE || !p.bits) return;                         // uniform
    __syncthreads();
    if (t < BLK) {
        const unsigned long long rw = (unsigned long long)rowseg[t][0] | (unsigned long long)rowseg[t][1] << 16 |
                                      (unsigned long long)rowseg[t][2] << 32 | (unsigned long long)rowseg[t][3] << 48;
        const unsigned long long cw = (unsigned long long)colseg[t][0] | (unsigned long long)colseg[t][1] << 16 |
                                      (unsigned long long)colseg[t][2] << 32 | (unsigned long long)colseg[t][3] << 48;
        if (I == J) {
            if (I * BLK + t < p.Na) p.bits[(size_t)(I * BLK + t) * p.W + I] = rw | cw;
        } else {
            if (I * BLK + t < p.Na) p.bits[(size_t)(I * BLK + t) * p.W + J] = rw;
            if (J * BLK + t < p.Na) p.bits[(size_t)(J * BLK + t) * p.W + I] = cw;
        }
    }
}

// grid (column blocks, row blocks, slabs with split else 1)
template <int MODE> __global__ __launch_bounds__(MT) void gram_kernel(Prm p) {
    const int J = MODE == MODE_NORM ? blockIdx.y : blockIdx.x, I = blockIdx.y;
    if (MODE == MODE_ONE && J < I) return;
    __shared__ float rows[WIN * 3 * RROW];
    __shared__ float panel[KC * PROW];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int ti = wave / (4 / TJ), tj0 = (wave % (4 / TJ)) * TJ;
    const int lr = lane & 15, lk = lane >> 4;
    bool on[TJ];
#pragma unroll
    for (int u = 0; u < TJ; ++u)                                     // uniform in the wave
        on[u] = MODE == MODE_NORM ? tj0 + u == ti : MODE == MODE_CROSS || I != J || tj0 + u >= ti;
    // this thread's structure s of the 128 and the quarter q of a window's columns
    const int s = t & (2 * BLK - 1), q = t >> 7;
    const bool second = s >= BLK;
    const int n_pool = second ? p.Nb : p.Na;
    const int gs = (second ? J : I) * BLK + (s & (BLK - 1));
    const bool ok = gs < n_pool && (second ? p.fy : p.fx)[min(gs, n_pool - 1)] != 0;
    const float *xs = (second ? p.y : p.x) + (size_t)min(gs, n_pool - 1) * p.n_atoms * 3;

    double4_t tot[TJ], acc[TJ];
#pragma unroll
    for (int u = 0; u < TJ; ++u) tot[u] = double4_t{0.0, 0.0, 0.0, 0.0};
    const int slab0 = p.split ? blockIdx.z : 0, slab1 = p.split ? slab0 + 1 : p.n_slabs;
    int staged = -1;                                                 // the row of windows whose atoms are in `rows`
    for (int slab = slab0; slab < slab1; ++slab) {
#pragma unroll
        for (int u = 0; u < TJ; ++u) acc[u] = double4_t{0.0, 0.0, 0.0, 0.0};
        int tile = slab * SLAB;
        const int tile_end = min(tile + SLAB, p.n_tiles);
        int tr = 0, left = tile;
        while (left >= p.T - tr) left -= p.T - tr, ++tr;
        int tc = tr + left;
        for (; tile < tile_end; ++tile, ++tc) {
            if (tc == p.T) ++tr, tc = tr;
            const int r0 = tr * WIN, c0 = tc * WIN, lmax = min(c0 + WIN, p.m) - 1;
            if (lmax - r0 < p.min_sep) continue;                     // uniform: no pair in this window
            if (staged != tr) {
                __syncthreads();                                     // the previous row of windows has been read
                for (int e = t; e < 2 * BLK * WIN * 3; e += MT) {
                    const int st = e / (WIN * 3), f = e % (WIN * 3), k = r0 + f / 3;
                    const bool sec = st >= BLK;
                    const int np = sec ? p.Nb : p.Na, g = min((sec ? J : I) * BLK + (st & (BLK - 1)), np - 1);
                    float v = 0.f;
                    if (k < p.m) v = (sec ? p.y : p.x)[((size_t)g * p.n_atoms + row_of(p.sel, k, p.n_atoms)) * 3 + f % 3];
                    rows[f * RROW + st] = v;
                }
                staged = tr;
            }
            float cx[4], cy[4], cz[4];
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const size_t a = row_of(p.sel, min(c0 + 4 * q + c, p.m - 1), p.n_atoms);
                cx[c] = xs[3 * a], cy[c] = xs[3 * a + 1], cz[c] = xs[3 * a + 2];
            }
            for (int k0 = r0; k0 < r0 + WIN; k0 += 2) {
                if (lmax - k0 < p.min_sep) break;                    // uniform: no pair from this window row on
                __syncthreads();                                     // the panel has been read, the staged rows are there
#pragma unroll
                for (int r2 = 0; r2 < 2; ++r2) {
                    const int k = k0 + r2, a3 = (k - r0) * 3;
                    const float rx = rows[a3 * RROW + s], ry = rows[(a3 + 1) * RROW + s], rz = rows[(a3 + 2) * RROW + s];
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
                        const int l = c0 + 4 * q + c;
                        const float dx = cx[c] - rx, dy = cy[c] - ry, dz = cz[c] - rz;
                        const float d = sqrtf((dx * dx + dy * dy) + dz * dz);
                        const bool pair = ok && k < p.m && l < p.m && l - k >= p.min_sep;
                        panel[(r2 * WIN + 4 * q + c) * PROW + s] = pair ? d : 0.f;
                    }
                }
                __syncthreads();
#pragma unroll
                for (int s4 = 0; s4 < KC / 4; ++s4) {
                    const float *pk = &panel[(s4 * 4 + lk) * PROW];
                    const double a = (double)pk[ti * 16 + lr];
#pragma unroll
                    for (int u = 0; u < TJ; ++u) {
                        if (!on[u]) continue;
                        const double b = (double)pk[BLK + (tj0 + u) * 16 + lr];
                        acc[u] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[u], 0, 0, 0);
                    }
                }
            }
        }
#pragma unroll
        for (int u = 0; u < TJ; ++u) tot[u] += acc[u];               // the slabs in ascending order, the first to +0
    }
    if (MODE == MODE_NORM) {
        // the diagonal of the diagonal wave tiles: row lk + 4 reg == column lr
        double *dst = p.gdst + (p.split ? (size_t)blockIdx.z * p.g_stride : 0);
#pragma unroll
        for (int u = 0; u < TJ; ++u)
            if (on[u] && lr >= lk && ((lr - lk) & 3) == 0) dst[I * BLK + ti * 16 + lr] = pick(tot[u], (lr - lk) >> 2);
    } else if (p.split) {
        const long long blk = MODE == MODE_ONE ? tri_block(I, J, gridDim.y) : (long long)I * gridDim.x + J;
        double *dst = p.part + ((size_t)blk * p.n_slabs + blockIdx.z) * PART;
#pragma unroll
        for (int u = 0; u < TJ; ++u)
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) dst[(u * 4 + reg) * MT + t] = pick(tot[u], reg);
    } else {
        tail<MODE>(p, I, J, tot);
    }
}

// split: G = the slabs' partial norms added to 0 in ascending order
__global__ __launch_bounds__(256) void norm_finish_kernel(const double *gpart, int n_pad, int n_slabs, double *g) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n_pad) return;
    double v = 0.0;
    for (int sl = 0; sl < n_slabs; ++sl) v += gpart[(size_t)sl * n_pad + i];
    g[i] = v;
}

// split: grid (column blocks, row blocks): the slabs' partial blocks added to 0 in ascending order, then the tail
template <int MODE> __global__ __launch_bounds__(MT) void finish_kernel(Prm p) {
    const int J = blockIdx.x, I = blockIdx.y;
    if (MODE == MODE_ONE && J < I) return;
    const long long blk = MODE == MODE_ONE ? tri_block(I, J, gridDim.y) : (long long)I * gridDim.x + J;
    const double *src = p.part + (size_t)blk * p.n_slabs * PART;
    double4_t tot[TJ];
#pragma unroll
    for (int u = 0; u < TJ; ++u) tot[u] = double4_t{0.0, 0.0, 0.0, 0.0};
    for (int sl = 0; sl < p.n_slabs; ++sl) {
        const double *ps = src + (size_t)sl * PART + threadIdx.x;
#pragma unroll
        for (int u = 0; u < TJ; ++u) tot[u] += double4_t{ps[(u * 4) * MT], ps[(u * 4 + 1) * MT], ps[(u * 4 + 2) * MT], ps[(u * 4 + 3) * MT]};
    }
    tail<MODE>(p, I, J, tot);
}

// ------------------------------------------------------------------------------------------------------------ pairs --
constexpr int PT = 256;

__device__ __forceinline__ float pair_dist(const float *xs, size_t ak, size_t al) {
    const float dx = xs[3 * al] - xs[3 * ak], dy = xs[3 * al + 1] - xs[3 * ak + 1], dz = xs[3 * al + 2] - xs[3 * ak + 2];
    return sqrtf((dx * dx + dy * dy) + dz * dz);
}

__global__ __launch_bounds__(PT) void pairs_kernel(const float *A, int na, const float *B, int nb, int n_atoms, const int32_t *sel,
                                                   int m, int min_sep, const int32_t *pairs, double P, double *msd, double *position) {
    __shared__ double red[PT / 64];
    const int ia = pairs[2 * (size_t)blockIdx.x], ib = pairs[2 * (size_t)blockIdx.x + 1];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double *pos = position ? position + (size_t)blockIdx.x * m : nullptr;
    const bool inside = (unsigned)ia < (unsigned)na && (unsigned)ib < (unsigned)nb;     // uniform
    const float *xa = A + (size_t)(inside ? ia : 0) * n_atoms * 3, *xb = B + (size_t)(inside ? ib : 0) * n_atoms * 3;
    int bad = inside ? 0 : 1;
    for (int k = threadIdx.x; k < m && inside; k += PT) {
        const size_t a = row_of(sel, k, n_atoms);
        bad |= non_finite(xa[3 * a]) | non_finite(xa[3 * a + 1]) | non_finite(xa[3 * a + 2]);
        bad |= non_finite(xb[3 * a]) | non_finite(xb[3 * a + 1]) | non_finite(xb[3 * a + 2]);
    }
    bad = __syncthreads_or(bad);
    if (bad) {
        if (threadIdx.x == 0) msd[blockIdx.x] = nan64();
        if (pos)
            for (int k = threadIdx.x; k < m; k += PT) pos[k] = nan64();
        return;
    }
    double tot = 0.0;
    for (int k = wave; k < m; k += PT / 64) {                        // uniform in the wave
        const size_t ak = row_of(sel, k, n_atoms);
        double row = 0.0;
        for (int l = lane; l < m; l += 64) {
            if (abs(l - k) < min_sep) continue;
            const size_t al = row_of(sel, l, n_atoms);
            const double diff = (double)pair_dist(xa, ak, al) - (double)pair_dist(xb, ak, al);
            row += diff * diff;
        }
        row = wave_sum(row);
        tot += row;
        if (pos && lane == 0) pos[k] = row / (double)(max(0, k - min_sep + 1) + max(0, m - k - min_sep));
    }
    if (lane == 0) red[wave] = tot;
    __syncthreads();
    if (threadIdx.x == 0) msd[blockIdx.x] = ((((red[0] + red[1]) + red[2]) + red[3]) * 0.5) / P;
}

// --------------------------------------------------------------------------------------------------------------- host --
struct Plan {
    int m, T, n_tiles, n_slabs, nbi, nbj, groups;
    long long blocks, pa, pb;                // blocks of the call; the pools' structures padded to whole blocks
    double P;
};

// cross = Nb > 0.  The split rule: a function of the blocks of the call and of (m, min_sep)'s slabs alone.
Plan plan_of(int Na, int Nb, int m, int min_sep) {
    Plan pl;
    pl.m = m;
    pl.T = (m + WIN - 1) / WIN;
    pl.n_tiles = pl.T * (pl.T + 1) / 2;
    pl.n_slabs = (pl.n_tiles + SLAB - 1) / SLAB;
    pl.nbi = (Na + BLK - 1) / BLK;
    pl.nbj = Nb > 0 ? (Nb + BLK - 1) / BLK : pl.nbi;
    pl.blocks = Nb > 0 ? (long long)pl.nbi * pl.nbj : (long long)pl.nbi * (pl.nbi + 1) / 2;
    pl.pa = (long long)pl.nbi * BLK, pl.pb = Nb > 0 ? (long long)pl.nbj * BLK : 0;
    const long long n = (long long)m - min_sep;
    pl.P = (double)(n * (n + 1) / 2);
    const bool split = pl.n_slabs > 1 && pl.blocks < CODLAD_DRMSD_SPLIT_MAX_BLOCKS &&
                       pl.blocks * pl.n_slabs * PART * 8ll <= (long long)CODLAD_DRMSD_SCRATCH_BUDGET;
    pl.groups = split ? pl.n_slabs : 1;
    return pl;
}

// scratch: G of x, G of y, then with the split the partial norms [slab][pa + pb] and the partial blocks
struct Layout {
    size_t gx, gy, gpart, part, bytes;
};
Layout layout_of(const Plan &pl) {
    Layout l;
    l.gx = 0;
    l.gy = l.gx + align256(8 * (size_t)pl.pa);
    l.gpart = l.gy + align256(8 * (size_t)pl.pb);
    l.part = l.gpart + (pl.groups > 1 ? align256(8 * (size_t)pl.n_slabs * (pl.pa + pl.pb)) : 0);
    l.bytes = l.part + (pl.groups > 1 ? 8 * (size_t)pl.blocks * pl.n_slabs * PART : 0);
    return l;
}

#define DRMSD_SIZES(Na, Nb, n_sel, min_sep)                                                                          \
    CODLAD_REQUIRE(Na > 0 && Nb >= 0 && (Nb > 0 || Na <= MAX_N), "bad sizes (Na >= 1, Nb >= 0; one pool: Na <= CODLAD_CLUSTER_MAX_N)"); \
    CODLAD_REQUIRE(n_sel >= 2 && n_sel <= MAX_SEL, "m outside 2 .. CODLAD_DRMSD_MAX_SEL");                          \
    CODLAD_REQUIRE(min_sep >= 1 && min_sep < n_sel, "min_sep outside 1 .. m - 1")
}  // namespace

extern "C" int codlad_drmsd_groups(int Na, int Nb, int n_sel, int min_sep) {
    DRMSD_SIZES(Na, Nb, n_sel, min_sep);
    return plan_of(Na, Nb, n_sel, min_sep).groups;
}

extern "C" long long codlad_drmsd_matrix_scratch_bytes(int Na, int Nb, int n_sel, int min_sep) {
    DRMSD_SIZES(Na, Nb, n_sel, min_sep);
    return (long long)layout_of(plan_of(Na, Nb, n_sel, min_sep)).bytes;
}

extern "C" int codlad_drmsd_matrix(const float *x, int Na, const float *y, int Nb, int n_atoms, const int32_t *sel, int n_sel,
                                   int min_sep, double cut2, int squared, double *msd, uint64_t *bits, uint8_t *finite_x,
                                   uint8_t *finite_y, void *scratch, void *stream) {
    CODLAD_REQUIRE(x && finite_x && scratch, "null pointer");
    CODLAD_REQUIRE((y != nullptr) == (Nb > 0) && (y != nullptr) == (finite_y != nullptr), "y, Nb and finite_y disagree (all three for cross mode, or none)");
    CODLAD_REQUIRE(n_atoms > 0 && n_sel >= 0, "bad counts");
    const int m = subset_size(sel, n_sel, n_atoms);
    CODLAD_REQUIRE(m > 0, "sel and n_sel disagree (sel with n_sel > 0, or neither)");
    DRMSD_SIZES(Na, Nb, m, min_sep);
    const bool cross = y != nullptr;
    CODLAD_REQUIRE(msd || bits, "neither msd nor bits is asked for");
    CODLAD_REQUIRE(!(cross && bits), "no bitmap in cross mode");
    CODLAD_REQUIRE(!bits || (cut2 >= 0.0 && cut2 < __builtin_inf()), "cut2 is not a finite number >= 0");
    const char *what = "codlad_drmsd_matrix";
    const Plan pl = plan_of(Na, Nb, m, min_sep);
    const Layout lay = layout_of(pl);
    CODLAD_REQUIRE(pl.nbi <= 65535 && pl.nbj <= 65535 && pl.groups <= 65535, "too many blocks for one call");
    hipStream_t st = (hipStream_t)stream;
    char *base = (char *)scratch;
    double *gx = (double *)(base + lay.gx), *gy = cross ? (double *)(base + lay.gy) : gx;
    double *gpart = (double *)(base + lay.gpart);
    const bool split = pl.groups > 1;
    const int g_stride = (int)(pl.pa + pl.pb);

    hipLaunchKernelGGL(finite_kernel, dim3((unsigned)((Na + 3) / 4)), dim3(256), 0, st, x, Na, n_atoms, sel, m, finite_x);
    if (cross) hipLaunchKernelGGL(finite_kernel, dim3((unsigned)((Nb + 3) / 4)), dim3(256), 0, st, y, Nb, n_atoms, sel, m, finite_y);
    int rc = codlad_check_launch(what);
    if (rc) return rc;

    Prm p;
    p.sel = sel, p.n_atoms = n_atoms, p.m = m, p.min_sep = min_sep, p.T = pl.T, p.n_tiles = pl.n_tiles, p.n_slabs = pl.n_slabs;
    p.split = split ? 1 : 0, p.squared = squared != 0, p.P = pl.P, p.cut2 = cut2, p.g_stride = g_stride;
    p.out = nullptr, p.bits = nullptr, p.part = (double *)(base + lay.part), p.gx = gx, p.gy = gy;
    // the norms: G of every pool, the diagonal blocks of its own product
    for (int pool = 0; pool < (cross ? 2 : 1); ++pool) {
        p.x = p.y = pool ? y : x, p.fx = p.fy = pool ? finite_y : finite_x, p.Na = p.Nb = pool ? Nb : Na;
        double *g = pool ? gy : gx;
        const int nb = pool ? pl.nbj : pl.nbi;
        p.gdst = split ? gpart + (pool ? pl.pa : 0) : g;
        hipLaunchKernelGGL(gram_kernel<MODE_NORM>, dim3(1, (unsigned)nb, (unsigned)pl.groups), dim3(MT), 0, st, p);
        if (split)
            hipLaunchKernelGGL(norm_finish_kernel, dim3((unsigned)((nb * BLK + 255) / 256)), dim3(256), 0, st, p.gdst, g_stride, pl.n_slabs, g);
    }
    rc = codlad_check_launch(what);
    if (rc) return rc;
    p.x = x, p.y = cross ? y : x, p.fx = finite_x, p.fy = cross ? finite_y : finite_x, p.Na = Na, p.Nb = cross ? Nb : Na;
    p.W = (Na + 63) / 64, p.out = msd, p.bits = (unsigned long long *)bits, p.gdst = nullptr;
    const dim3 grid((unsigned)pl.nbj, (unsigned)pl.nbi, (unsigned)pl.groups), flat((unsigned)pl.nbj, (unsigned)pl.nbi);
    if (cross) {
        hipLaunchKernelGGL(gram_kernel<MODE_CROSS>, grid, dim3(MT), 0, st, p);
        if (split) hipLaunchKernelGGL(finish_kernel<MODE_CROSS>, flat, dim3(MT), 0, st, p);
    } else {
        hipLaunchKernelGGL(gram_kernel<MODE_ONE>, grid, dim3(MT), 0, st, p);
        if (split) hipLaunchKernelGGL(finish_kernel<MODE_ONE>, flat, dim3(MT), 0, st, p);
    }
    return codlad_check_launch(what);
}

extern "C" int codlad_drmsd_pairs(const float *a, int na, const float *b, int nb, int n_atoms, const int32_t *sel, int n_sel,
                                  int min_sep, const int32_t *pairs, int K, double *msd, double *position, void *stream) {
    CODLAD_REQUIRE(a && b && pairs && msd, "null pointer");
    CODLAD_REQUIRE(na > 0 && nb > 0 && n_atoms > 0 && n_sel >= 0 && K > 0, "bad counts");
    const int m = subset_size(sel, n_sel, n_atoms);
    CODLAD_REQUIRE(m > 0, "sel and n_sel disagree (sel with n_sel > 0, or neither)");
    CODLAD_REQUIRE(m >= 2 && m <= MAX_SEL, "m outside 2 .. CODLAD_DRMSD_MAX_SEL");
    CODLAD_REQUIRE(min_sep >= 1 && min_sep < m, "min_sep outside 1 .. m - 1");
    const long long n = (long long)m - min_sep;
    hipLaunchKernelGGL(pairs_kernel, dim3((unsigned)K), dim3(PT), 0, (hipStream_t)stream, a, na, b, nb, n_atoms, sel, m, min_sep,
                       pairs, (double)(n * (n + 1) / 2), msd, position);
    return codlad_check_launch("codlad_drmsd_pairs");
}
