// Torsion-space analysis of an ensemble (include/codlad_hip.h, codlad_torsion_*): every structure as the unit vectors
// f_t = (cos theta_t, sin theta_t) of its T torsions - the periodicity-free representation of dihedral PCA - and what is
// made of that table: the weighted resultant, the deviations from it, the torsion distance of every pair of a pool or of
// two pools, and of a list of pairs.  The arithmetic is stated in the header; here is how it is laid out.
// (every kernel's name starts with torsion_: the unit shares the library with other units' gram and pairs kernels)
//   features_kernel   a workgroup per structure, thread l the torsions l, l + 256, ..: the float64 sequence of the header
//                     (+ - * / sqrt only), kept in registers until the workgroup knows whether the structure is finite;
//                     then the row or NaN.  One writer per element.
//   weight_kernel     a wave per chunk of structures: W's partial, lane l the structures l, l + 64, .. of the chunk, the
//                     xor butterfly
//   mean_kernel       thread e of chunk ch adds w_s F_se over the structures of the chunk in ascending order by fused
//                     multiply-adds (pca_mean_kernel's rule, reduce_math.h's chunks_of)
//   finish_kernel     the chunks in ascending order, one division
//   dev_kernel        D = F - mean, NaN rows for structures that are not finite
//   gram_kernel       the hot path: tmsd_ij = max(G_i + G_j - 2 C_ij, 0) / T, C = F F^T, on v_mfma_f64_16x16x4_f64.
//                     Workgroup (J, I) of 8 waves owns the 64 x 64 structure pairs of the blocks I and J (one pool: J >= I
//                     only); wave (ti, tj0) owns two 16 x 16 tiles.  The two 64-row panels of F come through LDS in
//                     chunks of KC = 32 features - a panel row of a chunk is 256 B, two whole cache lines, fetched as 16
//                     double2 by 16 consecutive lanes - the next chunk's global loads in flight under the current MFMAs
//                     (pca_cov_kernel's scheme).  A panel row is PROW = KC + 2 = 34 doubles: the operand read of a half
//                     wave (lane l: row l & 15, k = l >> 4, so rows 0 .. 15 at two consecutive k) is at the doubles 34 row
//                     + k = 2 (17 row) + k, and 17 is odd, so 17 row mod 16 takes all 16 values and the 32 lanes fall on
//                     32 different double-banks (address in doubles mod 32) - no conflict in either of ds_read_b64's two
//                     groups of 32 lanes.  A row of a structure that is not finite or not there, and every column
//                     past 2 T, is staged as zeros.  NORM: blocks (I, I), the diagonal wave tiles only, the diagonal of
//                     the product -> G, BY THE SAME SEQUENCE: one accumulator per element, the K steps in ascending
//                     order from +0, so C_ij of two structures with equal features is G_i = G_j to the bit.
//   tail              drmsd_kernels.hip's: per lane the pairs (row lk + 4 reg of tile ti, column lr of tile tj), the
//                     element and its mirror from one value, the decision through __ballot into 16-bit segments, one
//                     writer per 64-bit word.
//   pairs_kernel      a wave per pair of the list: the direct sum, lane l the torsions l, l + 64, .., the butterfly.
// No atomics, no scratch memory, no spills.  As built for gfx950 (kernel-resource-usage): gram_kernel 64 / 81 / 74 VGPRs
// (norm, one pool, two pools), no AGPRs, 35 KiB of LDS (34 KiB panels, 1 KiB bitmap segments): 8 / 5 / 6 waves per SIMD by
// registers - two workgroups a compute unit in one-pool mode, where the LDS would allow four; features_kernel 69 VGPRs,
// pairs_kernel 22, the mean's four kernels 6 - 16.
#include "common.h"
#include "host_util.h"
#include "reduce_math.h"
#include "structure_math.h"

namespace {
constexpr int MAX_N = CODLAD_CLUSTER_MAX_N, MAX_T = CODLAD_TORSION_MAX_T;
static_assert(2 * MAX_T <= CODLAD_PCA_MAX_DIM, "the feature table is a deviation table of codlad_feature_covariance");

// ---------------------------------------------------------------------------------------------------------- features --
constexpr int FT = 256, FE = MAX_T / FT;    // threads of a structure's workgroup, torsions of a thread
static_assert(FE * FT == MAX_T, "a thread's torsions cover the largest table");

struct D3 {
    double x, y, z;
};
__device__ __forceinline__ D3 dsub(const D3 &a, const D3 &b) { return D3{a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ D3 dcross(const D3 &a, const D3 &b) {
    return D3{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x};
}
__device__ __forceinline__ double ddot(const D3 &a, const D3 &b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }

// the atom's coordinates, converted exactly; bad collects a NaN or an infinity
__device__ __forceinline__ D3 atom64(const float *xs, int a, int n_atoms, int &bad) {
    const size_t r = 3 * (size_t)clampi(a, 0, n_atoms - 1);
    const float u = xs[r], v = xs[r + 1], w = xs[r + 2];
    bad |= non_finite(u) | non_finite(v) | non_finite(w);
    return D3{(double)u, (double)v, (double)w};
}

__global__ __launch_bounds__(FT) void torsion_features_kernel(const float *x, int n_atoms, const int32_t *quads, int T, double *F,
                                                      uint8_t *finite) {
    const int s = blockIdx.x;
    const float *xs = x + (size_t)s * n_atoms * 3;
    double c[FE], sn[FE];
    int bad = 0;
#pragma unroll
    for (int e = 0; e < FE; ++e) {
        const int t = threadIdx.x + FT * e;
        c[e] = sn[e] = 0.0;
        if (t >= T) continue;
        const int32_t *q = quads + 4 * (size_t)t;
        const D3 p0 = atom64(xs, q[0], n_atoms, bad), p1 = atom64(xs, q[1], n_atoms, bad);
        const D3 p2 = atom64(xs, q[2], n_atoms, bad), p3 = atom64(xs, q[3], n_atoms, bad);
        const D3 b1 = dsub(p1, p0), b2 = dsub(p2, p1), b3 = dsub(p3, p2);
        const D3 n1 = dcross(b1, b2), n2 = dcross(b2, b3);
        const double xx = ddot(n1, n2);
        const double yy = sqrt(ddot(b2, b2)) * ddot(b1, n2);
        const double h = sqrt(xx * xx + yy * yy);
        bad |= !(h > 0.0);                             // collinear atoms: no angle (a NaN from infinities is caught above)
        c[e] = xx / h, sn[e] = yy / h;
    }
    bad = __syncthreads_or(bad);
    if (threadIdx.x == 0) finite[s] = bad ? 0 : 1;
    double *row = F + (size_t)s * 2 * T;
#pragma unroll
    for (int e = 0; e < FE; ++e) {
        const int t = threadIdx.x + FT * e;
        if (t >= T) continue;
        row[2 * t] = bad ? nan64() : c[e];
        row[2 * t + 1] = bad ? nan64() : sn[e];
    }
}

// ------------------------------------------------------------------------------------------------------------- mean --
__device__ __forceinline__ double weight_of(const uint8_t *finite, const double *w, int s) {
    if (!finite[s]) return 0.0;
    const double ws = w ? w[s] : 1.0;
    return ws > 0.0 ? ws : 0.0;
}

// grid nch, a wave each: wpart[ch] = the weights of the chunk's structures, lane l the structures l, l + 64, .. in
// ascending order, the butterfly
__global__ __launch_bounds__(64) void torsion_weight_kernel(const uint8_t *finite, const double *w, int N, int chunk, double *wpart) {
    const int s0 = blockIdx.x * chunk, s1 = min(N, s0 + chunk);
    double acc = 0.0;
    for (int s = s0 + (int)threadIdx.x; s < s1; s += 64) acc += weight_of(finite, w, s);
    acc = wave_sum(acc);
    if (threadIdx.x == 0) wpart[blockIdx.x] = acc;
}

// grid (ceil(K / 256), nch): part[ch][e] = the sum of w_s F_se over the chunk, ascending
__global__ __launch_bounds__(256) void torsion_mean_kernel(const double *F, const uint8_t *finite, const double *w, int N, int K, int chunk,
                                                   double *part) {
    const int e = blockIdx.x * 256 + threadIdx.x, ch = blockIdx.y;
    if (e >= K) return;
    const int s0 = ch * chunk, s1 = min(N, s0 + chunk);
    double acc = 0.0;
    for (int s = s0; s < s1; ++s) {
        const double ws = weight_of(finite, w, s);     // uniform
        if (!(ws > 0.0)) continue;
        acc = fma(ws, F[(size_t)s * K + e], acc);
    }
    part[(size_t)ch * K + e] = acc;
}

__global__ __launch_bounds__(256) void torsion_finish_kernel(const double *part, const double *wpart, int K, int nch, double *mean, double *scal) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    double W = 0.0;
    for (int ch = 0; ch < nch; ++ch) W += wpart[ch];
    if (e == 0) {
        scal[CODLAD_PCA_SC_W] = W;
        for (int k = 1; k < CODLAD_PCA_SCALARS; ++k) scal[k] = nan64();
    }
    if (e >= K) return;
    double v = 0.0;
    for (int ch = 0; ch < nch; ++ch) v += part[(size_t)ch * K + e];
    mean[e] = v / W;                                   // no structure of positive weight: 0 / 0, NaN
}

// grid (N, ceil(K / 256))
__global__ __launch_bounds__(256) void torsion_dev_kernel(const double *F, const uint8_t *finite, const double *mean, int K, double *D) {
    const int e = blockIdx.y * 256 + threadIdx.x, s = blockIdx.x;
    if (e >= K) return;
    D[(size_t)s * K + e] = finite[s] ? F[(size_t)s * K + e] - mean[e] : nan64();
}

// ----------------------------------------------------------------------------------------------------------- matrix --
constexpr int BLK = 64;                     // structures of a block = bits of a word
constexpr int NW = 8, TJ = 2;               // waves of a workgroup, wave tiles of a wave
constexpr int MT = NW * 64;
constexpr int KC = 32;                      // features of a staged chunk: 8 MFMA steps
constexpr int PROW = KC + 2;                // doubles of a panel row: PROW / 2 odd, see the head of the file
constexpr int LOADS = 2 * BLK * (KC / 2) / MT;      // double2 per thread and chunk
static_assert(2 * BLK * (KC / 2) % MT == 0 && (PROW / 2) % 2 == 1 && PROW % 2 == 0, "the chunk is spread evenly; the stride");

enum { MODE_NORM = 0, MODE_ONE = 1, MODE_CROSS = 2 };

struct TorsionPrm {
    const double *fx, *fy;                  // the table of the row blocks and of the column blocks (one pool: the same)
    const uint8_t *okx, *oky;
    const double *gx, *gy;
    int Na, Nb, K, squared, W;
    double T, cut2;
    double *out;
    unsigned long long *bits;
    double *gdst;                           // NORM: G [N_pad]
};

__device__ __forceinline__ double pick(const double4_t &v, int reg) { return reg == 0 ? v.x : reg == 1 ? v.y : reg == 2 ? v.z : v.w; }

// The pairs (row lk + 4 reg of wave tile ti, column lr of wave tile tj0 + u) of this lane from their C.
template <int MODE> __device__ __forceinline__ void tail(const TorsionPrm &p, int I, int J, const double4_t (&c)[TJ]) {
    __shared__ unsigned short rowseg[BLK][4], colseg[BLK][4];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int ti = wave / (4 / TJ), tj0 = (wave % (4 / TJ)) * TJ;
    const int lr = lane & 15, lk = lane >> 4;
#pragma unroll
    for (int u = 0; u < TJ; ++u) {
        const int tj = tj0 + u, gj = J * BLK + tj * 16 + lr;
        const bool on = MODE == MODE_CROSS || I != J || tj >= ti;    // uniform in the wave
        const bool in_j = gj < p.Nb;
        const bool fj = in_j && p.oky[gj] != 0;
        const double Gj = in_j ? p.gy[gj] : 0.0;
        unsigned colbits = 0;
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            const int gi = I * BLK + ti * 16 + lk + 4 * reg;
            const bool valid = on && gi < p.Na && in_j;
            const bool upper = MODE == MODE_CROSS || gi < gj, diag = MODE != MODE_CROSS && gi == gj;
            const bool fin = valid && fj && p.okx[gi] != 0;
            double msd = nan64();
            if (fin && upper) {
                const double v = (p.gx[gi] + Gj) - 2.0 * pick(c[u], reg);
                msd = (v < 0.0 ? 0.0 : v) / p.T;
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

// double2 l of this thread of the chunk at k0: row r of the 128 (block I's 64, then block J's), features k0 + 2 c2, + 1
__device__ __forceinline__ double2 panel_load(const TorsionPrm &p, int I, int J, int k0, int e) {
    const int r = e / (KC / 2), c2 = e % (KC / 2), k = k0 + 2 * c2;
    const bool sec = r >= BLK;
    const int np = sec ? p.Nb : p.Na, g = (sec ? J : I) * BLK + (r & (BLK - 1));
    if (g >= np || k >= p.K || !(sec ? p.oky : p.okx)[g]) return make_double2(0.0, 0.0);      // K is even: the pair is in or out
    return *reinterpret_cast<const double2 *>((sec ? p.fy : p.fx) + (size_t)g * p.K + k);
}

// grid (column blocks, row blocks); NORM: (1, blocks)
template <int MODE> __global__ __launch_bounds__(MT) void torsion_gram_kernel(TorsionPrm p) {
    const int J = MODE == MODE_NORM ? blockIdx.y : blockIdx.x, I = blockIdx.y;
    if (MODE == MODE_ONE && J < I) return;
    __shared__ __attribute__((aligned(16))) double panel[2 * BLK * PROW];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int ti = wave / (4 / TJ), tj0 = (wave % (4 / TJ)) * TJ;
    const int lr = lane & 15, lk = lane >> 4;
    bool on[TJ];
#pragma unroll
    for (int u = 0; u < TJ; ++u)                                     // uniform in the wave
        on[u] = MODE == MODE_NORM ? tj0 + u == ti : MODE == MODE_CROSS || I != J || tj0 + u >= ti;
    double4_t acc[TJ];
#pragma unroll
    for (int u = 0; u < TJ; ++u) acc[u] = double4_t{0.0, 0.0, 0.0, 0.0};
    double2 stage[LOADS];
#pragma unroll
    for (int l = 0; l < LOADS; ++l) stage[l] = panel_load(p, I, J, 0, t + l * MT);
    for (int k0 = 0; k0 < p.K; k0 += KC) {
        __syncthreads();                                             // the previous chunk has been read
#pragma unroll
        for (int l = 0; l < LOADS; ++l) {
            const int e = t + l * MT;
            *reinterpret_cast<double2 *>(&panel[(e / (KC / 2)) * PROW + 2 * (e % (KC / 2))]) = stage[l];
        }
        __syncthreads();
        if (k0 + KC < p.K)
#pragma unroll
            for (int l = 0; l < LOADS; ++l) stage[l] = panel_load(p, I, J, k0 + KC, t + l * MT);
#pragma unroll
        for (int s4 = 0; s4 < KC / 4; ++s4) {
            const double a = panel[(ti * 16 + lr) * PROW + s4 * 4 + lk];
#pragma unroll
            for (int u = 0; u < TJ; ++u) {
                if (!on[u]) continue;
                const double b = panel[(BLK + (tj0 + u) * 16 + lr) * PROW + s4 * 4 + lk];
                acc[u] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[u], 0, 0, 0);
            }
        }
    }
    if (MODE == MODE_NORM) {
        // the diagonal of the diagonal wave tiles: row lk + 4 reg == column lr
#pragma unroll
        for (int u = 0; u < TJ; ++u)
            if (on[u] && lr >= lk && ((lr - lk) & 3) == 0) p.gdst[I * BLK + ti * 16 + lr] = pick(acc[u], (lr - lk) >> 2);
    } else {
        tail<MODE>(p, I, J, acc);
    }
}

// ------------------------------------------------------------------------------------------------------------ pairs --
constexpr int PT = 256;
// a wave per pair
__global__ __launch_bounds__(PT) void torsion_pairs_kernel(const double *Fa, int na, const double *Fb, int nb, int T, const int32_t *pairs,
                                                   int n_pairs, double *tmsd, double *terms) {
    const int k = blockIdx.x * (PT / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (k >= n_pairs) return;                                        // uniform in the wave
    const int ia = pairs[2 * (size_t)k], ib = pairs[2 * (size_t)k + 1];
    const bool inside = (unsigned)ia < (unsigned)na && (unsigned)ib < (unsigned)nb;     // uniform
    const double *fa = Fa + (size_t)(inside ? ia : 0) * 2 * T, *fb = Fb + (size_t)(inside ? ib : 0) * 2 * T;
    double acc = 0.0;
    for (int t = lane; t < T; t += 64) {
        const double dc = fa[2 * t] - fb[2 * t], ds = fa[2 * t + 1] - fb[2 * t + 1];
        const double term = inside ? dc * dc + ds * ds : nan64();    // the NaN row of a structure that is not finite stays NaN
        acc += term;
        if (terms) terms[(size_t)k * T + t] = term;
    }
    acc = wave_sum(acc);
    if (lane == 0) tmsd[k] = acc / (double)T;
}

#define TORSION_SIZES(N, T)                                                                                          \
    CODLAD_REQUIRE(N > 0 && N <= MAX_N && T >= 1 && T <= MAX_T, "bad sizes (1 <= N <= CODLAD_CLUSTER_MAX_N, 1 <= T <= CODLAD_TORSION_MAX_T)")
}  // namespace

extern "C" int codlad_torsion_features(const float *x, int N, int n_atoms, const int32_t *quads, int T, double *F, uint8_t *finite,
                                       void *stream) {
    CODLAD_REQUIRE(x && quads && F && finite, "null pointer");
    CODLAD_REQUIRE(n_atoms > 0, "bad counts");
    TORSION_SIZES(N, T);
    hipLaunchKernelGGL(torsion_features_kernel, dim3((unsigned)N), dim3(FT), 0, (hipStream_t)stream, x, n_atoms, quads, T, F, finite);
    return codlad_check_launch("codlad_torsion_features");
}

extern "C" long long codlad_torsion_mean_scratch_bytes(int N, int T) {
    TORSION_SIZES(N, T);
    const Chunks c = chunks_of(N);
    return 8ll * c.nch * (2ll * T + 1);
}

extern "C" int codlad_torsion_mean(const double *F, const uint8_t *finite, const double *w, int N, int T, double *mean, double *scal,
                                   double *D, void *scratch, void *stream) {
    CODLAD_REQUIRE(F && finite && mean && scal && scratch, "null pointer");
    TORSION_SIZES(N, T);
    const Chunks c = chunks_of(N);
    const int K = 2 * T;
    double *wpart = (double *)scratch, *part = wpart + c.nch;
    hipStream_t st = (hipStream_t)stream;
    const unsigned bx = (unsigned)((K + 255) / 256);
    hipLaunchKernelGGL(torsion_weight_kernel, dim3((unsigned)c.nch), dim3(64), 0, st, finite, w, N, c.chunk, wpart);
    hipLaunchKernelGGL(torsion_mean_kernel, dim3(bx, (unsigned)c.nch), dim3(256), 0, st, F, finite, w, N, K, c.chunk, part);
    hipLaunchKernelGGL(torsion_finish_kernel, dim3(bx), dim3(256), 0, st, (const double *)part, (const double *)wpart, K, c.nch, mean, scal);
    if (D) hipLaunchKernelGGL(torsion_dev_kernel, dim3((unsigned)N, bx), dim3(256), 0, st, F, finite, (const double *)mean, K, D);
    return codlad_check_launch("codlad_torsion_mean");
}

extern "C" long long codlad_torsion_matrix_scratch_bytes(int Na, int Nb) {
    CODLAD_REQUIRE(Na > 0 && Na <= MAX_N && Nb >= 0 && Nb <= MAX_N, "bad sizes (1 <= Na, 0 <= Nb, both <= CODLAD_CLUSTER_MAX_N)");
    return 8ll * BLK * ((Na + BLK - 1) / BLK + (Nb + BLK - 1) / BLK);
}

extern "C" int codlad_torsion_matrix(const double *Fx, const uint8_t *finite_x, int Na, const double *Fy, const uint8_t *finite_y,
                                     int Nb, int T, double cut2, int squared, double *tmsd, uint64_t *bits, void *scratch,
                                     void *stream) {
    CODLAD_REQUIRE(Fx && finite_x && scratch, "null pointer");
    CODLAD_REQUIRE((Fy != nullptr) == (Nb > 0) && (Fy != nullptr) == (finite_y != nullptr),
                   "Fy, Nb and finite_y disagree (all three for two pools, or none)");
    CODLAD_REQUIRE(Na > 0 && Na <= MAX_N && Nb >= 0 && Nb <= MAX_N && T >= 1 && T <= MAX_T,
                   "bad sizes (1 <= Na, 0 <= Nb, both <= CODLAD_CLUSTER_MAX_N, 1 <= T <= CODLAD_TORSION_MAX_T)");
    const bool cross = Fy != nullptr;
    CODLAD_REQUIRE(tmsd || bits, "neither tmsd nor bits is asked for");
    CODLAD_REQUIRE(!(cross && bits), "no bitmap with two pools");
    CODLAD_REQUIRE(!bits || (cut2 >= 0.0 && cut2 < __builtin_inf()), "cut2 is not a finite number >= 0");
    const char *what = "codlad_torsion_matrix";
    const int nbi = (Na + BLK - 1) / BLK, nbj = cross ? (Nb + BLK - 1) / BLK : nbi;
    hipStream_t st = (hipStream_t)stream;
    double *gx = (double *)scratch, *gy = cross ? gx + (size_t)nbi * BLK : gx;
    TorsionPrm p;
    p.K = 2 * T, p.T = (double)T, p.squared = squared != 0, p.cut2 = cut2, p.out = nullptr, p.bits = nullptr, p.gx = gx, p.gy = gy, p.W = 0;
    // the norms: G of every pool, the diagonal blocks of its own product
    for (int pool = 0; pool < (cross ? 2 : 1); ++pool) {
        p.fx = p.fy = pool ? Fy : Fx, p.okx = p.oky = pool ? finite_y : finite_x, p.Na = p.Nb = pool ? Nb : Na;
        p.gdst = pool ? gy : gx;
        hipLaunchKernelGGL(torsion_gram_kernel<MODE_NORM>, dim3(1, (unsigned)(pool ? nbj : nbi)), dim3(MT), 0, st, p);
    }
    int rc = codlad_check_launch(what);
    if (rc) return rc;
    p.fx = Fx, p.fy = cross ? Fy : Fx, p.okx = finite_x, p.oky = cross ? finite_y : finite_x, p.Na = Na, p.Nb = cross ? Nb : Na;
    p.W = (Na + 63) / 64, p.out = tmsd, p.bits = (unsigned long long *)bits, p.gdst = nullptr;
    const dim3 grid((unsigned)nbj, (unsigned)nbi);
    if (cross) hipLaunchKernelGGL(torsion_gram_kernel<MODE_CROSS>, grid, dim3(MT), 0, st, p);
    else hipLaunchKernelGGL(torsion_gram_kernel<MODE_ONE>, grid, dim3(MT), 0, st, p);
    return codlad_check_launch(what);
}

extern "C" int codlad_torsion_pairs(const double *Fa, int na, const double *Fb, int nb, int T, const int32_t *pairs, int K,
                                    double *tmsd, double *terms, void *stream) {
    CODLAD_REQUIRE(Fa && Fb && pairs && tmsd, "null pointer");
    CODLAD_REQUIRE(na > 0 && nb > 0 && K > 0 && T >= 1 && T <= MAX_T, "bad counts (na, nb, K >= 1, 1 <= T <= CODLAD_TORSION_MAX_T)");
    hipLaunchKernelGGL(torsion_pairs_kernel, dim3((unsigned)((K + PT / 64 - 1) / (PT / 64))), dim3(PT), 0, (hipStream_t)stream, Fa, na, Fb, nb, T,
                       pairs, K, tmsd, terms);
    return codlad_check_launch("codlad_torsion_pairs");
}
