// Essential dynamics of an ensemble (include/codlad_hip.h, codlad_pca_*): the mean structure after mutual superposition
// (generalised Procrustes), the deviations from it and their RMSF, the covariance of the aligned coordinates, its largest
// eigenpairs and the projections onto them.  The arithmetic is stated in the header; here is how it is laid out.
//
// The fit.  A pool of N structures is superposed on a float64 target M [m][3] over and over:
//   align_kernel    a workgroup per structure: the nine sums of S = sum (x - c)(M - cM)^T over the selected atoms, lane l
//                   of 256 adding atoms l, l + 256, .., the lanes by the tree of ensemble_kernels.hip, then the Horn tail of
//                   ensemble_math.h in one lane -> Rt.  The target is float64 and is never rounded to fp32.
//   mean_kernel     thread k of chunk ch adds w_s A_sk over the structures of the chunk in ascending order by fused
//                   multiply-adds, A_sk = R_s x_sk + t_s rounded as codlad_ens_apply rounds it
//   step_kernel     one workgroup: the chunks in ascending order, / W, the step against the target, the decision, and - only
//                   when the iteration goes on - the new target and its moments
// state[PCA_ST_PHASE] turns every launch of a finished problem into an immediate return (cluster_kernels.hip's discipline):
// the host enqueues batches of iterations and reads one word per batch.
//
// The covariance, the hot path: C = D^T diag(w) D / W as one float64 matrix product on v_mfma_f64_16x16x4_f64.  D [N][d]
// as it is stored - the structure is the contraction index, the coordinate is fastest - is the operand layout: an MFMA
// operand (row lane & 15, k lane >> 4) is 16 consecutive doubles of a row of D.
//   cov_kernel      workgroup (tile, chunk): a 64 x 64 tile (I, J), I >= J, of the lower triangle over one chunk of
//                   structures.  4 waves; wave ti owns rows 16 ti .. + 15 of the tile and its four 16 x 16 column tiles.
//                   The structures come in ascending order through LDS in steps of 16 (4 MFMAs of 4 structures), the next
//                   step's global loads in flight under the current MFMAs.  The weight multiplies the COLUMN operand (block
//                   J) when it is staged; a structure of weight 0 or that is not finite is staged as zeros in both.
//                   A row of a panel is 64 + 16 doubles, so the four k of an operand start on other banks.
//   cov_reduce_kernel  the chunks of an element in ascending order, / W, the element and its mirror from the one value
//   corr_kernel     the per-atom cross-correlation and the trace
//   trace_kernel    the trace alone, for codlad_feature_covariance: cov_kernel and cov_reduce_kernel on a table of any
//                   dimension d (torsion features; the 3 x 3 blocks of corr_kernel are what asks d % 3 == 0)
// The structures are cut into at most 32 chunks whose size depends on N alone (reduce_math.h's chunks_of).  No atomics, no scratch memory.
//
// The eigenpairs: blocked subspace iteration with a Rayleigh-Ritz step on b = min(k + 8, d) <= 72 columns, every block
// stored column by column ([b][d], the layout of `components`):
//   orth_kernel     one workgroup: Gram-Schmidt applied twice per column, the rule for a column that vanishes in the header
//   cq_kernel       Z = C Q, thread (row, 8 columns), ascending contraction by fused multiply-adds; C is symmetric to the
//                   bit, so the thread reads column `row` of C as a row: coalesced
//   h_kernel        H = Q^T Z, lower triangle, mirrored
//   jacobi_kernel   one workgroup: cyclic Jacobi in the round-robin order (b / 2 disjoint rotations at a time), eigenvalues
//                   sorted in descending order
//   rot_kernel      V = Q S, Y = Z S (= C V), |Y_i - theta_i V_i|, the sign of the largest entry
//   status_kernel   the stop rule; on the last iteration the results
// All sums have one order: ascending index per thread, the xor butterfly per wave (strides 32 .. 1), the waves in ascending
// order (reduce_math.h).  Compiled with -ffp-contract=off; fused multiply-adds are asked for by name.
#include "common.h"
#include "ensemble_math.h"
#include "host_util.h"
#include "reduce_math.h"

namespace {
constexpr int MAX_N = CODLAD_PCA_MAX_N, MAX_D = CODLAD_PCA_MAX_DIM, MAX_K = CODLAD_PCA_MAX_COMPONENTS;
constexpr int MAX_B = MAX_K + 8;            // columns of the iterated block
constexpr int BLOCK = 256;
enum { PH_NEW = 0, PH_RUNNING = 1, PH_DONE = 2 };

// ------------------------------------------------------------------------------------------------------------ the fit --
struct Fit {
    const float *x;
    const double *mom, *w;
    const int32_t *sel;
    int N, n_atoms, m, start, max_iter, nch, chunk;
    double tol;
    int32_t *state;
    double *scal, *target, *tmom, *mean, *Rt, *part;
    uint8_t *finite;
};

__device__ __forceinline__ int atom_row(const int32_t *sel, int k) { return sel ? sel[k] : k; }

// the centroid and G of a float64 structure M [m][3] by a whole workgroup -> tm[4] (thread 0 writes)
__device__ void target_moments(const double *M, int m, double *red, double *tm) {
    double c[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        double s = 0.0;
        for (int k = threadIdx.x; k < m; k += blockDim.x) s += M[3 * (size_t)k + r];
        c[r] = block_sum(s, red) / (double)m;
    }
    double g = 0.0;
    for (int k = threadIdx.x; k < m; k += blockDim.x) {
        const double dx = M[3 * (size_t)k] - c[0], dy = M[3 * (size_t)k + 1] - c[1], dz = M[3 * (size_t)k + 2] - c[2];
        g += (dx * dx + dy * dy) + dz * dz;
    }
    g = block_sum(g, red);
    if (threadIdx.x == 0) tm[0] = c[0], tm[1] = c[1], tm[2] = c[2], tm[3] = g;
}

__global__ __launch_bounds__(BLOCK) void pca_tmom_kernel(const double *M, int m, double *tm) {
    __shared__ double red[16];
    target_moments(M, m, red, tm);
}

// finite, W, the start structure, M_0 and its moments; only when the state says new
__global__ __launch_bounds__(1024) void pca_init_kernel(Fit f) {
    if (f.state[CODLAD_PCA_ST_PHASE] != PH_NEW) return;
    __shared__ double red[16];
    __shared__ int first[16];
    __shared__ int s_start;
    const int t = threadIdx.x;
    int mine = 0x7fffffff;                              // the first finite structure of positive weight
    for (int s = t; s < f.N; s += 1024) {
        const double *ms = f.mom + 4 * (size_t)s;
        const bool ok = fin64(ms[0]) && fin64(ms[1]) && fin64(ms[2]) && fin64(ms[3]);
        f.finite[s] = ok ? 1 : 0;
        if (ok && (!f.w || f.w[s] > 0.0) && s < mine) mine = s;
    }
#pragma unroll
    for (int st = 32; st > 0; st >>= 1) {
        const int o = __shfl_xor(mine, st);
        mine = o < mine ? o : mine;
    }
    if ((t & 63) == 0) first[t >> 6] = mine;
    __syncthreads();                                   // finite[] is written, too
    if (t == 0) {
        double W = 0.0;                                 // ascending index; a structure that is not finite has weight 0
        for (int s = 0; s < f.N; ++s)
            if (f.finite[s]) W += f.w ? f.w[s] : 1.0;
        int st = 0x7fffffff;
        for (int k = 0; k < 16; ++k) st = first[k] < st ? first[k] : st;
        if (f.start >= 0) st = (f.finite[f.start] && (!f.w || f.w[f.start] > 0.0)) ? f.start : 0x7fffffff;
        const bool ok = W > 0.0 && fin64(W) && st < f.N;
        f.scal[CODLAD_PCA_SC_W] = W;
        f.scal[CODLAD_PCA_SC_STEP] = nan64();
        f.state[CODLAD_PCA_ST_ITER] = 0;
        f.state[CODLAD_PCA_ST_START] = ok ? st : -1;
        f.state[CODLAD_PCA_ST_STATUS] = ok ? CODLAD_PCA_RUNNING : CODLAD_PCA_NO_WEIGHT;
        s_start = ok ? st : -1;
    }
    __syncthreads();
    const int st = s_start;
    if (st < 0) {                                       // nothing to fit: every result is NaN
        for (int e = t; e < 3 * f.m; e += 1024) f.mean[e] = f.target[e] = nan64();
        for (size_t e = t; e < 12 * (size_t)f.N; e += 1024) f.Rt[e] = nan64();
        if (t < 4) f.tmom[t] = nan64();
        __syncthreads();
        if (t == 0) f.state[CODLAD_PCA_ST_PHASE] = PH_DONE;
        return;
    }
    const float *xs = f.x + (size_t)st * f.n_atoms * 3;
    const double *ms = f.mom + 4 * (size_t)st;
    for (int e = t; e < 3 * f.m; e += 1024) {
        const int row = atom_row(f.sel, e / 3);
        const double v = (unsigned)row < (unsigned)f.n_atoms ? (double)xs[3 * (size_t)row + e % 3] - ms[e % 3] : nan64();
        f.target[e] = v;
        f.mean[e] = v;
    }
    __syncthreads();
    target_moments(f.target, f.m, red, f.tmom);
    __syncthreads();
    if (t == 0) f.state[CODLAD_PCA_ST_PHASE] = PH_RUNNING;
}

// a workgroup per structure.  state null: the free-standing alignment (codlad_pca_align), which also writes finite.
__global__ __launch_bounds__(BLOCK) void pca_align_kernel(const float *x, const double *mom, int n_atoms, const int32_t *sel, int m,
                                                          const double *target, const double *tmom, const int32_t *state,
                                                          double *Rt, uint8_t *finite) {
    if (state && state[CODLAD_PCA_ST_PHASE] != PH_RUNNING) return;
    __shared__ double part[4 * 9];
    const int s = blockIdx.x;
    const double *ms = mom + 4 * (size_t)s;
    const bool ok = fin64(ms[0]) && fin64(ms[1]) && fin64(ms[2]) && fin64(ms[3]);      // uniform
    if (!state && threadIdx.x == 0) finite[s] = ok ? 1 : 0;
    if (!ok) {
        if (threadIdx.x < 12) Rt[12 * (size_t)s + threadIdx.x] = nan64();
        return;
    }
    const float *xs = x + (size_t)s * n_atoms * 3;
    const double ca[3] = {ms[0], ms[1], ms[2]}, cb[3] = {tmom[0], tmom[1], tmom[2]};
    double S[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) S[k] = 0.0;
    for (int k = threadIdx.x; k < m; k += BLOCK) {
        const int row = atom_row(sel, k);
        double u[3], v[3];
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            u[r] = ((unsigned)row < (unsigned)n_atoms ? (double)xs[3 * (size_t)row + r] : nan64()) - ca[r];
            v[r] = target[3 * (size_t)k + r] - cb[r];
        }
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = 0; c < 3; ++c) S[3 * r + c] += u[r] * v[c];
    }
    // the tree of ensemble_kernels.hip: shuffle-down per wave, ((w0 + w1) + w2) + w3
#pragma unroll
    for (int k = 0; k < 9; ++k)
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) S[k] += __shfl_down(S[k], off, 64);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0)
#pragma unroll
        for (int k = 0; k < 9; ++k) part[wave * 9 + k] = S[k];
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < 9; ++k) S[k] = ((part[k] + part[9 + k]) + part[18 + k]) + part[27 + k];
        ens_solve_pair(S, ms[3], tmom[3], ca, cb, (double)m, Rt + 12 * (size_t)s);
    }
}

// A_sk = R_s x_sk + t_s, rounded as codlad_ens_apply rounds it before its conversion to fp32
__device__ __forceinline__ void moved_atom(const float *xs, const double *T, int row, int n_atoms, double a[3]) {
    if ((unsigned)row >= (unsigned)n_atoms) {
        a[0] = a[1] = a[2] = nan64();
        return;
    }
    const double u = (double)xs[3 * (size_t)row], v = (double)xs[3 * (size_t)row + 1], w = (double)xs[3 * (size_t)row + 2];
#pragma unroll
    for (int r = 0; r < 3; ++r) a[r] = ((T[3 * r] * u + T[3 * r + 1] * v) + T[3 * r + 2] * w) + T[9 + r];
}

// grid (ceil(m / 256), nch): part[ch][k][3] = the sum of w_s A_sk over the structures of chunk ch, ascending
__global__ __launch_bounds__(BLOCK) void pca_mean_kernel(Fit f) {
    if (f.state[CODLAD_PCA_ST_PHASE] != PH_RUNNING) return;
    const int k = blockIdx.x * BLOCK + threadIdx.x, ch = blockIdx.y;
    if (k >= f.m) return;
    const int row = atom_row(f.sel, k);
    const int s0 = ch * f.chunk, s1 = min(f.N, s0 + f.chunk);
    double acc[3] = {0.0, 0.0, 0.0};
    for (int s = s0; s < s1; ++s) {
        if (!f.finite[s]) continue;                    // uniform
        const double ws = f.w ? f.w[s] : 1.0;
        if (!(ws > 0.0)) continue;
        double a[3];
        moved_atom(f.x + (size_t)s * f.n_atoms * 3, f.Rt + 12 * (size_t)s, row, f.n_atoms, a);
#pragma unroll
        for (int r = 0; r < 3; ++r) acc[r] = fma(ws, a[r], acc[r]);
    }
#pragma unroll
    for (int r = 0; r < 3; ++r) f.part[((size_t)ch * f.m + k) * 3 + r] = acc[r];
}

__global__ __launch_bounds__(1024) void pca_step_kernel(Fit f) {
    if (f.state[CODLAD_PCA_ST_PHASE] != PH_RUNNING) return;
    __shared__ double red[16];
    const int t = threadIdx.x;
    const double W = f.scal[CODLAD_PCA_SC_W];
    double acc = 0.0;
    for (int e = t; e < 3 * f.m; e += 1024) {
        double v = 0.0;
        for (int ch = 0; ch < f.nch; ++ch) v += f.part[(size_t)ch * f.m * 3 + e];
        v /= W;
        const double dlt = v - f.target[e];
        acc = fma(dlt, dlt, acc);
        f.mean[e] = v;
    }
    const double step = sqrt(block_sum(acc, red) / (double)f.m);
    const int iter = f.state[CODLAD_PCA_ST_ITER] + 1;
    const bool conv = step <= f.tol, done = conv || iter >= f.max_iter || !fin64(step);      // uniform
    __syncthreads();                                   // everybody has read the state
    if (!done) {
        for (int e = t; e < 3 * f.m; e += 1024) f.target[e] = f.mean[e];
        __syncthreads();
        target_moments(f.target, f.m, red, f.tmom);
    }
    if (t == 0) {
        f.scal[CODLAD_PCA_SC_STEP] = step;
        f.state[CODLAD_PCA_ST_ITER] = iter;
        if (done) {
            f.state[CODLAD_PCA_ST_STATUS] = conv ? CODLAD_PCA_CONVERGED : CODLAD_PCA_LIMIT;
            f.state[CODLAD_PCA_ST_PHASE] = PH_DONE;
        }
    }
}

// ------------------------------------------------------------------------------------------- deviations and RMSF --
// grid (N, ceil(m / 256)): D [N][3 m] = A_s - mean, NaN for a structure that is not finite
__global__ __launch_bounds__(BLOCK) void pca_dev_kernel(const float *x, const double *Rt, const uint8_t *finite, int n_atoms,
                                                        const int32_t *sel, int m, const double *mean, double *D) {
    const int k = blockIdx.y * BLOCK + threadIdx.x, s = blockIdx.x;
    if (k >= m) return;
    double a[3] = {nan64(), nan64(), nan64()};
    if (finite[s]) moved_atom(x + (size_t)s * n_atoms * 3, Rt + 12 * (size_t)s, atom_row(sel, k), n_atoms, a);
#pragma unroll
    for (int r = 0; r < 3; ++r) D[(size_t)s * 3 * m + 3 * (size_t)k + r] = a[r] - mean[3 * (size_t)k + r];
}

// thread k: rmsf[k] = sqrt(sum_s w_s |D_sk|^2 / W), the structures in ascending order, D recomputed as pca_dev_kernel does
__global__ __launch_bounds__(BLOCK) void pca_rmsf_kernel(const float *x, const double *Rt, const uint8_t *finite, const double *w,
                                                         int N, int n_atoms, const int32_t *sel, int m, const double *mean,
                                                         const double *scal, double *rmsf) {
    const int k = blockIdx.x * BLOCK + threadIdx.x;
    if (k >= m) return;
    const int row = atom_row(sel, k);
    const double mk[3] = {mean[3 * (size_t)k], mean[3 * (size_t)k + 1], mean[3 * (size_t)k + 2]};
    double acc = 0.0;
    for (int s = 0; s < N; ++s) {
        if (!finite[s]) continue;
        const double ws = w ? w[s] : 1.0;
        if (!(ws > 0.0)) continue;
        double a[3];
        moved_atom(x + (size_t)s * n_atoms * 3, Rt + 12 * (size_t)s, row, n_atoms, a);
        const double dx = a[0] - mk[0], dy = a[1] - mk[1], dz = a[2] - mk[2];
        acc = fma(ws, (dx * dx + dy * dy) + dz * dz, acc);
    }
    rmsf[k] = sqrt(acc / scal[CODLAD_PCA_SC_W]);
}

// ----------------------------------------------------------------------------------------------------- covariance --
constexpr int TILE = 64;                    // coordinates of a tile side
constexpr int KC = 16;                      // structures of a staging step
constexpr int ROW = TILE + 16;              // doubles of one structure of a panel in LDS
constexpr int CT = 256;                     // threads: 4 waves, wave ti owns rows 16 ti .. of the tile
constexpr int LOADS = 2 * KC * TILE / CT;   // per thread and step
static_assert(2 * KC * TILE % CT == 0, "the step is spread evenly");

struct Cov {
    const double *D, *w, *scal;
    const uint8_t *finite;
    int N, d, ntiles, nch, chunk;
    double *part, *C;
};

// element e of a step's 2 * KC * TILE doubles: block I's rows, then block J's times the weight
__device__ __forceinline__ double cov_load(const Cov &p, int I, int J, int s0, int s1, int e) {
    const int which = e / (KC * TILE), r = (e % (KC * TILE)) / TILE, c = e % TILE;
    const int s = s0 + r, col = (which ? J : I) * TILE + c;
    if (s >= s1 || col >= p.d || !p.finite[s]) return 0.0;
    const double ws = p.w ? p.w[s] : 1.0;
    if (!(ws > 0.0)) return 0.0;
    const double v = p.D[(size_t)s * p.d + col];
    return which ? v * ws : v;
}

__global__ __launch_bounds__(CT) void pca_cov_kernel(Cov p) {
    __shared__ double panel[2][KC * ROW];
    int I, J;
    tri_tile_of(blockIdx.x, I, J);
    const int ch = blockIdx.y, t = threadIdx.x, lane = t & 63, ti = t >> 6;
    const int lr = lane & 15, lk = lane >> 4;
    const int s_begin = ch * p.chunk, s_end = min(p.N, s_begin + p.chunk);
    double4_t acc[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) acc[u] = double4_t{0.0, 0.0, 0.0, 0.0};
    double stage[LOADS];
#pragma unroll
    for (int l = 0; l < LOADS; ++l) stage[l] = cov_load(p, I, J, s_begin, s_end, t + l * CT);
    for (int s0 = s_begin; s0 < s_end; s0 += KC) {
        __syncthreads();                                     // the previous step has been read
#pragma unroll
        for (int l = 0; l < LOADS; ++l) {
            const int e = t + l * CT;
            panel[e / (KC * TILE)][((e % (KC * TILE)) / TILE) * ROW + e % TILE] = stage[l];
        }
        __syncthreads();
        if (s0 + KC < s_end)
#pragma unroll
            for (int l = 0; l < LOADS; ++l) stage[l] = cov_load(p, I, J, s0 + KC, s_end, t + l * CT);
#pragma unroll
        for (int s4 = 0; s4 < KC / 4; ++s4) {
            const double a = panel[0][(s4 * 4 + lk) * ROW + ti * 16 + lr];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                if (I == J && u > ti) continue;              // above the diagonal of a diagonal tile: uniform in the wave
                const double b = panel[1][(s4 * 4 + lk) * ROW + u * 16 + lr];
                acc[u] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[u], 0, 0, 0);
            }
        }
    }
    // element (row lk + 4 reg of wave tile ti, column lr of wave tile u)
    double *out = p.part + ((size_t)ch * p.ntiles + blockIdx.x) * (TILE * TILE);
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const double4_t v = acc[u];
        const int col = u * 16 + lr, row = ti * 16 + lk;
        out[(row + 0) * TILE + col] = v.x;
        out[(row + 4) * TILE + col] = v.y;
        out[(row + 8) * TILE + col] = v.z;
        out[(row + 12) * TILE + col] = v.w;
    }
}

// a workgroup per tile: element (i, j), i >= j, = the chunks in ascending order / W, written with its mirror
__global__ __launch_bounds__(BLOCK) void pca_cov_reduce_kernel(Cov p) {
    int I, J;
    tri_tile_of(blockIdx.x, I, J);
    const double W = p.scal[CODLAD_PCA_SC_W];
    for (int e = threadIdx.x; e < TILE * TILE; e += BLOCK) {
        const int i = I * TILE + e / TILE, j = J * TILE + e % TILE;
        if (i >= p.d || j >= p.d || j > i) continue;
        double v = 0.0;
        for (int ch = 0; ch < p.nch; ++ch) v += p.part[((size_t)ch * p.ntiles + blockIdx.x) * (TILE * TILE) + e];
        v /= W;
        p.C[(size_t)i * p.d + j] = v;
        if (i != j) p.C[(size_t)j * p.d + i] = v;
    }
}

// corr [m][m]: the trace of block (a, b) over the root of the two diagonal traces, the diagonal 1 where the trace is positive
// and NaN elsewhere; block 0 also adds the diagonal of C in ascending order -> total
__global__ __launch_bounds__(BLOCK) void pca_corr_kernel(const double *C, int d, int m, double *corr, double *total) {
    const size_t e = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        double s = 0.0;
        for (int i = 0; i < d; ++i) s += C[(size_t)i * d + i];
        *total = s;
    }
    if (e >= (size_t)m * m) return;
    const int a = (int)(e / m), b = (int)(e % m);
    const int lo = a < b ? a : b, hi = a < b ? b : a;       // one formula for (a, b) and (b, a)
    const double ta = (C[(size_t)(3 * lo) * d + 3 * lo] + C[(size_t)(3 * lo + 1) * d + 3 * lo + 1]) + C[(size_t)(3 * lo + 2) * d + 3 * lo + 2];
    const double tb = (C[(size_t)(3 * hi) * d + 3 * hi] + C[(size_t)(3 * hi + 1) * d + 3 * hi + 1]) + C[(size_t)(3 * hi + 2) * d + 3 * hi + 2];
    const double tab = (C[(size_t)(3 * hi) * d + 3 * lo] + C[(size_t)(3 * hi + 1) * d + 3 * lo + 1]) + C[(size_t)(3 * hi + 2) * d + 3 * lo + 2];
    corr[e] = a == b ? (ta > 0.0 ? 1.0 : nan64()) : tab / sqrt(ta * tb);
}

// ----------------------------------------------------------------------------------------------------- eigenpairs --
struct Eig {
    const double *C;
    int d, k, b, max_iter;
    double rtol;
    int32_t *state;
    double *Q, *Z, *V, *Y, *H, *S, *Ss, *theta, *resid, *sgn;      // scratch
    double *evals, *comps, *res_out;                               // results
};

// the start block: a fixed table of numbers in [-1/2, 1/2) from an integer hash of (column, row)
__device__ __forceinline__ double start_entry(int j, int r) {
    unsigned h = (unsigned)r * 2654435761u + (unsigned)j * 40503u + 12345u;
    h ^= h >> 15;
    h *= 2246822519u;
    h ^= h >> 13;
    h *= 3266489917u;
    h ^= h >> 16;
    return (double)(h >> 8) * 0x1p-24 - 0.5;
}

constexpr int OT = 1024, OE = MAX_D / OT;   // orth_kernel: threads, rows of a thread
static_assert(OE * OT == MAX_D, "a thread's rows cover the largest dimension");

// One pass of Gram-Schmidt of v (this thread's rows) against the columns 0 .. j - 1 of Q: the j dot products first, then
// the j subtractions in ascending order.  Returns nothing; v is updated.
__device__ void gs_pass(const double *Q, int d, int j, double v[OE], double (*red)[MAX_B], double *dots) {
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    __syncthreads();                                   // red and dots of the previous pass have been read
    for (int i = 0; i < j; ++i) {
        double p = 0.0;
#pragma unroll
        for (int e = 0; e < OE; ++e) {
            const int r = t + OT * e;
            if (r < d) p = fma(Q[(size_t)i * d + r], v[e], p);
        }
        p = wave_sum(p);
        if (lane == 0) red[wave][i] = p;
    }
    __syncthreads();
    if (t < j) {
        double s = 0.0;
        for (int k = 0; k < OT / 64; ++k) s += red[k][t];
        dots[t] = s;
    }
    __syncthreads();
    for (int i = 0; i < j; ++i) {
        const double c = dots[i];
#pragma unroll
        for (int e = 0; e < OE; ++e) {
            const int r = t + OT * e;
            if (r < d) v[e] = fma(-c, Q[(size_t)i * d + r], v[e]);
        }
    }
}

__device__ double norm2_of(const double v[OE], double *red16) {
    double p = 0.0;
#pragma unroll
    for (int e = 0; e < OE; ++e) p = fma(v[e], v[e], p);
    return block_sum(p, red16);
}

// Q <- the orthonormalised Y (START: the start block).  One workgroup, column after column.
template <bool START> __global__ __launch_bounds__(OT) void pca_orth_kernel(Eig g) {
    if (g.state[CODLAD_PCA_ST_PHASE] != (START ? PH_NEW : PH_RUNNING)) return;
    __shared__ double red[OT / 64][MAX_B];
    __shared__ double dots[MAX_B];
    __shared__ double red16[16];
    const int t = threadIdx.x, d = g.d;
    int unit = 0;                                       // the next unit vector to stand in for a column that vanished
    for (int j = 0; j < g.b; ++j) {
        double v[OE];
#pragma unroll
        for (int e = 0; e < OE; ++e) {
            const int r = t + OT * e;
            v[e] = r < d ? (START ? start_entry(j, r) : g.Y[(size_t)j * d + r]) : 0.0;
        }
        gs_pass(g.Q, d, j, v, red, dots);
        const double n1 = norm2_of(v, red16);
        gs_pass(g.Q, d, j, v, red, dots);
        double n2 = norm2_of(v, red16);
        // the column has vanished when the second pass still halves what the first left (Parlett's "twice is enough"
        // test), or when nothing is left; then e_p, p = 0, 1, .. in turn, stands in: the first whose remainder after both
        // passes is at least 1 / 128 long (one exists while j < d: their squares add up to d - j)
        bool gone = !(n1 > 0.0) || !(n2 > 0.25 * n1) || !fin64(n2);      // uniform: every thread holds the same sums
        while (gone && unit < d) {
#pragma unroll
            for (int e = 0; e < OE; ++e) v[e] = t + OT * e == unit ? 1.0 : 0.0;
            ++unit;
            gs_pass(g.Q, d, j, v, red, dots);
            gs_pass(g.Q, d, j, v, red, dots);
            n2 = norm2_of(v, red16);
            gone = !(n2 >= 0x1p-14);
        }
        const double inv = gone ? 0.0 : 1.0 / sqrt(n2);
#pragma unroll
        for (int e = 0; e < OE; ++e) {
            const int r = t + OT * e;
            if (r < d) g.Q[(size_t)j * d + r] = gone ? 0.0 : v[e] * inv;
        }
        __syncthreads();                                // column j is visible to the workgroup
    }
    if (START && t == 0) {
        g.state[CODLAD_PCA_ST_ITER] = 0;
        g.state[CODLAD_PCA_ST_STATUS] = CODLAD_PCA_RUNNING;
        g.state[CODLAD_PCA_ST_PHASE] = PH_RUNNING;
    }
}

constexpr int CQ_COLS = 8;
// grid (ceil(d / 256), ceil(b / 8)): Z[j][i] = sum_l C[l][i] Q[j][l], l ascending
__global__ __launch_bounds__(BLOCK) void pca_cq_kernel(Eig g) {
    if (g.state[CODLAD_PCA_ST_PHASE] != PH_RUNNING) return;
    const int i = blockIdx.x * BLOCK + threadIdx.x, j0 = blockIdx.y * CQ_COLS, d = g.d;
    if (i >= d) return;
    const int nj = min(CQ_COLS, g.b - j0);
    double acc[CQ_COLS];
#pragma unroll
    for (int u = 0; u < CQ_COLS; ++u) acc[u] = 0.0;
    for (int l = 0; l < d; ++l) {
        const double c = g.C[(size_t)l * d + i];
#pragma unroll
        for (int u = 0; u < CQ_COLS; ++u)
            if (u < nj) acc[u] = fma(c, g.Q[(size_t)(j0 + u) * d + l], acc[u]);
    }
#pragma unroll
    for (int u = 0; u < CQ_COLS; ++u)
        if (u < nj) g.Z[(size_t)(j0 + u) * d + i] = acc[u];
}

// a workgroup per (p, q), p >= q: H[p][q] = H[q][p] = Q_p . Z_q
__global__ __launch_bounds__(BLOCK) void pca_h_kernel(Eig g) {
    if (g.state[CODLAD_PCA_ST_PHASE] != PH_RUNNING) return;
    __shared__ double red[16];
    int p, q;
    tri_tile_of(blockIdx.x, p, q);
    double acc = 0.0;
    for (int r = threadIdx.x; r < g.d; r += BLOCK) acc = fma(g.Q[(size_t)p * g.d + r], g.Z[(size_t)q * g.d + r], acc);
    // 0.0 +: when every product underflows to -0.0 the waves' sum is -0.0, and its sign would reach H, a diagonal element
    // the Jacobi never rotates and so an eigenvalue; every other block_sum of this file adds squares or plain coordinates
    // from +0.0 and cannot be -0.0
    acc = 0.0 + block_sum(acc, red);
    if (threadIdx.x == 0) g.H[p * g.b + q] = g.H[q * g.b + p] = acc;
}

// One workgroup: cyclic Jacobi on H [b][b] (Golub & Van Loan 8.4, the rotation of ens_jacobi4) in the round-robin order:
// n = b rounded up to even, round r of n - 1 pairs (n - 1, r) and ((r + i) mod (n - 1), (r - i) mod (n - 1)), i = 1 .. n / 2 -
// 1; the pairs of a round are disjoint, so A <- A J for all of them, then A <- J^T A, then S <- S J.  A sweep starts only
// while off(A)^2 > 2^-120 |A|_F^2.  -> theta in descending order (the lower index first among equals), Ss = S's columns
// in that order.
constexpr int JT = 1024, LDH = MAX_B + 1;
__global__ __launch_bounds__(JT) void pca_jacobi_kernel(Eig g) {
    if (g.state[CODLAD_PCA_ST_PHASE] != PH_RUNNING) return;
    __shared__ double A[MAX_B * LDH];
    __shared__ double cs[MAX_B / 2][2];
    __shared__ int pq[MAX_B / 2][2];
    __shared__ double red[16];
    const int t = threadIdx.x, b = g.b, n = b + (b & 1), half = n / 2;
    for (int e = t; e < b * b; e += JT) {
        A[(e / b) * LDH + e % b] = g.H[e];
        g.S[e] = e / b == e % b ? 1.0 : 0.0;
    }
    __syncthreads();
    for (int sweep = 0; sweep < 40; ++sweep) {
        double off = 0.0, diag = 0.0;
        for (int e = t; e < b * b; e += JT) {
            const double a = A[(e / b) * LDH + e % b];
            if (e / b == e % b) diag = fma(a, a, diag);
            else off = fma(a, a, off);
        }
        off = block_sum(off, red);
        diag = block_sum(diag, red);
        if (!(off > 0x1p-120 * (diag + off))) break;   // uniform; NaN leaves, too
        for (int round = 0; round < n - 1; ++round) {
            if (t < half) {
                int p = t == 0 ? n - 1 : (round + t) % (n - 1), q = t == 0 ? round : (round - t + n - 1) % (n - 1);
                if (p > q) {
                    const int h = p;
                    p = q, q = h;
                }
                double c = 1.0, s = 0.0;
                if (q < b && A[p * LDH + q] != 0.0) {
                    const double tau = (A[q * LDH + q] - A[p * LDH + p]) / (2.0 * A[p * LDH + q]);
                    const double tt = tau >= 0.0 ? 1.0 / (tau + sqrt(1.0 + tau * tau)) : -1.0 / (-tau + sqrt(1.0 + tau * tau));
                    c = 1.0 / sqrt(1.0 + tt * tt), s = tt * c;
                }
                pq[t][0] = p, pq[t][1] = q < b ? q : -1;
                cs[t][0] = c, cs[t][1] = s;
            }
            __syncthreads();
            for (int e = t; e < b * half; e += JT) {      // A <- A J
                const int k = e / half, pr = e % half, p = pq[pr][0], q = pq[pr][1];
                if (q < 0) continue;
                const double c = cs[pr][0], s = cs[pr][1], x = A[k * LDH + p], y = A[k * LDH + q];
                A[k * LDH + p] = c * x - s * y;
                A[k * LDH + q] = s * x + c * y;
            }
            __syncthreads();
            for (int e = t; e < b * half; e += JT) {      // A <- J^T A, S <- S J
                const int k = e / half, pr = e % half, p = pq[pr][0], q = pq[pr][1];
                if (q < 0) continue;
                const double c = cs[pr][0], s = cs[pr][1];
                double x = A[p * LDH + k], y = A[q * LDH + k];
                A[p * LDH + k] = c * x - s * y;
                A[q * LDH + k] = s * x + c * y;
                x = g.S[k * b + p], y = g.S[k * b + q];
                g.S[k * b + p] = c * x - s * y;
                g.S[k * b + q] = s * x + c * y;
            }
            __syncthreads();
            if (t < half && pq[t][1] >= 0 && cs[t][1] != 0.0) {
                A[pq[t][0] * LDH + pq[t][1]] = 0.0;        // what the rotation was chosen for, exactly
                A[pq[t][1] * LDH + pq[t][0]] = 0.0;
            }
            __syncthreads();
        }
    }
    __syncthreads();
    if (t < b) {
        const double th = A[t * LDH + t];
        int rank = 0;
        for (int j = 0; j < b; ++j) {
            const double o = A[j * LDH + j];
            if (o > th || (o == th && j < t)) ++rank;
        }
        g.theta[rank] = th;
        for (int k = 0; k < b; ++k) g.Ss[k * b + rank] = g.S[k * b + t];
    }
}

// a workgroup per Ritz pair i: V_i = sum_j Q_j Ss[j][i], Y_i = sum_j Z_j Ss[j][i] (j ascending), resid[i] = |Y_i - theta_i
// V_i|_2, sgn[i] = the sign that makes the entry of largest magnitude (the lowest index among equals) positive
__global__ __launch_bounds__(BLOCK) void pca_rot_kernel(Eig g) {
    if (g.state[CODLAD_PCA_ST_PHASE] != PH_RUNNING) return;
    __shared__ double red[16];
    __shared__ double best_a[BLOCK / 64];
    __shared__ int best_r[BLOCK / 64];
    const int i = blockIdx.x, t = threadIdx.x, d = g.d, b = g.b;
    const double th = g.theta[i];
    double acc = 0.0, ba = -1.0;
    int br = 0x7fffffff;
    for (int r = t; r < d; r += BLOCK) {
        double v = 0.0, y = 0.0;
        for (int j = 0; j < b; ++j) {
            const double s = g.Ss[j * b + i];
            v = fma(g.Q[(size_t)j * d + r], s, v);
            y = fma(g.Z[(size_t)j * d + r], s, y);
        }
        g.V[(size_t)i * d + r] = v;
        g.Y[(size_t)i * d + r] = y;
        const double e = y - th * v;
        acc = fma(e, e, acc);
        if (fabs(v) > ba) ba = fabs(v), br = r;        // r ascends: the lowest index among equals stays
    }
    acc = block_sum(acc, red);
#pragma unroll
    for (int st = 32; st > 0; st >>= 1) {
        const double oa = __shfl_xor(ba, st);
        const int orr = __shfl_xor(br, st);
        if (oa > ba || (oa == ba && orr < br)) ba = oa, br = orr;
    }
    if ((t & 63) == 0) best_a[t >> 6] = ba, best_r[t >> 6] = br;
    __syncthreads();
    if (t == 0) {
        for (int k = 1; k < BLOCK / 64; ++k)
            if (best_a[k] > ba || (best_a[k] == ba && best_r[k] < br)) ba = best_a[k], br = best_r[k];
        g.resid[i] = sqrt(acc);
        g.sgn[i] = br < d && g.V[(size_t)i * d + br] < 0.0 ? -1.0 : 1.0;     // this thread's or another's write: after the barrier
    }
}

__global__ __launch_bounds__(BLOCK) void pca_status_kernel(Eig g) {
    if (g.state[CODLAD_PCA_ST_PHASE] != PH_RUNNING) return;
    const int t = threadIdx.x, iter = g.state[CODLAD_PCA_ST_ITER] + 1;
    const double lim = g.rtol * g.theta[0];
    bool conv = true;
    for (int i = 0; i < g.k; ++i) conv = conv && g.resid[i] <= lim;      // every thread the same answer; NaN fails
    const bool done = conv || iter >= g.max_iter;
    if (done) {
        for (int i = t; i < g.k; i += BLOCK) g.evals[i] = g.theta[i], g.res_out[i] = g.resid[i];
        for (size_t e = t; e < (size_t)g.k * g.d; e += BLOCK) g.comps[e] = g.sgn[e / g.d] * g.V[e];
    }
    __syncthreads();                                   // everybody has read the state
    if (t == 0) {
        g.state[CODLAD_PCA_ST_ITER] = iter;
        if (done) {
            g.state[CODLAD_PCA_ST_STATUS] = conv ? CODLAD_PCA_CONVERGED : CODLAD_PCA_LIMIT;
            g.state[CODLAD_PCA_ST_PHASE] = PH_DONE;
        }
    }
}

// thread (s, i): P[s][i] = sum_r D[s][r] V[i][r], r ascending
__global__ __launch_bounds__(BLOCK) void pca_project_kernel(const double *D, const double *V, int N, int d, int k, double *P) {
    const size_t e = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (e >= (size_t)N * k) return;
    const double *ds = D + (e / k) * (size_t)d, *vi = V + (e % k) * (size_t)d;
    double acc = 0.0;
    for (int r = 0; r < d; ++r) acc = fma(ds[r], vi[r], acc);
    P[e] = acc;
}

bool positive(double v) { return v > 0.0 && v < __builtin_inf(); }
long long eig_doubles(int d, int b) { return 4ll * b * d + 3ll * b * b + 3ll * b; }
}  // namespace

extern "C" long long codlad_pca_fit_scratch_bytes(int N, int n_sel) {
    CODLAD_REQUIRE(N > 0 && N <= MAX_N && n_sel > 0, "bad sizes (1 <= N <= CODLAD_PCA_MAX_N, n_sel >= 1)");
    return 8ll * (3ll * n_sel * chunks_of(N).nch + 4);
}

extern "C" int codlad_pca_fit(const float *x, const double *mom, int N, int n_atoms, const int32_t *sel, int n_sel,
                              const double *w, int start, double tol, int max_iter, int iters, int32_t *state, double *scal,
                              double *target, double *mean, double *Rt, uint8_t *finite, void *scratch, void *stream) {
    CODLAD_REQUIRE(x && mom && state && scal && target && mean && Rt && finite && scratch, "null pointer");
    CODLAD_REQUIRE(N > 0 && N <= MAX_N && n_atoms > 0 && n_sel >= 0, "bad sizes (1 <= N <= CODLAD_PCA_MAX_N)");
    const int m = subset_size(sel, n_sel, n_atoms);
    CODLAD_REQUIRE(m > 0, "sel and n_sel disagree (sel with n_sel > 0, or neither)");
    CODLAD_REQUIRE(start >= -1 && start < N, "start outside -1 .. N - 1");
    CODLAD_REQUIRE(positive(tol), "tol is not a positive finite number");
    CODLAD_REQUIRE(max_iter >= 1 && max_iter <= CODLAD_PCA_MAX_ITER && iters >= 0 && iters <= CODLAD_PCA_MAX_ITER,
                   "max_iter outside 1 .. CODLAD_PCA_MAX_ITER or iters outside 0 .. CODLAD_PCA_MAX_ITER");
    const Chunks c = chunks_of(N);
    Fit f;
    f.x = x, f.mom = mom, f.w = w, f.sel = sel, f.N = N, f.n_atoms = n_atoms, f.m = m, f.start = start, f.max_iter = max_iter;
    f.nch = c.nch, f.chunk = c.chunk, f.tol = tol, f.state = state, f.scal = scal, f.target = target, f.mean = mean, f.Rt = Rt;
    f.tmom = (double *)scratch, f.part = f.tmom + 4, f.finite = finite;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(pca_init_kernel, dim3(1), dim3(1024), 0, st, f);              // returns at once unless the state says new
    const dim3 mgrid((unsigned)((m + BLOCK - 1) / BLOCK), (unsigned)c.nch);
    for (int it = 0; it < iters; ++it) {
        hipLaunchKernelGGL(pca_align_kernel, dim3(N), dim3(BLOCK), 0, st, x, mom, n_atoms, sel, m, (const double *)target,
                           (const double *)f.tmom, (const int32_t *)state, Rt, finite);
        hipLaunchKernelGGL(pca_mean_kernel, mgrid, dim3(BLOCK), 0, st, f);
        hipLaunchKernelGGL(pca_step_kernel, dim3(1), dim3(1024), 0, st, f);
    }
    return codlad_check_launch("codlad_pca_fit");
}

extern "C" int codlad_pca_align(const float *x, const double *mom, int N, int n_atoms, const int32_t *sel, int n_sel,
                                const double *target, double *tmom, double *Rt, uint8_t *finite, void *stream) {
    CODLAD_REQUIRE(x && mom && target && tmom && Rt && finite, "null pointer");
    CODLAD_REQUIRE(N > 0 && N <= MAX_N && n_atoms > 0 && n_sel >= 0, "bad sizes (1 <= N <= CODLAD_PCA_MAX_N)");
    const int m = subset_size(sel, n_sel, n_atoms);
    CODLAD_REQUIRE(m > 0, "sel and n_sel disagree (sel with n_sel > 0, or neither)");
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(pca_tmom_kernel, dim3(1), dim3(BLOCK), 0, st, target, m, tmom);
    hipLaunchKernelGGL(pca_align_kernel, dim3(N), dim3(BLOCK), 0, st, x, mom, n_atoms, sel, m, target, (const double *)tmom,
                       (const int32_t *)nullptr, Rt, finite);
    return codlad_check_launch("codlad_pca_align");
}

extern "C" int codlad_pca_deviations(const float *x, const double *Rt, const uint8_t *finite, const double *w, int N, int n_atoms,
                                     const int32_t *sel, int n_sel, const double *mean, const double *scal, double *D,
                                     double *rmsf, void *stream) {
    CODLAD_REQUIRE(x && Rt && finite && mean && (D || rmsf), "null pointer");
    CODLAD_REQUIRE(!rmsf || scal, "rmsf asks for scal");
    CODLAD_REQUIRE(N > 0 && N <= MAX_N && n_atoms > 0 && n_sel >= 0, "bad sizes (1 <= N <= CODLAD_PCA_MAX_N)");
    const int m = subset_size(sel, n_sel, n_atoms);
    CODLAD_REQUIRE(m > 0, "sel and n_sel disagree (sel with n_sel > 0, or neither)");
    hipStream_t st = (hipStream_t)stream;
    const unsigned bx = (unsigned)((m + BLOCK - 1) / BLOCK);
    if (D) hipLaunchKernelGGL(pca_dev_kernel, dim3((unsigned)N, bx), dim3(BLOCK), 0, st, x, Rt, finite, n_atoms, sel, m, mean, D);
    if (rmsf) hipLaunchKernelGGL(pca_rmsf_kernel, dim3(bx), dim3(BLOCK), 0, st, x, Rt, finite, w, N, n_atoms, sel, m, mean, scal, rmsf);
    return codlad_check_launch("codlad_pca_deviations");
}

extern "C" long long codlad_pca_covariance_scratch_bytes(int N, int d) {
    CODLAD_REQUIRE(N > 0 && N <= MAX_N && d > 0 && d <= MAX_D && d % 3 == 0,
                   "bad sizes (1 <= N <= CODLAD_PCA_MAX_N, d = 3 m <= CODLAD_PCA_MAX_DIM)");
    return 8ll * chunks_of(N).nch * tri_tiles_of(d, TILE) * TILE * TILE;
}

extern "C" int codlad_pca_covariance(const double *D, const double *w, const uint8_t *finite, int N, int d, const double *scal,
                                     double *cov, double *corr, double *total, void *scratch, void *stream) {
    CODLAD_REQUIRE(D && finite && scal && cov && corr && total && scratch, "null pointer");
    CODLAD_REQUIRE(N > 0 && N <= MAX_N && d > 0 && d <= MAX_D && d % 3 == 0,
                   "bad sizes (1 <= N <= CODLAD_PCA_MAX_N, d = 3 m <= CODLAD_PCA_MAX_DIM)");
    const Chunks c = chunks_of(N);
    Cov p;
    p.D = D, p.w = w, p.scal = scal, p.finite = finite, p.N = N, p.d = d, p.ntiles = tri_tiles_of(d, TILE);
    p.nch = c.nch, p.chunk = c.chunk, p.part = (double *)scratch, p.C = cov;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(pca_cov_kernel, dim3((unsigned)p.ntiles, (unsigned)p.nch), dim3(CT), 0, st, p);
    hipLaunchKernelGGL(pca_cov_reduce_kernel, dim3((unsigned)p.ntiles), dim3(BLOCK), 0, st, p);
    const int m = d / 3;
    hipLaunchKernelGGL(pca_corr_kernel, dim3((unsigned)(((long long)m * m + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, st,
                       (const double *)cov, d, m, corr, total);
    return codlad_check_launch("codlad_pca_covariance");
}

// the diagonal of C in ascending order, as pca_corr_kernel's block 0 adds it
namespace {
__global__ void pca_trace_kernel(const double *C, int d, double *total) {
    double s = 0.0;
    for (int i = 0; i < d; ++i) s += C[(size_t)i * d + i];
    *total = s;
}
}  // namespace

extern "C" long long codlad_feature_covariance_scratch_bytes(int N, int d) {
    CODLAD_REQUIRE(N > 0 && N <= MAX_N && d > 0 && d <= MAX_D, "bad sizes (1 <= N <= CODLAD_PCA_MAX_N, 1 <= d <= CODLAD_PCA_MAX_DIM)");
    return 8ll * chunks_of(N).nch * tri_tiles_of(d, TILE) * TILE * TILE;
}

extern "C" int codlad_feature_covariance(const double *D, const double *w, const uint8_t *finite, int N, int d, const double *scal,
                                         double *cov, double *total, void *scratch, void *stream) {
    CODLAD_REQUIRE(D && finite && scal && cov && total && scratch, "null pointer");
    CODLAD_REQUIRE(N > 0 && N <= MAX_N && d > 0 && d <= MAX_D, "bad sizes (1 <= N <= CODLAD_PCA_MAX_N, 1 <= d <= CODLAD_PCA_MAX_DIM)");
    const Chunks c = chunks_of(N);
    Cov p;
    p.D = D, p.w = w, p.scal = scal, p.finite = finite, p.N = N, p.d = d, p.ntiles = tri_tiles_of(d, TILE);
    p.nch = c.nch, p.chunk = c.chunk, p.part = (double *)scratch, p.C = cov;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(pca_cov_kernel, dim3((unsigned)p.ntiles, (unsigned)p.nch), dim3(CT), 0, st, p);
    hipLaunchKernelGGL(pca_cov_reduce_kernel, dim3((unsigned)p.ntiles), dim3(BLOCK), 0, st, p);
    hipLaunchKernelGGL(pca_trace_kernel, dim3(1), dim3(1), 0, st, (const double *)cov, d, total);
    return codlad_check_launch("codlad_feature_covariance");
}

extern "C" long long codlad_pca_eigen_scratch_bytes(int d, int k) {
    CODLAD_REQUIRE(d > 0 && d <= MAX_D && k >= 1 && k <= MAX_K && k <= d,
                   "bad sizes (1 <= d <= CODLAD_PCA_MAX_DIM, 1 <= k <= min(CODLAD_PCA_MAX_COMPONENTS, d))");
    return 8ll * eig_doubles(d, k + 8 < d ? k + 8 : d);
}

extern "C" int codlad_pca_eigen(const double *cov, int d, int k, double rtol, int max_iter, int iters, int32_t *state,
                                double *evals, double *comps, double *resid, void *scratch, void *stream) {
    CODLAD_REQUIRE(cov && state && evals && comps && resid && scratch, "null pointer");
    CODLAD_REQUIRE(d > 0 && d <= MAX_D && k >= 1 && k <= MAX_K && k <= d,
                   "bad sizes (1 <= d <= CODLAD_PCA_MAX_DIM, 1 <= k <= min(CODLAD_PCA_MAX_COMPONENTS, d))");
    CODLAD_REQUIRE(positive(rtol), "rtol is not a positive finite number");
    CODLAD_REQUIRE(max_iter >= 1 && max_iter <= CODLAD_PCA_MAX_ITER && iters >= 0 && iters <= CODLAD_PCA_MAX_ITER,
                   "max_iter outside 1 .. CODLAD_PCA_MAX_ITER or iters outside 0 .. CODLAD_PCA_MAX_ITER");
    Eig g;
    const int b = k + 8 < d ? k + 8 : d;
    g.C = cov, g.d = d, g.k = k, g.b = b, g.max_iter = max_iter, g.rtol = rtol, g.state = state;
    double *s = (double *)scratch;
    const size_t bd = (size_t)b * d, bb = (size_t)b * b;
    g.Q = s, g.Z = s + bd, g.V = s + 2 * bd, g.Y = s + 3 * bd;
    g.H = s + 4 * bd, g.S = g.H + bb, g.Ss = g.S + bb, g.theta = g.Ss + bb, g.resid = g.theta + b, g.sgn = g.resid + b;
    g.evals = evals, g.comps = comps, g.res_out = resid;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(pca_orth_kernel<true>, dim3(1), dim3(OT), 0, st, g);          // only when the state says new
    const dim3 cq((unsigned)((d + BLOCK - 1) / BLOCK), (unsigned)((b + CQ_COLS - 1) / CQ_COLS));
    for (int it = 0; it < iters; ++it) {
        hipLaunchKernelGGL(pca_cq_kernel, cq, dim3(BLOCK), 0, st, g);
        hipLaunchKernelGGL(pca_h_kernel, dim3((unsigned)(b * (b + 1) / 2)), dim3(BLOCK), 0, st, g);
        hipLaunchKernelGGL(pca_jacobi_kernel, dim3(1), dim3(JT), 0, st, g);
        hipLaunchKernelGGL(pca_rot_kernel, dim3((unsigned)b), dim3(BLOCK), 0, st, g);
        hipLaunchKernelGGL(pca_status_kernel, dim3(1), dim3(BLOCK), 0, st, g);
        hipLaunchKernelGGL(pca_orth_kernel<false>, dim3(1), dim3(OT), 0, st, g);
    }
    return codlad_check_launch("codlad_pca_eigen");
}

extern "C" int codlad_pca_project(const double *D, const double *comps, int N, int d, int k, double *P, void *stream) {
    CODLAD_REQUIRE(D && comps && P, "null pointer");
    CODLAD_REQUIRE(N > 0 && N <= MAX_N && d > 0 && d <= MAX_D && k >= 1 && k <= MAX_K && k <= d,
                   "bad sizes (1 <= N <= CODLAD_PCA_MAX_N, d <= CODLAD_PCA_MAX_DIM, 1 <= k <= min(CODLAD_PCA_MAX_COMPONENTS, d))");
    hipLaunchKernelGGL(pca_project_kernel, dim3((unsigned)(((long long)N * k + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0,
                       (hipStream_t)stream, D, comps, N, d, k, P);
    return codlad_check_launch("codlad_pca_project");
}
