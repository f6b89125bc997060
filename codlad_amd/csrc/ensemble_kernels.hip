// Ensemble analysis after the path (stands in for md.rmsd in the reference's compute_div, test.py:37-95): the minimal
// RMSD of conformation a onto conformation b under a proper rotation plus translation, for many pairs per launch.
// fp32 coordinates are converted exactly; everything after that is fp64.  Centre first, then form the products - two
// passes over the atoms - because a one-pass formula on uncentred coordinates loses |centroid|^2 / spread^2 of its
// digits (a structure 1000 A from the origin: six of sixteen).
//   moments kernel : per conformation the centroid and G = sum |x - c|^2, once, so that the pairwise matrix does not
//                    recompute them G times
//   pair kernel    : per (a, b) the nine sums of S = sum (a - ca)(b - cb)^T, then one lane solves Horn's 4x4 by cyclic
//                    Jacobi (ensemble_math.h) -> msd, and R | t on request
//   pairwise kernel: one workgroup per (frame, member i) keeps conformation i in LDS and walks j > i
//   apply kernel   : out = R a + t in fp64, rounded once to fp32
// Every sum has ONE order, a function of the atom count alone: lane l of 256 adds atoms l, l + 256, ... in that order,
// a wave adds its 64 lanes by the shuffle tree 32, 16, .. 1, lane 0 adds the four waves 0..3.  No atomics.  So a replay
// is bit-identical and a pair's result depends neither on the other pairs of the launch nor on its place among them,
// and the pairwise kernel returns the pair kernel's bits.  Compiled with -ffp-contract=off: whether a product and an
// add fuse must not depend on the kernel the shared code was inlined into.
#include "common.h"
#include "ensemble_math.h"
#include "host_util.h"

namespace {
constexpr int BLOCK = 256;
constexpr int STAGE_ATOMS = 5376;      // conformation i of the pairwise kernel in LDS: 63 KB, the static limit less `part`

// Atom k of the (sub)set: row sel[k] of x when sel is given, else row k.  An index outside [0, n_atoms) reads nothing
// and poisons the result with NaN.
__device__ __forceinline__ void load_atom(const float *x, const int32_t *sel, int n_atoms, int k, double v[3]) {
    const int r = sel ? sel[k] : k;
    if ((unsigned)r >= (unsigned)n_atoms) {
        v[0] = v[1] = v[2] = __builtin_nan("");
        return;
    }
    v[0] = (double)x[3 * (size_t)r];
    v[1] = (double)x[3 * (size_t)r + 1];
    v[2] = (double)x[3 * (size_t)r + 2];
}

// The block's sum of NV per-lane values, in the one order described above; the result is valid in thread 0 (and
// returned to every thread through `wave_part`, which must hold 4 * NV doubles).
template <int NV>
__device__ __forceinline__ void block_sum(double v[NV], double *wave_part) {
#pragma unroll
    for (int k = 0; k < NV; ++k)
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v[k] += __shfl_down(v[k], off, 64);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __syncthreads();                                   // the previous use of wave_part has been read
    if (lane == 0)
#pragma unroll
        for (int k = 0; k < NV; ++k) wave_part[wave * NV + k] = v[k];
    __syncthreads();
#pragma unroll
    for (int k = 0; k < NV; ++k)
        v[k] = ((wave_part[k] + wave_part[NV + k]) + wave_part[2 * NV + k]) + wave_part[3 * NV + k];
}

__global__ __launch_bounds__(BLOCK) void ens_moments_kernel(const float *x, int n_atoms, const int32_t *sel, int m,
                                                            double *mom) {
    __shared__ double part[4 * 3];
    const float *xc = x + (size_t)blockIdx.x * n_atoms * 3;
    double s[3] = {0.0, 0.0, 0.0};
    for (int k = threadIdx.x; k < m; k += BLOCK) {
        double v[3];
        load_atom(xc, sel, n_atoms, k, v);
        s[0] += v[0]; s[1] += v[1]; s[2] += v[2];
    }
    block_sum<3>(s, part);
    const double c[3] = {s[0] / (double)m, s[1] / (double)m, s[2] / (double)m};
    double g[1] = {0.0};
    for (int k = threadIdx.x; k < m; k += BLOCK) {
        double v[3];
        load_atom(xc, sel, n_atoms, k, v);
        const double dx = v[0] - c[0], dy = v[1] - c[1], dz = v[2] - c[2];
        g[0] += (dx * dx + dy * dy) + dz * dz;
    }
    block_sum<1>(g, part);
    if (threadIdx.x == 0) {
        double *o = mom + 4 * (size_t)blockIdx.x;
        o[0] = c[0]; o[1] = c[1]; o[2] = c[2]; o[3] = g[0];
    }
}

// S of one pair.  a: conformation a's rows (global, gathered through sel_a) or its staged subset in LDS (sel_a null, na =
// m); b likewise from global.  Result valid in every thread.
__device__ __forceinline__ void pair_products(const float *a, const int32_t *sel_a, int na, const float *b,
                                              const int32_t *sel_b, int nb, int m, const double *ma, const double *mb,
                                              double *part, double S[9]) {
#pragma unroll
    for (int k = 0; k < 9; ++k) S[k] = 0.0;
    const double ca[3] = {ma[0], ma[1], ma[2]}, cb[3] = {mb[0], mb[1], mb[2]};
    for (int k = threadIdx.x; k < m; k += BLOCK) {
        double u[3], v[3];
        load_atom(a, sel_a, na, k, u);
        load_atom(b, sel_b, nb, k, v);
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            u[r] -= ca[r];
            v[r] -= cb[r];
        }
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = 0; c < 3; ++c) S[3 * r + c] += u[r] * v[c];
    }
    block_sum<9>(S, part);
}

__device__ __forceinline__ double finish(double msd, int squared) { return squared ? msd : sqrt(msd); }

__global__ __launch_bounds__(BLOCK) void ens_pair_kernel(const float *A, const double *momA, int nA, const float *B,
                                                         const double *momB, int nB, int n_atoms, const int32_t *sel,
                                                         int m, const int32_t *pairs, int squared, double *out,
                                                         double *Rt) {
    __shared__ double part[4 * 9];
    const int p = blockIdx.x;
    const int ia = pairs[2 * p], ib = pairs[2 * p + 1];
    if ((unsigned)ia >= (unsigned)nA || (unsigned)ib >= (unsigned)nB) {      // uniform over the block
        if (threadIdx.x == 0) {
            out[p] = __builtin_nan("");
            if (Rt)
                for (int k = 0; k < 12; ++k) Rt[12 * (size_t)p + k] = __builtin_nan("");
        }
        return;
    }
    const double *ma = momA + 4 * (size_t)ia, *mb = momB + 4 * (size_t)ib;
    double S[9];
    pair_products(A + (size_t)ia * n_atoms * 3, sel, n_atoms, B + (size_t)ib * n_atoms * 3, sel, n_atoms, m, ma, mb, part, S);
    if (threadIdx.x == 0)
        out[p] = finish(ens_solve_pair(S, ma[3], mb[3], ma, mb, (double)m, Rt ? Rt + 12 * (size_t)p : nullptr), squared);
}

// x [G][F][n_atoms][3]; out [F][G][G]: workgroup (f, i) writes the zero of the diagonal, row i right of it and column i
// below it (the mirror), so every element has exactly one writer.
__global__ __launch_bounds__(BLOCK) void ens_pairwise_kernel(const float *x, const double *mom, int G, int F, int n_atoms,
                                                             const int32_t *sel, int m, int squared, double *out) {
    __shared__ float stage[3 * STAGE_ATOMS];
    __shared__ double part[4 * 9];
    const int f = blockIdx.x % F, i = blockIdx.x / F;
    const size_t conf = (size_t)n_atoms * 3;
    const float *a = x + ((size_t)i * F + f) * conf;
    const int32_t *sel_a = sel;
    int na = n_atoms;
    if (m <= STAGE_ATOMS && i + 1 < G) {
        for (int k = threadIdx.x; k < m; k += BLOCK) {
            const int r = sel ? sel[k] : k;
            const bool ok = (unsigned)r < (unsigned)n_atoms;
#pragma unroll
            for (int c = 0; c < 3; ++c) stage[3 * k + c] = ok ? a[3 * (size_t)r + c] : __builtin_nanf("");
        }
        __syncthreads();
        a = stage;
        sel_a = nullptr;
        na = m;
    }
    double *o = out + (size_t)f * G * G;
    if (threadIdx.x == 0) o[(size_t)i * G + i] = 0.0;
    const double *ma = mom + 4 * ((size_t)i * F + f);
    for (int j = i + 1; j < G; ++j) {
        const double *mb = mom + 4 * ((size_t)j * F + f);
        double S[9];
        pair_products(a, sel_a, na, x + ((size_t)j * F + f) * conf, sel, n_atoms, m, ma, mb, part, S);
        if (threadIdx.x == 0) {
            const double v = finish(ens_solve_pair(S, ma[3], mb[3], ma, mb, (double)m, nullptr), squared);
            o[(size_t)i * G + j] = v;
            o[(size_t)j * G + i] = v;
        }
    }
}

// bx workgroups per conformation, each striding over its atoms
__global__ __launch_bounds__(BLOCK) void ens_apply_kernel(const float *x, const double *Rt, int n_atoms, int bx, float *out) {
    const int conf = blockIdx.x / bx, chunk = blockIdx.x % bx;
    const double *T = Rt + 12 * (size_t)conf;
    const size_t base = (size_t)conf * n_atoms * 3;
    for (int k = chunk * BLOCK + threadIdx.x; k < n_atoms; k += bx * BLOCK) {
        const double u = (double)x[base + 3 * (size_t)k], v = (double)x[base + 3 * (size_t)k + 1],
                     w = (double)x[base + 3 * (size_t)k + 2];
#pragma unroll
        for (int r = 0; r < 3; ++r)
            out[base + 3 * (size_t)k + r] = (float)((((T[3 * r] * u + T[3 * r + 1] * v) + T[3 * r + 2] * w)) + T[9 + r]);
    }
}

// The atoms summed over: n_sel of sel, or all n_atoms when sel is null.  -1: inconsistent.
constexpr int MAX_GRID = 0x7fffffff;
}  // namespace

extern "C" int codlad_ens_moments(const float *x, int n_conf, int n_atoms, const int32_t *sel, int n_sel, double *mom,
                                  void *stream) {
    CODLAD_REQUIRE(x && mom, "null pointer");
    CODLAD_REQUIRE(n_conf > 0 && n_atoms > 0 && n_sel >= 0, "bad sizes");
    const int m = subset_size(sel, n_sel, n_atoms);
    CODLAD_REQUIRE(m > 0, "sel and n_sel disagree (sel with n_sel > 0, or neither)");
    hipLaunchKernelGGL(ens_moments_kernel, dim3(n_conf), dim3(BLOCK), 0, (hipStream_t)stream, x, n_atoms, sel, m, mom);
    return codlad_check_launch("codlad_ens_moments");
}

extern "C" int codlad_ens_pair_msd(const float *A, const double *momA, int nA, const float *B, const double *momB, int nB,
                                   int n_atoms, const int32_t *sel, int n_sel, const int32_t *pairs, int n_pairs,
                                   int squared, double *out, double *Rt, void *stream) {
    CODLAD_REQUIRE(A && momA && B && momB && pairs && out, "null pointer");
    CODLAD_REQUIRE(nA > 0 && nB > 0 && n_atoms > 0 && n_sel >= 0 && n_pairs > 0, "bad sizes");
    const int m = subset_size(sel, n_sel, n_atoms);
    CODLAD_REQUIRE(m > 0, "sel and n_sel disagree (sel with n_sel > 0, or neither)");
    hipLaunchKernelGGL(ens_pair_kernel, dim3(n_pairs), dim3(BLOCK), 0, (hipStream_t)stream, A, momA, nA, B, momB, nB,
                       n_atoms, sel, m, pairs, squared != 0, out, Rt);
    return codlad_check_launch("codlad_ens_pair_msd");
}

extern "C" int codlad_ens_apply(const float *x, const double *Rt, int n_conf, int n_atoms, float *out, void *stream) {
    CODLAD_REQUIRE(x && Rt && out, "null pointer");
    CODLAD_REQUIRE(n_conf > 0 && n_atoms > 0, "bad sizes");
    int bx = (n_atoms + BLOCK - 1) / BLOCK;
    bx = bx > 16 ? 16 : bx;
    CODLAD_REQUIRE((long long)n_conf * bx <= MAX_GRID, "too many conformations for one call");
    hipLaunchKernelGGL(ens_apply_kernel, dim3(n_conf * bx), dim3(BLOCK), 0, (hipStream_t)stream, x, Rt, n_atoms, bx, out);
    return codlad_check_launch("codlad_ens_apply");
}

extern "C" int codlad_ens_pairwise(const float *x, const double *mom, int G, int F, int n_atoms, const int32_t *sel,
                                   int n_sel, int squared, double *out, void *stream) {
    CODLAD_REQUIRE(x && mom && out, "null pointer");
    CODLAD_REQUIRE(G > 0 && F > 0 && n_atoms > 0 && n_sel >= 0 && (long long)G * F <= MAX_GRID, "bad sizes");
    const int m = subset_size(sel, n_sel, n_atoms);
    CODLAD_REQUIRE(m > 0, "sel and n_sel disagree (sel with n_sel > 0, or neither)");
    hipLaunchKernelGGL(ens_pairwise_kernel, dim3(G * F), dim3(BLOCK), 0, (hipStream_t)stream, x, mom, G, F, n_atoms, sel, m,
                       squared != 0, out);
    return codlad_check_launch("codlad_ens_pairwise");
}
