// What the ensemble-analysis units (observables, saxs, saxs_hydration, pair_hist, reweight, cluster, pca, compare) share
// in FLOAT64 and in their REDUCTIONS, stated once: what NaN and "finite" mean for a double, the one order of a wave's and
// of a workgroup's sum, the lower-triangle tile walk and the chunks of structures of the two covariance products.  The
// fp32 three-vector helpers are structure_math.h's; ensemble_kernels.hip's block_sum<NV> is another tree (shuffle-down,
// its header states it) and stays there.  Every unit that includes this is compiled with -ffp-contract=off: one rounding
// per operation, in the order written here.
#pragma once
#include <hip/hip_runtime.h>

namespace {   // internal linkage, as each unit's own copy had
typedef double double4_t __attribute__((ext_vector_type(4)));   // the accumulator of v_mfma_f64_16x16x4_f64

__device__ inline double nan64() { return __longlong_as_double(0x7ff8000000000000ll); }
__device__ inline bool fin64(double x) { return fabs(x) < __longlong_as_double(0x7ff0000000000000ll); }
// a NaN on either side stays
__device__ inline double max_nan(double a, double b) { return (b > a || b != b) ? b : a; }

// A wave's 64 values (double, int, long long) by the xor butterfly, strides 32 .. 1: every lane gets the result.
template <typename T> __device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
    for (int st = 32; st > 0; st >>= 1) v += __shfl_xor(v, st);
    return v;
}
__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
    for (int st = 32; st > 0; st >>= 1) v = max_nan(v, __shfl_xor(v, st));
    return v;
}
// The workgroup's sum (any multiple of 64 threads up to 1024): the butterfly per wave, then the waves in ascending order
// from red[0] - ((w0 + w1) + w2) + .. - and every thread gets it.  red holds one T per wave.  There is no leading zero:
// waves that all hold -0.0 give -0.0 (a caller that wants +0.0 there writes 0.0 + block_sum(..)).
template <typename T> __device__ __forceinline__ T block_sum(T v, T *red) {
    v = wave_sum(v);
    __syncthreads();                                   // the previous use of red has been read
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    T s = red[0];
    for (int k = 1; k < (int)(blockDim.x >> 6); ++k) s += red[k];
    return s;
}
__device__ __forceinline__ double block_max(double v, double *red) {
    v = wave_max(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    double m = red[0];
    for (int k = 1; k < (int)(blockDim.x >> 6); ++k) m = max_nan(m, red[k]);
    return m;
}

// tile t of the lower triangle, row by row: t = I (I + 1) / 2 + J, J <= I
__device__ __forceinline__ void tri_tile_of(int t, int &I, int &J) {
    I = 0;
    while ((I + 1) * (I + 2) / 2 <= t) ++I;
    J = t - I * (I + 1) / 2;
}
// the tiles of the lower triangle of a d x d matrix (host)
inline int tri_tiles_of(int d, int tile) {
    const int T = (d + tile - 1) / tile;
    return T * (T + 1) / 2;
}

// The chunks of structures of a partial sum (host): at most 32 of about 512 rows, a multiple of 16 (the rows staged at a
// time), their number and size depending on N alone.  In long long: any int N.
struct Chunks {
    int nch, chunk;
};
inline Chunks chunks_of(int N) {
    constexpr long long MAX_CHUNKS = 32, CHUNK_ROWS = 512, STEP = 16;
    long long nch = (N + CHUNK_ROWS - 1) / CHUNK_ROWS;
    nch = nch > MAX_CHUNKS ? MAX_CHUNKS : nch;
    Chunks c;
    c.chunk = (int)(((N + nch - 1) / nch + STEP - 1) / STEP * STEP);
    c.nch = (int)(((long long)N + c.chunk - 1) / c.chunk);
    return c;
}
}  // namespace
