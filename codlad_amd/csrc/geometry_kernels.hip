// Reference-free geometry check of generated structures (codlad_geometry_check, include/codlad_hip.h): every structure
// of a batch is judged against the TEMPLATE topology all of them share - is its covalent graph (pairs closer than
// (r_i + r_j) * scale, the criterion of bond_graph_kernel) the template's bond graph, and do atoms that are more than
// `order` bonds apart overlap.  An all-pairs pass per structure over the upper triangle i < j.
//
// One workgroup = one structure x one block of ROWS rows; a thread owns one row atom in registers and walks the columns,
// which are staged through LDS in tiles of COLS atoms as float4 {x, y, z, radius}: all lanes read the same LDS address
// (a broadcast), so any n_atoms works with 16 KiB of LDS.  Tiles left of the row block are skipped.
//
// The exclusion list (pairs within `order` bonds) is NOT consulted per pair: near_dist (9 A) is no rare event.  The pair
// pass counts ALL pairs under each threshold, and a second pass over the row's own CSR partners (a dozen per atom, local
// in index) takes the excluded ones off again - integer arithmetic, so the difference is exact.  Only the minimum needs
// the list per pair, and only when a pair undercuts the thread's running minimum (a binary search of the row, rare after
// the first few columns).  Template bonds are walked as a list for the broken count; the intact ones are the order-1
// partners under the cut-off, so spurious = bonded - intact, and bonded == n_bonds - broken + spurious ties the bond list
// to the flags of the CSR.
//
// Counts are integer atomics (one per block and counter) and the minimum is a signed integer atomicMin on the bit pattern
// of a non-negative float: both are order-independent, so results are bit-identical from run to run and a structure's row
// does not depend on the other structures of the call.
//
// Non-finite coordinates: every comparison with a NaN distance is false, so such a pair is in no count except `broken`,
// which is !(d < cut) - the complement of `intact`, so bonded == n_bonds - broken + spurious holds for any bits.  A row
// atom with a coordinate that is NaN or +-inf puts NAN_BITS into the minimum instead of a distance: a NaN whose bit
// pattern is a negative integer, so it wins the signed atomicMin against every distance in any order.  min_dist of such a
// structure is NaN, which is what metrics.geometry_check's `valid` reads.
// Compiled with -ffp-contract=off: distances round as bond_graph_kernel's and metrics_partial_kernel's do.
#include "common.h"
#include "host_util.h"
#include "structure_math.h"

namespace {
constexpr int ROWS = 256;        // rows per workgroup = threads per workgroup
constexpr int COLS = 1024;       // atoms per LDS column tile
constexpr float EPS = 1e-7f;     // as metrics_partial_kernel (reference test.py:27)
constexpr int32_t BOND_FLAG = CODLAD_GEOM_BOND_FLAG;
constexpr int N_COUNTS = 5;
constexpr uint32_t NAN_BITS = 0xffc00000u;   // a quiet NaN, negative as an int32

struct Cuts { float scale, clash, near; };

// sqrtf(d2 + EPS) < clash: sqrtf(d2 + EPS) >= sqrtf(d2) (both roundings are monotonic), so d < clash is necessary and
// the second root is taken for the few pairs that pass it
__device__ inline bool is_clash(float d2, float d, float clash) { return d < clash && sqrtf(d2 + EPS) < clash; }

__global__ __launch_bounds__(ROWS) void geometry_check_kernel(const float *xyz, int n, int row_blocks, const float *radius,
                                                              const int32_t *excl_ptr, const int32_t *excl,
                                                              const int32_t *bonds, int n_bonds, Cuts cut,
                                                              int32_t *counts, uint32_t *min_bits) {
    __shared__ float4 tile[COLS];
    __shared__ int red[ROWS];
    const int s = blockIdx.x / row_blocks, rb = blockIdx.x % row_blocks;
    const float *x = xyz + (size_t)s * n * 3;
    const int row0 = rb * ROWS, i = row0 + (int)threadIdx.x;
    const bool have = i < n;
    float xi = 0.f, yi = 0.f, zi = 0.f, ri = 0.f;
    int e_lo = 0, e_hi = 0;
    if (have) {
        xi = x[3 * i], yi = x[3 * i + 1], zi = x[3 * i + 2], ri = radius[i];
        e_lo = excl_ptr[i], e_hi = excl_ptr[i + 1];
    }
    int broken = 0, bonded = 0, intact = 0, near = 0, clash = 0;
    float dmin = __uint_as_float(INF_BITS);

    // --- all pairs i < j, column tiles from the one that holds row0 + 1
    for (int c0 = ((row0 + 1) / COLS) * COLS; c0 < n; c0 += COLS) {
        const int width = min(COLS, n - c0);
        __syncthreads();                                  // the previous tile has been read
        for (int k = threadIdx.x; k < width; k += ROWS) {
            const int j = c0 + k;
            tile[k] = make_float4(x[3 * j], x[3 * j + 1], x[3 * j + 2], radius[j]);
        }
        __syncthreads();
        if (!have) continue;
        for (int k = max(row0 + 1 - c0, 0); k < width; ++k) {        // the bound is the block's: no divergence in the trip
            const float4 a = tile[k];
            const int j = c0 + k;
            if (j <= i) continue;
            const float d2 = dist2(xi, yi, zi, a.x, a.y, a.z);
            const float d = sqrtf(d2);
            bonded += d < (ri + a.w) * cut.scale;
            near += d <= cut.near;
            clash += is_clash(d2, d, cut.clash);
            if (d < dmin && !excluded(excl, e_lo, e_hi, j)) dmin = d;
        }
    }

    // --- the row's partners within `order` bonds (j > i): taken off near / clash; the order-1 ones that hold are intact
    for (int e = e_lo; e < e_hi; ++e) {
        const int word = excl[e], j = word & ~BOND_FLAG;
        if (j <= i || j >= n) continue;
        const float d2 = dist2(xi, yi, zi, x[3 * j], x[3 * j + 1], x[3 * j + 2]);
        const float d = sqrtf(d2);
        near -= d <= cut.near;
        clash -= is_clash(d2, d, cut.clash);
        if (word & BOND_FLAG) intact += d < (ri + radius[j]) * cut.scale;
    }

    // --- template bonds, dealt to the row blocks of the structure
    for (int b = row0 + (int)threadIdx.x; b < n_bonds; b += row_blocks * ROWS) {
        const int p = bonds[2 * b], q = bonds[2 * b + 1];
        if ((unsigned)p >= (unsigned)n || (unsigned)q >= (unsigned)n) continue;
        const float d = sqrtf(dist2(x[3 * p], x[3 * p + 1], x[3 * p + 2], x[3 * q], x[3 * q + 1], x[3 * q + 2]));
        broken += !(d < (radius[p] + radius[q]) * cut.scale);
    }

    // --- block sums, then one integer atomic per counter
    const int part[N_COUNTS] = {broken, bonded - intact, bonded, near, clash};
    for (int c = 0; c < N_COUNTS; ++c) {
        __syncthreads();
        red[threadIdx.x] = part[c];
        __syncthreads();
        for (int st = ROWS / 2; st > 0; st >>= 1) {
            if ((int)threadIdx.x < st) red[threadIdx.x] += red[threadIdx.x + st];
            __syncthreads();
        }
        if (threadIdx.x == 0 && red[0]) atomicAdd(counts + N_COUNTS * s + c, red[0]);
    }
    __syncthreads();
    // d >= 0: the bit patterns order as the values do, as signed integers too, and NAN_BITS lies below all of them
    red[threadIdx.x] = (int)((non_finite(xi) || non_finite(yi) || non_finite(zi)) ? NAN_BITS : __float_as_uint(dmin));
    __syncthreads();
    for (int st = ROWS / 2; st > 0; st >>= 1) {
        if ((int)threadIdx.x < st) red[threadIdx.x] = min(red[threadIdx.x], red[threadIdx.x + st]);
        __syncthreads();
    }
    if (threadIdx.x == 0 && red[0] < (int)INF_BITS) atomicMin(reinterpret_cast<int *>(min_bits) + s, red[0]);
}
}  // namespace

extern "C" int codlad_geometry_check(const float *xyz, int n_struct, int n_atoms, const float *radius,
                                     const int32_t *excl_ptr, const int32_t *excl, const int32_t *bonds, int n_bonds,
                                     float scale, float clash_dist, float near_dist, int32_t *counts, float *min_dist,
                                     void *stream) {
    CODLAD_REQUIRE(xyz && radius && excl_ptr && counts && min_dist, "null pointer");
    CODLAD_REQUIRE(n_struct > 0 && n_atoms > 0 && n_atoms < BOND_FLAG && n_bonds >= 0, "bad counts");
    CODLAD_REQUIRE(n_bonds == 0 || bonds, "a non-empty bond list has a null pointer");
    CODLAD_REQUIRE(scale > 0.f && clash_dist >= 0.f && near_dist >= 0.f, "bad thresholds");
    const int64_t row_blocks = ((int64_t)n_atoms + ROWS - 1) / ROWS;
    CODLAD_REQUIRE(row_blocks * n_struct < (int64_t)1 << 31, "too many workgroups for one launch");
    // every pair counter of a structure fits an int32
    CODLAD_REQUIRE((int64_t)n_atoms * (n_atoms - 1) / 2 < (int64_t)1 << 31, "n_atoms too large for int32 pair counts");
    hipStream_t st = (hipStream_t)stream;
    hipError_t e = hipMemsetAsync(counts, 0, sizeof(int32_t) * N_COUNTS * (size_t)n_struct, st);
    if (e == hipSuccess) e = hipMemsetD32Async((hipDeviceptr_t)min_dist, (int)INF_BITS, (size_t)n_struct, st);
    if (e != hipSuccess) return codlad_hip_failed("codlad_geometry_check", e);
    const Cuts cut = {scale, clash_dist, near_dist};
    hipLaunchKernelGGL(geometry_check_kernel, dim3((unsigned)(row_blocks * n_struct)), dim3(ROWS), 0, st, xyz, n_atoms,
                       (int)row_blocks, radius, excl_ptr, excl, bonds, n_bonds, cut, counts, (uint32_t *)min_dist);
    return codlad_check_launch("codlad_geometry_check");
}
