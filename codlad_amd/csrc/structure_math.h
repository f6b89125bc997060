// What the structure-analysis units (geometry, stereo, relax, observables, dssp, saxs, saxs_hydration, pair_hist, compare,
// lddt) share on the DEVICE in fp32, stated once: the three-vector helpers and the squared distance in the one expression
// order every "float32 restatement" of the tests repeats, the non-finite test with the kernel that applies it to a whole
// structure, the clamp of a table's index and the search of a flagged exclusion row.  The float64 and reduction pieces are
// reduce_math.h's.  No MFMA code, nothing of the denoiser (that is common.h).  Every unit that includes this is compiled
// with -ffp-contract=off: one rounding per operation, in the order written here.
#pragma once
#include <hip/hip_runtime.h>
#include "../../include/codlad_hip.h"

namespace {   // internal linkage, as each unit's own copy had
constexpr uint32_t INF_BITS = 0x7f800000u;

struct V3 { float x, y, z; };

__device__ inline V3 load3(const float *x, int a) { return {x[3 * a], x[3 * a + 1], x[3 * a + 2]}; }
__device__ inline V3 sub(V3 a, V3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ inline V3 cross(V3 a, V3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
__device__ inline float dot(V3 a, V3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
__device__ inline float dist2(float xi, float yi, float zi, float xj, float yj, float zj) {
    const float dx = xi - xj, dy = yi - yj, dz = zi - zj;
    return (dx * dx + dy * dy) + dz * dz;
}
__device__ inline float quiet_nan() { return __uint_as_float(0x7fc00000u); }
// NaN or +-inf: the exponent bits are all set
__device__ inline bool non_finite(float v) { return (__float_as_uint(v) & INF_BITS) == INF_BITS; }
// an index read from a table, into [lo, hi] (lo <= hi at every call): a wrong table reads wrongly, inside the buffers
__device__ inline int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }

// One workgroup of THREADS per structure: finite[s] = none of its n3 = 3 n coordinates is NaN or +-inf.
template <int THREADS> __global__ __launch_bounds__(THREADS) void finite_kernel(const float *xyz, int n3, uint8_t *finite) {
    const float *x = xyz + (size_t)blockIdx.x * n3;
    int bad = 0;
    for (int k = threadIdx.x; k < n3; k += THREADS) bad |= non_finite(x[k]);
    bad = __syncthreads_or(bad);
    if (threadIdx.x == 0) finite[blockIdx.x] = bad ? 0 : 1;
}

// is j among the partners of the CSR row [lo, hi) (sorted by partner index, flag bit ignored)?
__device__ inline bool excluded(const int32_t *excl, int lo, int hi, int j) {
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        const int p = excl[mid] & ~CODLAD_GEOM_BOND_FLAG;
        if (p == j) return true;
        if (p < j) lo = mid + 1; else hi = mid;
    }
    return false;
}
}  // namespace
