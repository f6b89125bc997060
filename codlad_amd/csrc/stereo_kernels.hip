// Stereochemistry check of generated structures (codlad_stereo_check, include/codlad_hip.h): the other half of the
// reference-free judgement beside geometry_kernels.hip.  Per residue of every structure the backbone and side-chain
// torsions (phi, psi, omega_in, chi1..chi4, degrees) and two signed volumes (v_ca at the alpha carbon, v_side at the beta
// carbon of THR / TPO / ILE), the decisions taken on them (inverted centre, cis / twisted peptide bond, undefined) and
// their counts per structure.  All structures share one topology: sites [n_res][9][4] names the four atoms of each of a
// residue's nine quantities, an entry with an index out of [0, n_atoms) is absent.
//
// One thread = one (structure, residue); 256 residues per workgroup, the workgroup index runs over the structures'
// residue blocks (structure-major, so any number of structures fits one launch).  A thread reads its 144-byte site row as
// nine 16-byte loads - the row is the same for every structure and stays in L2 - and gathers at most 36 atoms: 108
// independent loads, nothing depends on another quantity's result, so the memory pipe stays full with few waves.  No LDS
// beyond the six block counters, no scratch.
//
// Arithmetic: fp32, one rounding per operation (compiled with -ffp-contract=off), in the order written in torsion_deg()
// and volume() below and stated in the header; sqrtf and the division are the correctly rounded ones, atan2f is the
// device library's.
//
// Counts: every counter is a sum of 0 / 1 per thread, so a wave's share is the population count of a ballot; the waves of
// a workgroup add theirs in LDS and one integer atomic per counter and workgroup goes to the table the launch zeroed.
// Integers only: bit-identical from run to run, a structure's row independent of the other structures of the call.
#include <cmath>

#include "common.h"
#include "host_util.h"
#include "structure_math.h"

namespace {
constexpr int RES = 256;                     // residues (= threads) per workgroup
constexpr int N_Q = CODLAD_STEREO_COLUMNS;   // quantities per residue
constexpr int N_COUNTS = CODLAD_STEREO_COUNTS;
constexpr int COL_OMEGA = 2, COL_V_CA = 7, COL_V_SIDE = 8;
constexpr float DEG = 57.295779513082320877f;   // 180 / pi
constexpr float CIS_BELOW = 30.f, TWISTED_UPTO = 150.f;

// IUPAC torsion p0-p1-p2-p3 in degrees, in (-180, 180].  No angle exists where both arguments of atan2f are zero (two
// of the atoms coincide, three are exactly collinear) or one is not a number: NaN.
__device__ inline float torsion_deg(V3 p0, V3 p1, V3 p2, V3 p3) {
    const V3 b1 = sub(p1, p0), b2 = sub(p2, p1), b3 = sub(p3, p2);
    const V3 n1 = cross(b1, b2), n2 = cross(b2, b3);
    const float x = dot(n1, n2);
    const float y = dot(cross(n1, n2), b2) / sqrtf(dot(b2, b2));
    if (x == 0.f && y == 0.f) return quiet_nan();          // a NaN in either goes through atan2f
    const float deg = atan2f(y, x) * DEG;
    return deg == -180.f ? 180.f : deg;
}

// (p1 - p0) . ((p2 - p0) x (p3 - p0)), A^3
__device__ inline float volume(V3 p0, V3 p1, V3 p2, V3 p3) { return dot(sub(p1, p0), cross(sub(p2, p0), sub(p3, p0))); }

__device__ inline bool finite(float v) { return fabsf(v) < __uint_as_float(0x7f800000u); }

__global__ __launch_bounds__(RES) void stereo_check_kernel(const float *xyz, int n_atoms, int n_res, int res_blocks,
                                                           const int4 *sites, const uint8_t *res_kind, float *values,
                                                           uint8_t *flags, int32_t *counts) {
    __shared__ int red[N_COUNTS];
    const int s = blockIdx.x / res_blocks, r = (blockIdx.x % res_blocks) * RES + (int)threadIdx.x;
    const bool have = r < n_res;
    if (threadIdx.x < N_COUNTS) red[threadIdx.x] = 0;
    __syncthreads();

    unsigned flag = 0;
    bool pro = false;
    if (have) {
        const float *x = xyz + (size_t)s * n_atoms * 3;
        float *out = values + ((size_t)s * n_res + r) * N_Q;
        const int4 *row = sites + (size_t)r * N_Q;
        pro = res_kind[r] & CODLAD_STEREO_KIND_PRO;
        bool undefined = false;
        // every load before the first use: an absent quantity reads atom 0 four times instead (never the index it was
        // given) and is thrown away, so the 9 row loads and then the 108 coordinate loads are unconditional and all in
        // flight together - two dependent round trips per thread instead of eighteen
        int4 a[N_Q];
#pragma unroll
        for (int q = 0; q < N_Q; ++q) a[q] = row[q];
        bool exists[N_Q];
        V3 p[N_Q][4];
#pragma unroll
        for (int q = 0; q < N_Q; ++q) {
            const unsigned n = (unsigned)n_atoms;
            exists[q] = (unsigned)a[q].x < n && (unsigned)a[q].y < n && (unsigned)a[q].z < n && (unsigned)a[q].w < n;
            p[q][0] = load3(x, exists[q] ? a[q].x : 0), p[q][1] = load3(x, exists[q] ? a[q].y : 0);
            p[q][2] = load3(x, exists[q] ? a[q].z : 0), p[q][3] = load3(x, exists[q] ? a[q].w : 0);
        }
#pragma unroll
        for (int q = 0; q < N_Q; ++q) {
            const V3 p0 = p[q][0], p1 = p[q][1], p2 = p[q][2], p3 = p[q][3];
            float v = q < COL_V_CA ? torsion_deg(p0, p1, p2, p3) : volume(p0, p1, p2, p3);
            if (!exists[q]) v = quiet_nan();
            undefined |= exists[q] && !finite(v);
            if (q == COL_OMEGA) {
                const float w = fabsf(v);                           // NaN: neither comparison holds
                if (w < CIS_BELOW) flag |= CODLAD_STEREO_CIS;
                if (w >= CIS_BELOW && w <= TWISTED_UPTO) flag |= CODLAD_STEREO_TWISTED;
            }
            if (q == COL_V_CA && finite(v) && !(v > 0.f)) flag |= CODLAD_STEREO_INVERTED_CA;
            if (q == COL_V_SIDE && finite(v) && !(v > 0.f)) flag |= CODLAD_STEREO_INVERTED_SIDE;
            out[q] = v;
        }
        if (undefined) flag |= CODLAD_STEREO_UNDEFINED;
        flags[(size_t)s * n_res + r] = (uint8_t)flag;
    }

    // --- a wave's share of each counter is a population count; LDS integer adds across the waves, one atomic per counter
    const bool cis = flag & CODLAD_STEREO_CIS;
    const bool part[N_COUNTS] = {(flag & CODLAD_STEREO_INVERTED_CA) != 0, (flag & CODLAD_STEREO_INVERTED_SIDE) != 0,
                                 cis && pro, cis && !pro, (flag & CODLAD_STEREO_TWISTED) != 0,
                                 (flag & CODLAD_STEREO_UNDEFINED) != 0};
#pragma unroll
    for (int c = 0; c < N_COUNTS; ++c) {
        const int n = __popcll(__ballot(part[c]));
        if ((threadIdx.x & 63) == 0 && n) atomicAdd(&red[c], n);
    }
    __syncthreads();
    if (threadIdx.x < N_COUNTS && red[threadIdx.x]) atomicAdd(counts + (size_t)N_COUNTS * s + threadIdx.x, red[threadIdx.x]);
}
}  // namespace

extern "C" int codlad_stereo_check(const float *xyz, int n_struct, int n_atoms, const int32_t *sites,
                                   const uint8_t *res_kind, int n_res, float *values, uint8_t *flags, int32_t *counts,
                                   void *stream) {
    CODLAD_REQUIRE(xyz && sites && res_kind && values && flags && counts, "null pointer");
    CODLAD_REQUIRE(n_struct > 0 && n_res > 0 && n_atoms > 0, "bad counts");
    CODLAD_REQUIRE(((uintptr_t)sites & 15) == 0, "sites is not 16-byte aligned");
    const int64_t res_blocks = ((int64_t)n_res + RES - 1) / RES;
    CODLAD_REQUIRE(res_blocks * n_struct < (int64_t)1 << 31, "too many workgroups for one launch");
    hipStream_t st = (hipStream_t)stream;
    const hipError_t e = hipMemsetAsync(counts, 0, sizeof(int32_t) * N_COUNTS * (size_t)n_struct, st);
    if (e != hipSuccess) return codlad_hip_failed("codlad_stereo_check", e);
    hipLaunchKernelGGL(stereo_check_kernel, dim3((unsigned)(res_blocks * n_struct)), dim3(RES), 0, st, xyz, n_atoms, n_res,
                       (int)res_blocks, (const int4 *)sites, res_kind, values, flags, counts);
    return codlad_check_launch("codlad_stereo_check");
}
