// Ensemble observables of generated structures (codlad_sasa, codlad_contact_counts; include/codlad_hip.h): what a user of
// a backmapped ensemble computes after the single-structure checks - solvent-accessible surface area per atom / residue /
// structure (Shrake-Rupley) and the contact counts of an atom selection over the structures of a call.  The radius of
// gyration needs no kernel: it is sqrt(G / m) of codlad_ens_moments.
//
// SASA, three launches on the caller's stream:
//   finite_kernel   structure_math.h's: one workgroup per structure, is any coordinate NaN or +-inf (an integer test on
//                   the bit pattern)
//   sasa_kernel     one WAVE per atom i.  Lane l owns the sphere points l, l + 64, ... (at most 16) as R_i * u_k in
//                   registers and one alive bit per point.  The structure's atoms are walked in chunks of 64, one candidate
//                   j per lane: the lane forms x_j - x_i and the conservative overlap test, the wave ballots, and a
//                   wave-uniform loop over the set bits reads the neighbour's difference vector and R_j^2 from its lane
//                   (v_readlane) and clears the points it buries.  No neighbour list, so no capacity: a collapsed structure
//                   with hundreds of neighbours takes the same path.  The chunk loop ends early when no lane has a live
//                   point.  exposed = the wave's sum of the lanes' population counts: integers, no atomics.
//   sasa_sum_kernel the float64 sums: res_area per (structure, residue) by one thread in index order, total per structure
//                   by one workgroup in the fixed order the header states.  The residue table is a HOST table (it is
//                   validated before any launch) and reaches the device in the kernel arguments, RES_CHUNK residues a launch.
// Every decision is `fl32 < fl32` on values whose order of operations the header fixes (-ffp-contract=off: one rounding
// per operation), every count an integer, every sum in one order: results are bit-identical from call to call, and a
// structure's results depend on nothing but its own coordinates and the tables.
//
// The pre-filter skips atom j only when d2 > (R_i + R_j)^2 * (1 + 2^-10): a point of i lies within R_i (1 + 2^-23) of x_i,
// so j can bury one only if d < R_i + R_j up to a few 2^-24 relative, and fp32 rounding of d2 and of the threshold is three
// orders of magnitude inside the 2^-10 slack.  The filter therefore never changes a decision; a NaN d2 compares false and
// is not skipped.
//
// Contacts: one thread per pair (a, b) of a 16 x 16 tile of the selection, a loop over the structures; tiles below the
// diagonal do nothing, the others write (a, b) and (b, a), the diagonal 0: every element is written exactly once.
#include "common.h"
#include "reduce_math.h"
#include "structure_math.h"

namespace {
constexpr int WAVE = 64;
constexpr int WAVES = 4;                     // atoms per workgroup of sasa_kernel
constexpr int SUM_THREADS = 256;
constexpr int RES_CHUNK = 512;               // residue boundaries per launch: 2 KiB of kernel arguments
constexpr int TILE = 16;
constexpr float SLACK = 1.0f + 0x1p-10f;

__device__ inline float lane_read(float v, int lane) {
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane));
}

// T = points per lane (the smallest of 1, 2, 4, 8, 16 that covers n_points): the point arrays stay in registers
template <int T>
__global__ __launch_bounds__(WAVE * WAVES) void sasa_kernel(const float *xyz, int n, int blocks, const float *radius,
                                                             const float *unit_area, const float *dirs, int n_points,
                                                             const uint8_t *finite, int32_t *exposed, float *atom_area) {
    const int s = blockIdx.x / blocks, lane = threadIdx.x & (WAVE - 1);
    const int i = (blockIdx.x % blocks) * WAVES + (int)(threadIdx.x / WAVE);          // wave-uniform
    if (i >= n) return;
    const size_t row = (size_t)s * n;
    if (!finite[s]) {
        if (lane == 0) {
            exposed[row + i] = -1;
            atom_area[row + i] = __uint_as_float(0x7fc00000u);
        }
        return;
    }
    const float *x = xyz + row * 3;
    const float xi = x[3 * i], yi = x[3 * i + 1], zi = x[3 * i + 2], ri = radius[i];
    float px[T], py[T], pz[T];
    uint32_t alive = 0;
#pragma unroll
    for (int t = 0; t < T; ++t) {
        const int k = lane + WAVE * t;
        const bool have = k < n_points;
        px[t] = have ? ri * dirs[3 * k] : 0.f;
        py[t] = have ? ri * dirs[3 * k + 1] : 0.f;
        pz[t] = have ? ri * dirs[3 * k + 2] : 0.f;
        alive |= (uint32_t)have << t;
    }
    for (int c0 = 0; c0 < n; c0 += WAVE) {
        const int j = c0 + lane;
        const bool have = j < n;
        float dx = 0.f, dy = 0.f, dz = 0.f, rj = 0.f;
        if (have) dx = x[3 * j] - xi, dy = x[3 * j + 1] - yi, dz = x[3 * j + 2] - zi, rj = radius[j];
        const float d2 = (dx * dx + dy * dy) + dz * dz, sum = ri + rj;
        const float rj2 = rj * rj;
        unsigned long long near = __ballot(have && j != i && !(d2 > (sum * sum) * SLACK));
        while (near) {
            const int b = __builtin_ctzll(near);
            near &= near - 1;
            const float bx = lane_read(dx, b), by = lane_read(dy, b), bz = lane_read(dz, b), br2 = lane_read(rj2, b);
#pragma unroll
            for (int t = 0; t < T; ++t) {
                const float ex = px[t] - bx, ey = py[t] - by, ez = pz[t] - bz;
                const bool buried = (ex * ex + ey * ey) + ez * ez < br2;
                alive &= ~((uint32_t)buried << t);
            }
        }
        if (!__any(alive != 0)) break;
    }
    const int count = wave_sum((int)__popc(alive));
    if (lane == 0) {
        exposed[row + i] = count;
        atom_area[row + i] = (float)count * unit_area[i];
    }
}

struct ResChunk { int32_t ptr[RES_CHUNK + 1]; };

// blocks [0, res_blocks): one thread per (structure, residue of this chunk); then, if with_total, one block per structure
__global__ __launch_bounds__(SUM_THREADS) void sasa_sum_kernel(const float *atom_area, int n, int n_struct, const uint8_t *finite,
                                                               ResChunk res, int res0, int res_count, int n_res,
                                                               int res_blocks, float *res_area, double *total) {
    const double nan = nan64();
    if ((int)blockIdx.x < res_blocks) {
        const int k = blockIdx.x * SUM_THREADS + threadIdx.x;
        if (k >= n_struct * res_count) return;
        const int s = k / res_count, r = k % res_count;
        const float *a = atom_area + (size_t)s * n;
        double sum = 0.0;
        for (int q = res.ptr[r]; q < res.ptr[r + 1]; ++q) sum += (double)a[q];
        res_area[(size_t)s * n_res + res0 + r] = finite[s] ? (float)sum : (float)nan;
        return;
    }
    __shared__ double part[SUM_THREADS];
    const int s = blockIdx.x - res_blocks;
    const float *a = atom_area + (size_t)s * n;
    double sum = 0.0;
    for (int q = threadIdx.x; q < n; q += SUM_THREADS) sum += (double)a[q];
    part[threadIdx.x] = sum;
    __syncthreads();
    for (int st = SUM_THREADS / 2; st > 0; st >>= 1) {
        if ((int)threadIdx.x < st) part[threadIdx.x] += part[threadIdx.x + st];
        __syncthreads();
    }
    if (threadIdx.x == 0) total[s] = finite[s] ? part[0] : nan;
}

__global__ __launch_bounds__(TILE * TILE) void contact_kernel(const float *xyz, int n_struct, int n, const int32_t *sel, int m,
                                                              float cut2, int32_t *counts) {
    if (blockIdx.y > blockIdx.x) return;                      // x = the column tile: the upper triangle
    const int a = blockIdx.y * TILE + threadIdx.y, b = blockIdx.x * TILE + threadIdx.x;
    if (a >= m || b >= m || a > b) return;
    if (a == b) {
        counts[(size_t)a * m + a] = 0;
        return;
    }
    const int ia = sel ? sel[a] : a, ib = sel ? sel[b] : b;
    int count = 0;
    if ((unsigned)ia < (unsigned)n && (unsigned)ib < (unsigned)n) {
        const float *pa = xyz + 3 * (size_t)ia, *pb = xyz + 3 * (size_t)ib;
        for (int s = 0; s < n_struct; ++s, pa += 3 * (size_t)n, pb += 3 * (size_t)n) {
            const float dx = pa[0] - pb[0], dy = pa[1] - pb[1], dz = pa[2] - pb[2];
            count += (dx * dx + dy * dy) + dz * dz < cut2;
        }
    }
    counts[(size_t)a * m + b] = count;
    counts[(size_t)b * m + a] = count;
}

template <int T>
void launch_sasa(hipStream_t st, unsigned grid, const float *xyz, int n, int blocks, const float *radius, const float *unit_area,
                 const float *dirs, int n_points, const uint8_t *finite, int32_t *exposed, float *atom_area) {
    hipLaunchKernelGGL(sasa_kernel<T>, dim3(grid), dim3(WAVE * WAVES), 0, st, xyz, n, blocks, radius, unit_area, dirs, n_points,
                       finite, exposed, atom_area);
}
}  // namespace

extern "C" int codlad_sasa(const float *xyz, int n_struct, int n_atoms, const float *radius, const float *unit_area,
                           const float *dirs, int n_points, const int32_t *res_ptr, int n_res, int32_t *exposed,
                           float *atom_area, float *res_area, double *total, uint8_t *finite, void *stream) {
    CODLAD_REQUIRE(xyz && radius && unit_area && dirs && exposed && atom_area && total && finite, "null pointer");
    CODLAD_REQUIRE(n_struct > 0 && n_atoms > 0, "bad counts");
    CODLAD_REQUIRE(n_points >= 1 && n_points <= CODLAD_SASA_MAX_POINTS, "n_points outside 1 .. 1024");
    CODLAD_REQUIRE(n_res >= 0 && (n_res > 0) == (res_ptr != nullptr) && (n_res > 0) == (res_area != nullptr),
                   "res_ptr, n_res and res_area go together");
    for (int r = 0; r < n_res; ++r)
        CODLAD_REQUIRE(res_ptr[r] >= 0 && res_ptr[r] <= res_ptr[r + 1] && res_ptr[r + 1] <= n_atoms,
                       "res_ptr is not a non-decreasing table into [0, n_atoms]");
    const int64_t blocks = ((int64_t)n_atoms + WAVES - 1) / WAVES;
    CODLAD_REQUIRE(blocks * n_struct < (int64_t)1 << 31 && (int64_t)n_atoms * 3 < (int64_t)1 << 31 &&
                   (int64_t)n_struct * RES_CHUNK < (int64_t)1 << 31, "too many workgroups for one launch");
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(finite_kernel<SUM_THREADS>, dim3((unsigned)n_struct), dim3(SUM_THREADS), 0, st, xyz, n_atoms * 3, finite);
    int rc = codlad_check_launch("codlad_sasa");
    if (rc) return rc;
    const unsigned grid = (unsigned)(blocks * n_struct);
    const int per_lane = (n_points + WAVE - 1) / WAVE;
#define CODLAD_SASA_ARGS st, grid, xyz, n_atoms, (int)blocks, radius, unit_area, dirs, n_points, finite, exposed, atom_area
    if (per_lane <= 1) launch_sasa<1>(CODLAD_SASA_ARGS);
    else if (per_lane <= 2) launch_sasa<2>(CODLAD_SASA_ARGS);
    else if (per_lane <= 4) launch_sasa<4>(CODLAD_SASA_ARGS);
    else if (per_lane <= 8) launch_sasa<8>(CODLAD_SASA_ARGS);
    else launch_sasa<16>(CODLAD_SASA_ARGS);
#undef CODLAD_SASA_ARGS
    rc = codlad_check_launch("codlad_sasa");
    if (rc) return rc;
    // the total rides with the first launch of the sums (the only one when there are no residues)
    int r0 = 0;
    do {
        ResChunk chunk = {};
        const int count = n_res - r0 < RES_CHUNK ? n_res - r0 : RES_CHUNK;
        for (int r = 0; r <= count && count; ++r) chunk.ptr[r] = res_ptr[r0 + r];
        const int res_blocks = (int)(((int64_t)n_struct * count + SUM_THREADS - 1) / SUM_THREADS);
        hipLaunchKernelGGL(sasa_sum_kernel, dim3((unsigned)(res_blocks + (r0 == 0 ? n_struct : 0))), dim3(SUM_THREADS), 0, st,
                           atom_area, n_atoms, n_struct, finite, chunk, r0, count, n_res, res_blocks, res_area, total);
        rc = codlad_check_launch("codlad_sasa");
        if (rc) return rc;
        r0 += RES_CHUNK;
    } while (r0 < n_res);
    return 0;
}

extern "C" int codlad_contact_counts(const float *xyz, int n_struct, int n_atoms, const int32_t *sel, int n_sel, float cut2,
                                     int32_t *counts, void *stream) {
    CODLAD_REQUIRE(xyz && counts, "null pointer");
    CODLAD_REQUIRE(n_struct > 0 && n_atoms > 0, "bad counts");
    CODLAD_REQUIRE(n_sel >= 0 && (n_sel > 0) == (sel != nullptr), "sel and n_sel go together");
    CODLAD_REQUIRE(cut2 >= 0.f, "cut2 is negative or not a number");
    const int m = n_sel ? n_sel : n_atoms;
    const int tiles = (m + TILE - 1) / TILE;
    CODLAD_REQUIRE(tiles <= 65535, "more than 65535 x 16 atoms in the map");
    hipLaunchKernelGGL(contact_kernel, dim3((unsigned)tiles, (unsigned)tiles), dim3(TILE, TILE), 0, (hipStream_t)stream, xyz,
                       n_struct, n_atoms, sel, m, cut2, counts);
    return codlad_check_launch("codlad_contact_counts");
}
