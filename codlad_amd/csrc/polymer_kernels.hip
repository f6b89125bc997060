// Chain statistics of disordered ensembles (codlad_chain_sums, codlad_gyration; include/codlad_hip.h): per structure and
// per sequence separation s the sums of r^2 and of 1 / r over the pairs (k, k + s) of an ordered atom selection - what
// the hydrodynamic radius (Kirkwood's double sum) and the internal distance scaling R(s) are made of - and the gyration
// tensor with its eigenvalues and the end-to-end distance.
//
// Per pair, float64 from the fp32 coordinates (polymer_math.h), i = k the lower chain position, j = k + s:
//   dx = (double)x_j - (double)x_i per component, r2 = (dx*dx + dy*dy) + dz*dz, r = sqrt(r2), inv = 1.0 / r
// -ffp-contract=off: one rounding per operation; sqrt and the division are the correctly rounded ones.
//
// codlad_chain_sums, two launches on the caller's stream:
//   chain_sums_kernel    grid (N, chunks), 256 lanes.  Every workgroup stages the m selected atoms of its structure in
//                        LDS, component-major (12 m bytes: 51 KB at m = 4325, 96 KB at the limit), and finds `finite`
//                        on the way.  The unit of work is the PAIR of separations (u, m - u), u = 1 .. m / 2: m - u
//                        terms of the first and u of the second, m terms in all whatever u is, so the units are equal
//                        shares (m even: the last unit is m / 2 alone).  A unit belongs to ONE wave: wave w of chunk c
//                        takes the units 1 + 4 c + w, then every 4 * chunks-th.  The wave walks the unit's m terms
//                        t = lane, lane + 64, ..: t < m - u is term k = t of separation u, the others are term
//                        k = t - (m - u) of separation m - u.  A lane keeps one partial per separation and per sum and
//                        adds its terms in ascending k; the wave adds the 64 partials by the xor butterfly 32 .. 1
//                        (reduce_math.h) and lane 0 writes the element.
//   chain_finish_kernel  one wave per structure: inv_sum = ((0 + sep_inv[1]) + sep_inv[2]) + .., s ascending, the
//                        values read 64 at a time and added by lane-broadcast in one chain.
// The order of every sum is a function of m and s alone: not of N, not of the number of chunks (which only says WHICH
// wave owns a unit), not of the structure's place in the batch.  Every output element has one writer; no atomics of
// any kind, no scratch memory.  chunks = 1 unless N < CODLAD_POLYMER_SPLIT_MAX_N and m >= CODLAD_POLYMER_SPLIT_MIN_SEL;
// then as many as bring the grid to TARGET_GROUPS workgroups, four units per workgroup at least.
//
// codlad_gyration: one wave per structure.  Lane l adds the atoms l, l + 64, .. in that order, six products of
// (double)x - c per atom with c the centroid of codlad_ens_moments; the butterfly; one correctly rounded division by m;
// the eigenvalues by cyclic Jacobi (polymer_math.h), computed alike by every lane.
#include "common.h"
#include "host_util.h"
#include "polymer_math.h"
#include "reduce_math.h"
#include "structure_math.h"

namespace {
constexpr int WAVE = 64;
constexpr int THREADS = 256;
constexpr int WAVES = THREADS / WAVE;
constexpr int TARGET_GROUPS = 1024;                    // workgroups that fill the device: 4 per compute unit

// lane l's double, in every lane (l is uniform)
__device__ __forceinline__ double read_lane(double v, int l) {
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), l), hi = __builtin_amdgcn_readlane(__double2hiint(v), l);
    return __hiloint2double(hi, lo);
}

// dynamic LDS: 3 m floats
__global__ __launch_bounds__(THREADS) void chain_sums_kernel(const float *x, int n_atoms, const int32_t *sel, int m,
                                                             double *sep_r2, double *sep_inv, uint8_t *finite) {
    extern __shared__ float lds[];
    float *cx = lds, *cy = cx + m, *cz = cy + m;
    const float *xs = x + (size_t)blockIdx.x * n_atoms * 3;
    int bad = 0;
    for (int k = threadIdx.x; k < m; k += THREADS) {
        const size_t a = sel ? clampi(sel[k], 0, n_atoms - 1) : k;
        const float vx = xs[3 * a], vy = xs[3 * a + 1], vz = xs[3 * a + 2];
        bad |= non_finite(vx) | non_finite(vy) | non_finite(vz);
        cx[k] = vx, cy[k] = vy, cz[k] = vz;
    }
    bad = __syncthreads_or(bad);                                  // and the staged atoms are there
    if (blockIdx.y == 0 && threadIdx.x == 0) finite[blockIdx.x] = bad ? 0 : 1;
    double *row2 = sep_r2 + (size_t)blockIdx.x * (m - 1), *rowi = sep_inv + (size_t)blockIdx.x * (m - 1);
    const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
    for (int u = 1 + blockIdx.y * WAVES + wave; u <= m / 2; u += gridDim.y * WAVES) {     // uniform in the wave
        const int sa = u, sb = m - u, na = m - u;                 // separation sa has na terms, sb has u
        const int total = sb > sa ? m : na;                       // m even, u = m / 2: one separation
        double a2 = 0.0, ai = 0.0, b2 = 0.0, bi = 0.0;
        if (bad) {
            a2 = ai = b2 = bi = nan64();
        } else {
            for (int t = lane; t < total; t += WAVE) {
                const bool first = t < na;
                const int k = first ? t : t - na, j = k + (first ? sa : sb);
                const double r2 = poly_dist2(cx[k], cy[k], cz[k], cx[j], cy[j], cz[j]);
                const double inv = 1.0 / sqrt(r2);
                if (first) a2 += r2, ai += inv;
                else b2 += r2, bi += inv;
            }
            a2 = wave_sum(a2), ai = wave_sum(ai), b2 = wave_sum(b2), bi = wave_sum(bi);
        }
        if (lane == 0) {
            row2[sa - 1] = a2, rowi[sa - 1] = ai;
            if (sb > sa) row2[sb - 1] = b2, rowi[sb - 1] = bi;
        }
    }
}

__global__ __launch_bounds__(WAVE) void chain_finish_kernel(const double *sep_inv, int m, const uint8_t *finite,
                                                            double *inv_sum) {
    const double *row = sep_inv + (size_t)blockIdx.x * (m - 1);
    double s = 0.0;
    for (int k0 = 0; k0 < m - 1; k0 += WAVE) {
        const int k = k0 + threadIdx.x;
        const double v = k < m - 1 ? row[k] : 0.0;
#pragma unroll
        for (int l = 0; l < WAVE; ++l)
            if (k0 + l < m - 1) s += read_lane(v, l);             // uniform
    }
    if (threadIdx.x == 0) inv_sum[blockIdx.x] = finite[blockIdx.x] ? s : nan64();
}

__global__ __launch_bounds__(WAVE) void gyration_kernel(const float *x, int n_atoms, const int32_t *sel, int m,
                                                        const double *mom, double *tensor, double *eig, double *ree,
                                                        uint8_t *finite) {
    const float *xs = x + (size_t)blockIdx.x * n_atoms * 3;
    const double *c = mom + 4 * (size_t)blockIdx.x;
    const double c0 = c[0], c1 = c[1], c2 = c[2];
    double t[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    int bad = 0;
    for (int k = threadIdx.x; k < m; k += WAVE) {
        const size_t a = sel ? clampi(sel[k], 0, n_atoms - 1) : k;
        const float vx = xs[3 * a], vy = xs[3 * a + 1], vz = xs[3 * a + 2];
        bad |= non_finite(vx) | non_finite(vy) | non_finite(vz);
        const double dx = (double)vx - c0, dy = (double)vy - c1, dz = (double)vz - c2;
        t[0] += dx * dx, t[1] += dy * dy, t[2] += dz * dz;
        t[3] += dx * dy, t[4] += dx * dz, t[5] += dy * dz;
    }
    bad = __syncthreads_or(bad);
    const double dm = (double)m;
#pragma unroll
    for (int i = 0; i < 6; ++i) t[i] = bad ? nan64() : wave_sum(t[i]) / dm;
    double e[3] = {t[0], t[0], t[0]};                             // NaN when bad (uniform): no sweep is spent on it
    if (!bad) poly_eigenvalues(t, e);
    if (threadIdx.x == 0) {
        const size_t a = sel ? clampi(sel[0], 0, n_atoms - 1) : 0, b = sel ? clampi(sel[m - 1], 0, n_atoms - 1) : m - 1;
        const double r = sqrt(poly_dist2(xs[3 * a], xs[3 * a + 1], xs[3 * a + 2], xs[3 * b], xs[3 * b + 1], xs[3 * b + 2]));
        double *to = tensor + 6 * (size_t)blockIdx.x, *eo = eig + 3 * (size_t)blockIdx.x;
#pragma unroll
        for (int i = 0; i < 6; ++i) to[i] = t[i];
#pragma unroll
        for (int i = 0; i < 3; ++i) eo[i] = e[i];
        ree[blockIdx.x] = bad ? nan64() : r;
        finite[blockIdx.x] = bad ? 0 : 1;
    }
}

// workgroups per structure of chain_sums_kernel: a function of N and m alone
int chunks_of(int N, int m) {
    if (N >= CODLAD_POLYMER_SPLIT_MAX_N || m < CODLAD_POLYMER_SPLIT_MIN_SEL) return 1;
    const int by_units = (m / 2 + WAVES - 1) / WAVES, by_grid = (TARGET_GROUPS + N - 1) / N;
    return by_units < by_grid ? by_units : by_grid;
}
}  // namespace

extern "C" int codlad_chain_sums_groups(int N, int m) {
    CODLAD_REQUIRE(N >= 1, "N < 1");
    CODLAD_REQUIRE(m >= 2 && m <= CODLAD_POLYMER_MAX_SEL, "m outside 2 .. 8192");
    return chunks_of(N, m);
}

extern "C" int codlad_chain_sums(const float *x, int N, int n_atoms, const int32_t *sel, int n_sel, double *sep_r2,
                                 double *sep_inv, double *inv_sum, uint8_t *finite, void *stream) {
    CODLAD_REQUIRE(x && sep_r2 && sep_inv && inv_sum && finite, "null pointer");
    CODLAD_REQUIRE(N >= 1 && n_atoms >= 1 && n_sel >= 0, "bad counts");
    CODLAD_REQUIRE((sel != nullptr) == (n_sel > 0), "sel and n_sel disagree");
    const int m = sel ? n_sel : n_atoms;
    CODLAD_REQUIRE(m >= 2 && m <= CODLAD_POLYMER_MAX_SEL, "m outside 2 .. 8192");
    const char *what = "codlad_chain_sums";
    hipStream_t st = (hipStream_t)stream;
    static bool attr_set = false;
    if (!attr_set) {
        set_max_lds(reinterpret_cast<const void *>(chain_sums_kernel), (size_t)CODLAD_POLYMER_MAX_SEL * 12);
        attr_set = true;
    }
    hipLaunchKernelGGL(chain_sums_kernel, dim3((unsigned)N, (unsigned)chunks_of(N, m)), dim3(THREADS), (size_t)m * 12, st, x,
                       n_atoms, sel, m, sep_r2, sep_inv, finite);
    const int rc = codlad_check_launch(what);
    if (rc) return rc;
    hipLaunchKernelGGL(chain_finish_kernel, dim3((unsigned)N), dim3(WAVE), 0, st, sep_inv, m, finite, inv_sum);
    return codlad_check_launch(what);
}

extern "C" int codlad_gyration(const float *x, int N, int n_atoms, const int32_t *sel, int n_sel, const double *mom,
                               double *tensor, double *eig, double *ree, uint8_t *finite, void *stream) {
    CODLAD_REQUIRE(x && mom && tensor && eig && ree && finite, "null pointer");
    CODLAD_REQUIRE(N >= 1 && n_atoms >= 1 && n_sel >= 0, "bad counts");
    CODLAD_REQUIRE((sel != nullptr) == (n_sel > 0), "sel and n_sel disagree");
    const int m = sel ? n_sel : n_atoms;
    CODLAD_REQUIRE(m <= CODLAD_POLYMER_MAX_SEL, "m outside 1 .. 8192");
    hipLaunchKernelGGL(gyration_kernel, dim3((unsigned)N), dim3(WAVE), 0, (hipStream_t)stream, x, n_atoms, sel, m, mom, tensor,
                       eig, ree, finite);
    return codlad_check_launch("codlad_gyration");
}
