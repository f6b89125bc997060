// Restrained clash relaxation of generated structures (codlad_relax, codlad_relax_energy, include/codlad_hip.h): the step
// after geometry_kernels.hip and stereo_kernels.hip have flagged a structure.  Per structure an energy of three terms -
// harmonic restraints on every pair within two bonds to its distance in the START structure, periodic restraints on the
// torsions about rigid bonds to their START values, and a one-sided harmonic repulsion between atoms more than `order`
// bonds apart that are closer than (r_i + r_j) * contact_scale - is minimised by steepest descent with a step that grows
// by 1.2 on an accepted trial and halves on a rejected one.  All structures share ONE topology.
//
// Evaluation (relax_eval_kernel, the ONE kernel behind both entry points): rows and column tiles as
// geometry_check_kernel - one workgroup = one structure x one block of ROWS atoms, a thread owns atom i in registers and
// walks ALL atoms j in ascending order (the full matrix, not the triangle), staged through LDS in tiles of COLS float4
// {x, y, z, radius}.  The thread gathers its own force: no floating-point atomics anywhere.  The exclusion row is searched
// only for pairs that pass d < sigma (rare).  Then the thread walks its row of the pair-restraint CSR and its row of the
// quad CSR; a quad's gradient is recomputed by each of its four atoms, which keeps its own share.  A term's energy is
// counted by ONE of its atoms (the lower index of a pair, the first atom of a quad).
// Energy: fp32 terms, added in float64 - per thread, then a fixed tree per workgroup into that workgroup's own slot of
// `partials`; the slots of a structure are added in ascending order by whoever reads them.  gmax: an integer atomicMax on
// the bit pattern of a non-negative float.  Both are order-independent, so results are bit-identical from run to run and
// a structure does not depend on its batch mates.
//
// Loop: iterations are separated by kernel boundaries on the caller's stream, two launches each - relax_eval_kernel on the
// trial positions, then relax_step_kernel, in which EVERY workgroup of a structure re-derives the accept / reject decision
// from the partials and the state of the previous iteration (read at index t - 1, written at index t by one workgroup: no
// race), moves its own atoms' accepted state and forms their next trial x' = x - fl32(h / gmax) * g: one multiply and one
// subtract (compiled with -ffp-contract=off).  No host synchronisation, no grid-wide barrier, no cooperative launch.
#include "common.h"
#include "host_util.h"
#include "structure_math.h"

namespace {
constexpr int ROWS = 256;        // rows per workgroup = threads per workgroup
constexpr int COLS = 1024;       // atoms per LDS column tile
constexpr float EPS = 1e-7f;     // as metrics_partial_kernel: d = sqrtf(d2 + EPS), coincident atoms have a gradient
constexpr int32_t BOND_FLAG = CODLAD_GEOM_BOND_FLAG;
constexpr float MIN_SIN = 0.1f;  // a quad with a flatter bond angle in the start structure has weight 0

struct Tables {
    const float *radius;
    const uint8_t *fixed;
    const int32_t *excl_ptr, *excl, *pair_ptr, *pair_j, *quads, *quad_ptr, *quad_ref;
    int n, n_pairs, n_quads, n_refs;
};
struct Consts { float k_r, k_t, k_c, contact_scale; };

__device__ inline bool quad_in_range(int4 q, int n) {
    return (unsigned)q.x < (unsigned)n && (unsigned)q.y < (unsigned)n && (unsigned)q.z < (unsigned)n && (unsigned)q.w < (unsigned)n;
}

// The torsion p0-p1-p2-p3 as (cos, sin) = (x, y) / |(x, y)| with x = n1 . n2, y = |b2| b1 . n2 (IUPAC sign; no atan2f).
struct Torsion { V3 b1, b2, b3, n1, n2; float c, s, lb2; };
__device__ inline Torsion torsion(V3 p0, V3 p1, V3 p2, V3 p3) {
    Torsion t;
    t.b1 = sub(p1, p0), t.b2 = sub(p2, p1), t.b3 = sub(p3, p2);
    t.n1 = cross(t.b1, t.b2), t.n2 = cross(t.b2, t.b3);
    t.lb2 = sqrtf(dot(t.b2, t.b2));
    const float x = dot(t.n1, t.n2), y = t.lb2 * dot(t.b1, t.n2);
    const float r = sqrtf(x * x + y * y);
    t.c = x / r, t.s = y / r;
    return t;
}

// Start-structure constants: d0 [n_struct][n_pairs] per CSR entry, q0 [n_struct][n_quads][3] = {cos phi0, sin phi0, weight}.
__global__ __launch_bounds__(ROWS) void relax_prep_kernel(const float *xyz0, Tables T, int row_blocks, float *d0, float *q0) {
    const int s = blockIdx.x / row_blocks, rb = blockIdx.x % row_blocks;
    const float *x = xyz0 + (size_t)s * T.n * 3;
    const int i = rb * ROWS + (int)threadIdx.x;
    if (i < T.n) {
        const V3 pi = load3(x, i);
        const int lo = max(T.pair_ptr[i], 0), hi = min(T.pair_ptr[i + 1], T.n_pairs);
        for (int e = lo; e < hi; ++e) {
            const int j = T.pair_j[e] & ~BOND_FLAG;
            float d = 0.f;
            if ((unsigned)j < (unsigned)T.n) {
                const V3 r = sub(pi, load3(x, j));
                d = sqrtf(dot(r, r) + EPS);
            }
            d0[(size_t)s * T.n_pairs + e] = d;
        }
    }
    for (int q = i; q < T.n_quads; q += row_blocks * ROWS) {
        const int4 a = ((const int4 *)T.quads)[q];
        float c = 1.f, sn = 0.f, w = 0.f;
        if (quad_in_range(a, T.n)) {
            const Torsion t = torsion(load3(x, a.x), load3(x, a.y), load3(x, a.z), load3(x, a.w));
            // |sin| of the two bond angles: |b1 x b2| / (|b1| |b2|) and |b2 x b3| / (|b2| |b3|)
            const float s1 = sqrtf(dot(t.n1, t.n1)) / (sqrtf(dot(t.b1, t.b1)) * t.lb2);
            const float s2 = sqrtf(dot(t.n2, t.n2)) / (t.lb2 * sqrtf(dot(t.b3, t.b3)));
            if (s1 >= MIN_SIN && s2 >= MIN_SIN) c = t.c, sn = t.s, w = 1.f;        // a NaN fails both comparisons
        }
        float *o = q0 + ((size_t)s * T.n_quads + q) * 3;
        o[0] = c, o[1] = sn, o[2] = w;
    }
}

// Energy and gradient of one structure's block of ROWS atoms: the function every evaluation of both entry points runs.
// partial [3] (the workgroup's slot), grad [n][3] of the structure (fixed atoms: 0), gmax_bits: the structure's word.
__device__ inline void relax_eval_block(const float *x, const Tables &T, Consts k, const float *d0, const float *q0, int rb,
                                        double *partial, float *grad, uint32_t *gmax_bits) {
    __shared__ float4 tile[COLS];
    __shared__ double red[ROWS];
    __shared__ uint32_t gred[ROWS];
    const int n = T.n, row0 = rb * ROWS, i = row0 + (int)threadIdx.x;
    const bool have = i < n;
    float xi = 0.f, yi = 0.f, zi = 0.f, ri = 0.f;
    int e_lo = 0, e_hi = 0;
    if (have) {
        xi = x[3 * i], yi = x[3 * i + 1], zi = x[3 * i + 2], ri = T.radius[i];
        e_lo = T.excl_ptr[i], e_hi = T.excl_ptr[i + 1];
    }
    double e_r = 0.0, e_t = 0.0, e_c = 0.0;
    float gx = 0.f, gy = 0.f, gz = 0.f;

    // --- repulsion: all j in ascending order
    const float two_kc = 2.f * k.k_c;
    for (int c0 = 0; c0 < n; c0 += COLS) {
        const int width = min(COLS, n - c0);
        __syncthreads();                                  // the previous tile has been read
        for (int kk = threadIdx.x; kk < width; kk += ROWS) {
            const int j = c0 + kk;
            tile[kk] = make_float4(x[3 * j], x[3 * j + 1], x[3 * j + 2], T.radius[j]);
        }
        __syncthreads();
        if (!have) continue;
        for (int kk = 0; kk < width; ++kk) {
            const float4 a = tile[kk];
            const float dx = xi - a.x, dy = yi - a.y, dz = zi - a.z;
            const float d2 = (dx * dx + dy * dy) + dz * dz;
            const float sig = (ri + a.w) * k.contact_scale;
            // d < sig needs d2 <= sig^2 (1 + a few ulp): the root is taken for the few pairs that pass the wider test
            if (d2 <= sig * sig * 1.0001f) {
                const int j = c0 + kk;
                const float d = sqrtf(d2 + EPS);
                if (j != i && d < sig && !excluded(T.excl, e_lo, e_hi, j)) {
                    const float t = sig - d;
                    if (j > i) e_c += (double)(k.k_c * (t * t));
                    const float coef = (two_kc * t) / d;
                    gx -= coef * dx, gy -= coef * dy, gz -= coef * dz;
                }
            }
        }
    }

    if (have) {
        // --- distance restraints: the row's partners within two bonds
        const float two_kr = 2.f * k.k_r;
        const int lo = max(T.pair_ptr[i], 0), hi = min(T.pair_ptr[i + 1], T.n_pairs);
        for (int e = lo; e < hi; ++e) {
            const int j = T.pair_j[e] & ~BOND_FLAG;
            if ((unsigned)j >= (unsigned)n) continue;
            const float dx = xi - x[3 * j], dy = yi - x[3 * j + 1], dz = zi - x[3 * j + 2];
            const float d = sqrtf(((dx * dx + dy * dy) + dz * dz) + EPS);
            const float t = d - d0[e];
            if (j > i) e_r += (double)(k.k_r * (t * t));
            const float coef = (two_kr * t) / d;
            gx += coef * dx, gy += coef * dy, gz += coef * dz;
        }
        // --- torsion restraints: the quads this atom is part of; ref = 4 * quad + position
        const int q_lo = max(T.quad_ptr[i], 0), q_hi = min(T.quad_ptr[i + 1], T.n_refs);
        for (int r = q_lo; r < q_hi; ++r) {
            const int ref = T.quad_ref[r], q = ref >> 2, pos = ref & 3;
            if ((unsigned)q >= (unsigned)T.n_quads) continue;
            const float c0 = q0[3 * q], s0 = q0[3 * q + 1], w = q0[3 * q + 2];
            if (w == 0.f) continue;
            const int4 a = ((const int4 *)T.quads)[q];
            const Torsion t = torsion(load3(x, a.x), load3(x, a.y), load3(x, a.z), load3(x, a.w));
            const float kw = k.k_t * w;
            // 1 - cos(phi - phi0) as half the squared chord of the two unit vectors: exactly 0 at the start structure, and no
            // cancellation near it
            const float dc = t.c - c0, ds = t.s - s0;
            if (pos == 0) e_t += (double)(kw * (0.5f * (dc * dc + ds * ds)));
            const float de = kw * (t.s * c0 - t.c * s0);                     // dE / dphi
            const float bb = dot(t.b2, t.b2);
            const float f0 = -t.lb2 / dot(t.n1, t.n1), f3 = t.lb2 / dot(t.n2, t.n2);   // dphi/dp0 = f0 n1, dphi/dp3 = f3 n2
            const float u = dot(t.b1, t.b2) / bb, v = dot(t.b3, t.b2) / bb;
            float a1, a2;                                                     // dphi/dp[pos] = a1 n1 + a2 n2
            if (pos == 0) a1 = f0, a2 = 0.f;
            else if (pos == 1) a1 = -f0 - u * f0, a2 = v * f3;
            else if (pos == 2) a1 = u * f0, a2 = -f3 - v * f3;
            else a1 = 0.f, a2 = f3;
            gx += de * (a1 * t.n1.x + a2 * t.n2.x), gy += de * (a1 * t.n1.y + a2 * t.n2.y), gz += de * (a1 * t.n1.z + a2 * t.n2.z);
        }
        if (T.fixed[i]) gx = gy = gz = 0.f;
        grad[3 * i] = gx, grad[3 * i + 1] = gy, grad[3 * i + 2] = gz;
    }

    // --- the workgroup's energies: a fixed tree in float64, into the workgroup's own slot
    const double part[3] = {e_r, e_t, e_c};
    for (int c = 0; c < 3; ++c) {
        __syncthreads();
        red[threadIdx.x] = part[c];
        __syncthreads();
        for (int st = ROWS / 2; st > 0; st >>= 1) {
            if ((int)threadIdx.x < st) red[threadIdx.x] += red[threadIdx.x + st];
            __syncthreads();
        }
        if (threadIdx.x == 0) partial[c] = red[0];
    }
    // --- gmax: |g| >= 0, the bit patterns order as the values do
    gred[threadIdx.x] = __float_as_uint(fmaxf(fmaxf(fabsf(gx), fabsf(gy)), fabsf(gz)));
    __syncthreads();
    for (int st = ROWS / 2; st > 0; st >>= 1) {
        if ((int)threadIdx.x < st) gred[threadIdx.x] = max(gred[threadIdx.x], gred[threadIdx.x + st]);
        __syncthreads();
    }
    if (threadIdx.x == 0 && gred[0]) atomicMax(gmax_bits, gred[0]);
}

// gmax_bits + s * gmax_stride: the word of structure s this evaluation raises (zeroed by the host before the launch)
__global__ __launch_bounds__(ROWS) void relax_eval_kernel(const float *xyz, Tables T, Consts k, int row_blocks, const float *d0,
                                                          const float *q0, double *partials, float *grad, uint32_t *gmax_bits,
                                                          int gmax_stride) {
    const int s = blockIdx.x / row_blocks, rb = blockIdx.x % row_blocks;
    relax_eval_block(xyz + (size_t)s * T.n * 3, T, k, d0 + (size_t)s * T.n_pairs, q0 + (size_t)s * T.n_quads * 3, rb,
                     partials + ((size_t)s * row_blocks + rb) * 3, grad + (size_t)s * T.n * 3,
                     gmax_bits + (size_t)s * gmax_stride);
}

// the three energies of a structure: its workgroups' slots in ascending order
__device__ inline void sum_partials(const double *partials, int row_blocks, double e[3]) {
    e[0] = e[1] = e[2] = 0.0;
    for (int rb = 0; rb < row_blocks; ++rb)
        for (int c = 0; c < 3; ++c) e[c] += partials[3 * rb + c];
}

__global__ void relax_finish_kernel(const double *partials, int row_blocks, int n_struct, double *energy) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n_struct) return;
    double e[3];
    sum_partials(partials + (size_t)s * row_blocks * 3, row_blocks, e);
    for (int c = 0; c < 3; ++c) energy[3 * s + c] = e[c];
}

struct Trace {
    double *energy, *trial_energy;
    float *step, *gmax;
    uint8_t *accepted, *converged;
};

// Call t = 0 .. n_iter, after evaluation t (0: the input in xa -> ga; t >= 1: the trial of iteration t - 1 in xt -> gt).
// Decides iteration t - 1, records it, moves the accepted state and forms the trial of iteration t.  hst / gacc / gtrial
// [n_struct][n_iter + 1]: the step, the accepted state's gmax and the evaluation's gmax per index.
__global__ __launch_bounds__(ROWS) void relax_step_kernel(int t, int n_iter, int n, int row_blocks, const double *partials,
                                                          float *xa, float *ga, float *xt, const float *gt, float *hst,
                                                          float *gacc, const uint32_t *gtrial, Trace tr, float h0, float h_max) {
    __shared__ double e_sh;
    const int s = blockIdx.x / row_blocks, rb = blockIdx.x % row_blocks;
    const size_t row = (size_t)s * (n_iter + 1);
    if (threadIdx.x == 0) {
        double e[3];
        sum_partials(partials + (size_t)s * row_blocks * 3, row_blocks, e);
        e_sh = (e[0] + e[1]) + e[2];
    }
    __syncthreads();
    const double e_new = e_sh;
    const float g_new = __uint_as_float(gtrial[row + t]);
    double energy = e_new;
    float h = h0, gm = g_new;
    bool accept = false;
    if (t > 0) {
        const double e_old = tr.energy[row + t - 1];
        const float h_old = hst[row + t - 1];
        accept = e_new < e_old;
        energy = accept ? e_new : e_old;
        h = accept ? fminf(h_old * 1.2f, h_max) : h_old * 0.5f;
        gm = accept ? g_new : gacc[row + t - 1];
    }
    if (rb == 0 && threadIdx.x == 0) {
        tr.energy[row + t] = energy;
        hst[row + t] = h;
        gacc[row + t] = gm;
        if (t > 0) {
            tr.trial_energy[(size_t)s * n_iter + t - 1] = e_new;
            tr.accepted[(size_t)s * n_iter + t - 1] = accept;
        }
        if (t < n_iter) {
            tr.step[(size_t)s * n_iter + t] = h;
            tr.gmax[(size_t)s * n_iter + t] = gm;
        } else {
            tr.converged[s] = gm == 0.f;
        }
    }
    const int i = rb * ROWS + (int)threadIdx.x;
    if (i >= n) return;
    const size_t o = ((size_t)s * n + i) * 3;
    if (accept)
        for (int c = 0; c < 3; ++c) xa[o + c] = xt[o + c], ga[o + c] = gt[o + c];
    if (t < n_iter) {
        // gmax == 0 (nothing pushes: converged) or not a number: the trial IS the state, and is rejected as E' == E
        const bool move = gm > 0.f;
        const float scale = move ? h / gm : 0.f;
        for (int c = 0; c < 3; ++c) xt[o + c] = move ? xa[o + c] - scale * ga[o + c] : xa[o + c];
    }
}


struct Scratch {
    size_t partials, d0, q0, xt, ga, gt, hst, gacc, gtrial, total;
};

// n_iter < 0: the single evaluation (no loop state)
Scratch scratch_layout(int64_t S, int64_t n, int64_t n_pairs, int64_t n_quads, int64_t n_iter) {
    const int64_t row_blocks = (n + ROWS - 1) / ROWS;
    Scratch L = {};
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t at = off; off += align256(bytes); return at; };
    L.partials = take(sizeof(double) * 3 * S * row_blocks);
    L.d0 = take(sizeof(float) * S * n_pairs);
    L.q0 = take(sizeof(float) * 3 * S * n_quads);
    if (n_iter >= 0) {
        L.xt = take(sizeof(float) * 3 * S * n);
        L.ga = take(sizeof(float) * 3 * S * n);
        L.gt = take(sizeof(float) * 3 * S * n);
        L.hst = take(sizeof(float) * S * (n_iter + 1));
        L.gacc = take(sizeof(float) * S * (n_iter + 1));
        L.gtrial = take(sizeof(uint32_t) * S * (n_iter + 1));
    }
    L.total = off;
    return L;
}
}  // namespace

#define RELAX_CHECK_COMMON()                                                                                               \
    CODLAD_REQUIRE(xyz && radius && fixed && excl_ptr && pair_ptr && quad_ptr && scratch, "null pointer");                 \
    CODLAD_REQUIRE(n_struct > 0 && n_atoms > 0 && n_atoms < BOND_FLAG && n_pairs >= 0 && n_quads >= 0 && n_refs >= 0,      \
                   "bad counts");                                                                                          \
    CODLAD_REQUIRE(n_pairs == 0 || pair_j, "a non-empty pair list has a null pointer");                                    \
    CODLAD_REQUIRE(n_quads == 0 || quads, "a non-empty quad list has a null pointer");                                     \
    CODLAD_REQUIRE(n_refs == 0 || (quad_ref && n_quads > 0), "a non-empty quad reference list has no quads");              \
    CODLAD_REQUIRE(((uintptr_t)quads & 15) == 0, "quads is not 16-byte aligned");                                          \
    CODLAD_REQUIRE(((uintptr_t)scratch & 7) == 0, "scratch is not 8-byte aligned");                                        \
    CODLAD_REQUIRE(k_r > 0.f && k_t > 0.f && k_c > 0.f, "the force constants must be positive");                           \
    CODLAD_REQUIRE(contact_scale > 0.f, "contact_scale must be positive");                                                 \
    const int64_t row_blocks = ((int64_t)n_atoms + ROWS - 1) / ROWS;                                                       \
    CODLAD_REQUIRE(row_blocks * n_struct < (int64_t)1 << 31, "too many workgroups for one launch");                        \
    CODLAD_REQUIRE((int64_t)n_atoms * (n_atoms - 1) / 2 < (int64_t)1 << 31, "n_atoms too large")

extern "C" long long codlad_relax_scratch_bytes(int n_struct, int n_atoms, int n_pairs, int n_quads, int n_iter) {
    if (n_struct <= 0 || n_atoms <= 0 || n_pairs < 0 || n_quads < 0) return -1;
    return (long long)scratch_layout(n_struct, n_atoms, n_pairs, n_quads, n_iter).total;
}

extern "C" int codlad_relax_energy(const float *xyz, const float *xyz0, int n_struct, int n_atoms, const float *radius,
                                   const uint8_t *fixed, const int32_t *excl_ptr, const int32_t *excl,
                                   const int32_t *pair_ptr, const int32_t *pair_j, int n_pairs, const int32_t *quads,
                                   int n_quads, const int32_t *quad_ptr, const int32_t *quad_ref, int n_refs, float k_r,
                                   float k_t, float k_c, float contact_scale, double *energy, float *grad, float *gmax,
                                   void *scratch, void *stream) {
    RELAX_CHECK_COMMON();
    CODLAD_REQUIRE(xyz0 && energy && grad && gmax, "null pointer");
    const Scratch L = scratch_layout(n_struct, n_atoms, n_pairs, n_quads, -1);
    char *base = (char *)scratch;
    double *partials = (double *)(base + L.partials);
    float *d0 = (float *)(base + L.d0), *q0 = (float *)(base + L.q0);
    const Tables T = {radius, fixed, excl_ptr, excl, pair_ptr, pair_j, quads, quad_ptr, quad_ref, n_atoms, n_pairs, n_quads, n_refs};
    const Consts k = {k_r, k_t, k_c, contact_scale};
    hipStream_t st = (hipStream_t)stream;
    const hipError_t e = hipMemsetAsync(gmax, 0, sizeof(float) * (size_t)n_struct, st);
    if (e != hipSuccess) return codlad_hip_failed("codlad_relax_energy", e);
    const dim3 grid((unsigned)(row_blocks * n_struct));
    hipLaunchKernelGGL(relax_prep_kernel, grid, dim3(ROWS), 0, st, xyz0, T, (int)row_blocks, d0, q0);
    hipLaunchKernelGGL(relax_eval_kernel, grid, dim3(ROWS), 0, st, xyz, T, k, (int)row_blocks, d0, q0, partials, grad,
                       (uint32_t *)gmax, 1);
    hipLaunchKernelGGL(relax_finish_kernel, dim3((unsigned)((n_struct + 63) / 64)), dim3(64), 0, st, partials, (int)row_blocks,
                       n_struct, energy);
    return codlad_check_launch("codlad_relax_energy");
}

extern "C" int codlad_relax(const float *xyz, int n_struct, int n_atoms, const float *radius, const uint8_t *fixed,
                            const int32_t *excl_ptr, const int32_t *excl, const int32_t *pair_ptr, const int32_t *pair_j,
                            int n_pairs, const int32_t *quads, int n_quads, const int32_t *quad_ptr, const int32_t *quad_ref,
                            int n_refs, float k_r, float k_t, float k_c, float contact_scale, float h0, float h_max,
                            int n_iter, float *xyz_out, double *trace_energy, double *trace_trial_energy, float *trace_step,
                            uint8_t *trace_accepted, float *trace_gmax, uint8_t *converged, void *scratch, void *stream) {
    RELAX_CHECK_COMMON();
    CODLAD_REQUIRE(xyz_out && trace_energy && converged, "null pointer");
    CODLAD_REQUIRE(n_iter >= 0 && n_iter < 1 << 24, "n_iter must be in [0, 2^24)");
    CODLAD_REQUIRE(n_iter == 0 || (trace_trial_energy && trace_step && trace_accepted && trace_gmax), "null trace pointer");
    CODLAD_REQUIRE(h0 > 0.f && h_max > 0.f, "the step lengths must be positive");
    CODLAD_REQUIRE(xyz_out != xyz, "xyz_out must not be xyz");
    const Scratch L = scratch_layout(n_struct, n_atoms, n_pairs, n_quads, n_iter);
    char *base = (char *)scratch;
    double *partials = (double *)(base + L.partials);
    float *d0 = (float *)(base + L.d0), *q0 = (float *)(base + L.q0);
    float *xa = xyz_out, *xt = (float *)(base + L.xt), *ga = (float *)(base + L.ga), *gt = (float *)(base + L.gt);
    float *hst = (float *)(base + L.hst), *gacc = (float *)(base + L.gacc);
    uint32_t *gtrial = (uint32_t *)(base + L.gtrial);
    const Tables T = {radius, fixed, excl_ptr, excl, pair_ptr, pair_j, quads, quad_ptr, quad_ref, n_atoms, n_pairs, n_quads, n_refs};
    const Consts k = {k_r, k_t, k_c, contact_scale};
    const Trace tr = {trace_energy, trace_trial_energy, trace_step, trace_gmax, trace_accepted, converged};
    hipStream_t st = (hipStream_t)stream;
    hipError_t e = hipMemsetAsync(gtrial, 0, sizeof(uint32_t) * (size_t)n_struct * (n_iter + 1), st);
    if (e == hipSuccess) e = hipMemcpyAsync(xa, xyz, sizeof(float) * 3 * (size_t)n_struct * n_atoms, hipMemcpyDeviceToDevice, st);
    if (e != hipSuccess) return codlad_hip_failed("codlad_relax", e);
    const dim3 grid((unsigned)(row_blocks * n_struct));
    hipLaunchKernelGGL(relax_prep_kernel, grid, dim3(ROWS), 0, st, xyz, T, (int)row_blocks, d0, q0);
    for (int t = 0; t <= n_iter; ++t) {
        hipLaunchKernelGGL(relax_eval_kernel, grid, dim3(ROWS), 0, st, t ? xt : xa, T, k, (int)row_blocks, d0, q0, partials,
                           t ? gt : ga, gtrial + t, n_iter + 1);
        hipLaunchKernelGGL(relax_step_kernel, grid, dim3(ROWS), 0, st, t, n_iter, n_atoms, (int)row_blocks, partials, xa, ga, xt,
                           gt, hst, gacc, gtrial, tr, h0, h_max);
    }
    return codlad_check_launch("codlad_relax");
}
