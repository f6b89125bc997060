// Maximum-entropy reweighting of an ensemble against experimental data (codlad_reweight_solve; include/codlad_hip.h): for
// every theta of the call the minimiser mu of
//   Gamma(mu) = log sum_j w0_j exp(-mu . z_j) + (theta / 2) |mu|^2,   z_jk = c U_jk - v_k, U = Y / sigma, v = y / sigma
// by a damped Newton iteration that never returns to the host: the host enqueues a fixed sequence of launches per
// iteration, and status[p] (-1 while problem p runs) turns the launches of a finished problem into immediate returns.
// No kernel waits for another one.  Float64 throughout, one rounding per operation (-ffp-contract=off; the covariance
// tile asks for its fused multiply-adds by name).
//
// Once per call:
//   prep_kernel     U = Y / sigma, zero rows for the excluded structures; used; the blocks' sums of the cleaned w0
//   prior_kernel    log w0 (normalised), the blocks' partials of <U>_w0
//   prior_sum       <U>_w0
//   init_kernel     per problem: theta, c, mu = mu0 or 0, chi2_prior; status 4 and NaN everywhere when no row is usable
// Per iteration (grid.y = the problem):
//   dot_kernel<0>   a_j = log w0_j - mu . z_j, a wave per row; the blocks' maxima
//   exp_kernel      e_j = exp(a_j - max); the blocks' sums
//   norm_kernel     w_j = e_j / Z; the blocks' partials of <U>_w, sum_j w_j |z_jk| and sum_j w_j log(w_j / w0_j)
//   grad_kernel     one workgroup: <U>_w, g, gscale, every scalar output; converged / cap
//   cov_kernel      the hot path: 64 x 64 tiles of the lower triangle of sum_j w_j (U_jk - <U>_k)(U_jl - <U>_l) per chunk of
//                   rows, one wave per (tile, chunk), 8 x 8 accumulators per lane, both operands staged through LDS
//   hess_kernel     H = c^2 * (the chunks' partials in ascending order) + theta I, padded with an identity to a multiple of 32
//   chol_kernel     one workgroup: blocked Cholesky (32-column panels, diagonal block and trailing-update rows in LDS, the
//                   matrix in global memory), then L y = -g and L^T p = y by blocks of 32
//   dot_kernel<1>   s_j = p . z_j
//   ladder_max, ladder_sum, ladder_pick   Gamma(mu + t p) for t = 2^0 .. 2^-15 from a_j - t s_j; the largest t that
//                   passes the Armijo test moves mu
// Reductions over the structures: blocks of 256 rows whatever the grid, a wave's 64 values by the xor butterfly, the four
// waves and then the blocks in ascending order (reduce_math.h).  No atomics.  An excluded row has U = 0 and w = 0: it adds exact zeros.
#include "common.h"
#include "reduce_math.h"
#include "../../include/codlad_hip.h"

namespace {
constexpr int RB = 256;                  // rows of a block of structures = threads of a workgroup
constexpr int TILE = 64, JT = 16;        // covariance: the tile, the rows staged at a time
constexpr int NB = 32;                   // Cholesky: the panel width
constexpr int NT = CODLAD_REWEIGHT_LADDER;
constexpr int PAR = 8;                   // per problem: theta, c, Gamma, max a, Z, log Z
enum { P_THETA, P_C, P_GAMMA, P_AMAX, P_Z, P_LOGZ };
enum { S_CHI2_PRIOR, S_CHI2, S_SREL, S_PHI };
static_assert(NT == 16 && CODLAD_REWEIGHT_SCALARS == 4, "the ladder and the scalar outputs as the header states them");

struct Rw {
    int N, M, Mp, P, nb, nch, chunk, nt, max_iter;
    double gtol;
    const double *Y, *y, *sigma, *w0_in, *mu0;
    double *U, *w0c, *logw0, *w0blk, *v, *ubar0, *col0;                 // shared by the problems
    double *par, *g, *pv, *ubar, *a, *s, *bmax, *bsum, *bsrel, *col, *lmax, *lsum, *cov, *H;   // per problem
    double *mu, *w, *mean, *scal;                                        // outputs
    int32_t *n_iter, *status;
    uint8_t *used;
};

__device__ inline double ninf64() { return __longlong_as_double(0xfff0000000000000ll); }

// ------------------------------------------------------------------------------------------------------ once per call --
__global__ __launch_bounds__(RB) void prep_kernel(Rw r) {
    __shared__ double red[4];
    __shared__ double wrow[RB];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    for (int rr = 0; rr < 64; ++rr) {
        const int j = blockIdx.x * RB + wv * 64 + rr;                 // uniform in the wave
        if (j >= r.N) {
            if (lane == 0) wrow[wv * 64 + rr] = 0.0;
            continue;
        }
        const double *Yj = r.Y + (size_t)j * r.M;
        int bad = 0;
        for (int k = lane; k < r.M; k += 64) bad |= !fin64(Yj[k]);
        const double w0 = r.w0_in ? r.w0_in[j] : 1.0;
        const bool use = !__any(bad) && fin64(w0) && w0 > 0.0;
        double *Uj = r.U + (size_t)j * r.M;
        for (int k = lane; k < r.M; k += 64) Uj[k] = use ? Yj[k] / r.sigma[k] : 0.0;
        if (lane == 0) {
            r.used[j] = use ? 1 : 0;
            r.w0c[j] = use ? w0 : 0.0;
            wrow[wv * 64 + rr] = use ? w0 : 0.0;
        }
    }
    __syncthreads();
    const double sum = block_sum(wrow[threadIdx.x], red);
    if (threadIdx.x == 0) r.w0blk[blockIdx.x] = sum;
    if (blockIdx.x == 0)
        for (int k = threadIdx.x; k < r.Mp; k += RB) r.v[k] = k < r.M ? r.y[k] / r.sigma[k] : 0.0;
}

__device__ inline double blocks_sum(const double *part, int nb) {    // ascending; every thread reads the same words
    double sum = 0.0;
    for (int b = 0; b < nb; ++b) sum += part[b];
    return sum;
}

__global__ __launch_bounds__(RB) void prior_kernel(Rw r) {
    __shared__ double wrow[RB];
    const double W0 = blocks_sum(r.w0blk, r.nb);
    const int j = blockIdx.x * RB + threadIdx.x;
    double wn = 0.0;
    if (j < r.N) {
        const bool use = r.used[j] != 0;
        wn = use ? r.w0c[j] / W0 : 0.0;
        r.logw0[j] = use ? log(wn) : ninf64();
    }
    wrow[threadIdx.x] = wn;
    __syncthreads();
    const int rows = min(RB, r.N - blockIdx.x * RB);
    for (int k = threadIdx.x; k < r.Mp; k += RB) {
        double su = 0.0;
        if (k < r.M)
            for (int rr = 0; rr < rows; ++rr) su += wrow[rr] * r.U[(size_t)(blockIdx.x * RB + rr) * r.M + k];
        r.col0[(size_t)blockIdx.x * r.Mp + k] = su;
    }
}

__global__ __launch_bounds__(RB) void prior_sum(Rw r) {
    for (int k = threadIdx.x; k < r.Mp; k += RB) {
        double su = 0.0;
        for (int b = 0; b < r.nb; ++b) su += r.col0[(size_t)b * r.Mp + k];
        r.ubar0[k] = su;
    }
}

__global__ __launch_bounds__(RB) void init_kernel(Rw r, int p, double theta, double c) {
    __shared__ double red[4];
    const double W0 = blocks_sum(r.w0blk, r.nb);
    const bool none = !(W0 > 0.0);
    const int e = blockIdx.x * RB + threadIdx.x;
    if (e < r.M) {
        r.mu[(size_t)p * r.M + e] = none ? nan64() : r.mu0 ? r.mu0[(size_t)p * r.M + e] : 0.0;
        if (none) r.mean[(size_t)p * r.M + e] = nan64();
    }
    if (e < r.N && none) r.w[(size_t)p * r.N + e] = nan64();
    if (blockIdx.x) return;
    double part = 0.0;
    for (int k = threadIdx.x; k < r.M; k += RB) {
        const double d = c * r.ubar0[k] - r.v[k];
        part += d * d;
    }
    const double sum = block_sum(part, red);
    if (threadIdx.x == 0) {
        double *par = r.par + (size_t)p * PAR, *sc = r.scal + (size_t)p * CODLAD_REWEIGHT_SCALARS;
        par[P_THETA] = theta;
        par[P_C] = c;
        sc[S_CHI2_PRIOR] = none ? nan64() : r.M > 1 ? sum / (double)(r.M - 1) : 0.0;
        sc[S_CHI2] = sc[S_SREL] = sc[S_PHI] = nan64();
        r.n_iter[p] = 0;
        r.status[p] = none ? CODLAD_REWEIGHT_NONE : -1;
    }
}

// ------------------------------------------------------------------------------------------------------ per iteration --
// MODE 0: a_j = log w0_j - mu . z_j and the block's maximum; MODE 1: s_j = p . z_j.  A wave per row, k = lane, lane + 64, ..
template <int MODE> __global__ __launch_bounds__(RB) void dot_kernel(Rw r) {
    const int p = blockIdx.y;
    if (r.status[p] != -1) return;
    __shared__ double red[4];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const double c = r.par[(size_t)p * PAR + P_C];
    const double *vec = MODE == 0 ? r.mu + (size_t)p * r.M : r.pv + (size_t)p * r.Mp;
    double *out = (MODE == 0 ? r.a : r.s) + (size_t)p * r.N;
    double wmax = ninf64();
    for (int rr = 0; rr < 64; ++rr) {
        const int j = blockIdx.x * RB + wv * 64 + rr;                 // uniform in the wave
        if (j >= r.N) break;
        if (!r.used[j]) {
            if (lane == 0) out[j] = MODE == 0 ? ninf64() : 0.0;
            continue;
        }
        const double *Uj = r.U + (size_t)j * r.M;
        double acc = 0.0;
        for (int k = lane; k < r.M; k += 64) acc += vec[k] * (c * Uj[k] - r.v[k]);
        acc = wave_sum(acc);
        const double val = MODE == 0 ? r.logw0[j] - acc : acc;
        if (lane == 0) out[j] = val;
        if (MODE == 0) wmax = max_nan(wmax, val);
    }
    if (MODE == 0) {
        if (lane == 0) red[wv] = wmax;
        __syncthreads();
        if (threadIdx.x == 0)
            r.bmax[(size_t)p * r.nb + blockIdx.x] = max_nan(max_nan(max_nan(red[0], red[1]), red[2]), red[3]);
    }
}

__global__ __launch_bounds__(RB) void exp_kernel(Rw r) {
    const int p = blockIdx.y;
    if (r.status[p] != -1) return;
    __shared__ double red[4];
    const double *bmax = r.bmax + (size_t)p * r.nb;
    double m = ninf64();
    for (int b = 0; b < r.nb; ++b) m = max_nan(m, bmax[b]);
    const int j = blockIdx.x * RB + threadIdx.x;
    double e = 0.0;
    if (j < r.N) {
        e = r.used[j] ? exp(r.a[(size_t)p * r.N + j] - m) : 0.0;
        r.w[(size_t)p * r.N + j] = e;
    }
    const double sum = block_sum(e, red);
    if (threadIdx.x == 0) {
        r.bsum[(size_t)p * r.nb + blockIdx.x] = sum;
        if (blockIdx.x == 0) r.par[(size_t)p * PAR + P_AMAX] = m;
    }
}

__global__ __launch_bounds__(RB) void norm_kernel(Rw r) {
    const int p = blockIdx.y;
    if (r.status[p] != -1) return;
    __shared__ double red[4];
    __shared__ double wrow[RB];
    const double Z = blocks_sum(r.bsum + (size_t)p * r.nb, r.nb);
    const double c = r.par[(size_t)p * PAR + P_C];
    const int j = blockIdx.x * RB + threadIdx.x;
    double wj = 0.0, term = 0.0;
    if (j < r.N) {
        wj = r.w[(size_t)p * r.N + j] / Z;
        r.w[(size_t)p * r.N + j] = wj;
        if (wj > 0.0) term = wj * (log(wj) - r.logw0[j]);
    }
    wrow[threadIdx.x] = wj;
    const double srel = block_sum(term, red);                         // its barriers publish wrow
    if (threadIdx.x == 0) {
        r.bsrel[(size_t)p * r.nb + blockIdx.x] = srel;
        if (blockIdx.x == 0) r.par[(size_t)p * PAR + P_Z] = Z;
    }
    const int rows = min(RB, r.N - blockIdx.x * RB);
    double *col = r.col + ((size_t)p * r.nb + blockIdx.x) * 2 * r.Mp;
    for (int k = threadIdx.x; k < r.Mp; k += RB) {
        double su = 0.0, sa = 0.0;
        if (k < r.M) {
            const double vk = r.v[k];
            const double *Uk = r.U + (size_t)blockIdx.x * RB * r.M + k;
            for (int rr = 0; rr < rows; ++rr) {
                const double u = Uk[(size_t)rr * r.M], ww = wrow[rr];
                su += ww * u;
                sa += ww * fabs(c * u - vk);
            }
        }
        col[k] = su;
        col[r.Mp + k] = sa;
    }
}

__global__ __launch_bounds__(RB) void grad_kernel(Rw r) {
    const int p = blockIdx.x;
    if (r.status[p] != -1) return;
    __shared__ double red[4];
    const double *par = r.par + (size_t)p * PAR;
    const double theta = par[P_THETA], c = par[P_C];
    const double *mu = r.mu + (size_t)p * r.M;
    double ginf = 0.0, zinf = 0.0, minf = 0.0, chi = 0.0, mu2 = 0.0;
    for (int k = threadIdx.x; k < r.Mp; k += RB) {
        double su = 0.0, sa = 0.0, gk = 0.0;
        if (k < r.M) {
            for (int b = 0; b < r.nb; ++b) {
                const double *col = r.col + ((size_t)p * r.nb + b) * 2 * r.Mp;
                su += col[k];
                sa += col[r.Mp + k];
            }
            const double zk = c * su - r.v[k];
            gk = theta * mu[k] - zk;
            r.mean[(size_t)p * r.M + k] = su * r.sigma[k];
            ginf = max_nan(ginf, fabs(gk));
            zinf = max_nan(zinf, sa);
            minf = max_nan(minf, fabs(mu[k]));
            chi += zk * zk;
            mu2 += mu[k] * mu[k];
        }
        r.ubar[(size_t)p * r.Mp + k] = su;
        r.g[(size_t)p * r.Mp + k] = gk;
    }
    ginf = block_max(ginf, red);
    zinf = block_max(zinf, red);
    minf = block_max(minf, red);
    chi = block_sum(chi, red);
    mu2 = block_sum(mu2, red);
    const double srel = blocks_sum(r.bsrel + (size_t)p * r.nb, r.nb);
    if (threadIdx.x) return;
    const double logZ = par[P_AMAX] + log(par[P_Z]);
    double *pw = r.par + (size_t)p * PAR, *sc = r.scal + (size_t)p * CODLAD_REWEIGHT_SCALARS;
    pw[P_LOGZ] = logZ;
    pw[P_GAMMA] = logZ + (0.5 * theta) * mu2;
    sc[S_CHI2] = r.M > 1 ? chi / (double)(r.M - 1) : 0.0;
    sc[S_SREL] = srel;
    sc[S_PHI] = exp(-srel);
    const double gscale = zinf + theta * minf;
    if (ginf <= r.gtol * gscale) r.status[p] = CODLAD_REWEIGHT_CONVERGED;
    else if (r.n_iter[p] >= r.max_iter) r.status[p] = CODLAD_REWEIGHT_CAP;
}

// one wave per (tile, chunk): lane (ty, tx) of 8 x 8 owns the rows ty * 4 .. + 3 and 32 + ty * 4 .. + 3 of the tile and the
// columns tx * 4 .. + 3 and 32 + tx * 4 .. + 3: four 32-byte LDS reads feed 64 fused multiply-adds
__global__ __launch_bounds__(64) void cov_kernel(Rw r) {
    const int p = blockIdx.y;
    if (r.status[p] != -1) return;
    __shared__ __attribute__((aligned(32))) double As[JT][TILE];
    __shared__ __attribute__((aligned(32))) double Bs[JT][TILE];
    const int ch = blockIdx.x / r.nt, ti = blockIdx.x % r.nt;
    int bi, bj;
    tri_tile_of(ti, bi, bj);
    const int t = threadIdx.x, ty = t >> 3, tx = t & 7;
    const int ka = bi * TILE + t, kb = bj * TILE + t;
    const bool ina = ka < r.M, inb = kb < r.M;
    const double ua = ina ? r.ubar[(size_t)p * r.Mp + ka] : 0.0, ub = inb ? r.ubar[(size_t)p * r.Mp + kb] : 0.0;
    const double *w = r.w + (size_t)p * r.N;
    const int j0 = ch * r.chunk, j1 = min(r.N, j0 + r.chunk);
    double acc[8][8];
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int l = 0; l < 8; ++l) acc[i][l] = 0.0;
    for (int jj = j0; jj < j1; jj += JT) {
#pragma unroll
        for (int rr = 0; rr < JT; ++rr) {
            const int j = jj + rr;
            const bool row = j < j1;                                  // uniform
            const double wj = row ? w[j] : 0.0;
            const double xa = row && ina ? r.U[(size_t)j * r.M + ka] - ua : 0.0;
            const double xb = row && inb ? r.U[(size_t)j * r.M + kb] - ub : 0.0;
            As[rr][t] = wj * xa;
            Bs[rr][t] = xb;
        }
        __syncthreads();
#pragma unroll
        for (int rr = 0; rr < JT; ++rr) {
            double av[8], bv[8];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                av[i] = As[rr][ty * 4 + i];
                av[4 + i] = As[rr][32 + ty * 4 + i];
                bv[i] = Bs[rr][tx * 4 + i];
                bv[4 + i] = Bs[rr][32 + tx * 4 + i];
            }
#pragma unroll
            for (int i = 0; i < 8; ++i)
#pragma unroll
                for (int l = 0; l < 8; ++l) acc[i][l] = fma(av[i], bv[l], acc[i][l]);
        }
        __syncthreads();
    }
    double *out = r.cov + (((size_t)p * r.nch + ch) * r.nt + ti) * (TILE * TILE);
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int l = 0; l < 8; ++l) {
            const int row = (i < 4 ? 0 : 28) + ty * 4 + i, colm = (l < 4 ? 0 : 28) + tx * 4 + l;
            out[row * TILE + colm] = acc[i][l];
        }
}

__global__ __launch_bounds__(RB) void hess_kernel(Rw r) {
    const int p = blockIdx.y;
    if (r.status[p] != -1) return;
    int bi, bj;
    tri_tile_of(blockIdx.x, bi, bj);
    const double theta = r.par[(size_t)p * PAR + P_THETA], c = r.par[(size_t)p * PAR + P_C];
    const double *part = r.cov + ((size_t)p * r.nch * r.nt + blockIdx.x) * (TILE * TILE);
    double *H = r.H + (size_t)p * r.Mp * r.Mp;
    for (int e = threadIdx.x; e < TILE * TILE; e += RB) {
        const int gr = bi * TILE + e / TILE, gs = bj * TILE + e % TILE;
        if (gr >= r.Mp || gs > gr) continue;
        double val = gr == gs ? 1.0 : 0.0;                            // the padding: an identity
        if (gr < r.M) {
            double sum = 0.0;
            for (int ch = 0; ch < r.nch; ++ch) sum += part[(size_t)ch * r.nt * (TILE * TILE) + e];
            val = (c * c) * sum + (gr == gs ? theta : 0.0);
        }
        H[(size_t)gr * r.Mp + gs] = val;
    }
}

__global__ __launch_bounds__(RB) void chol_kernel(Rw r) {
    const int p = blockIdx.x;
    if (r.status[p] != -1) return;
    __shared__ double Ds[NB][NB + 1], Li[TILE][NB + 1], Lj[TILE][NB + 1], yv[CODLAD_SAXS_MAX_Q], part[8][NB + 1];
    __shared__ int bad;
    const int t = threadIdx.x, Mp = r.Mp;
    double *H = r.H + (size_t)p * Mp * Mp;
    if (t == 0) bad = 0;
    for (int kb = 0; kb < Mp; kb += NB) {
        __syncthreads();
        for (int e = t; e < NB * NB; e += RB) {
            const int rr = e / NB, cc = e % NB;
            Ds[rr][cc] = cc <= rr ? H[(size_t)(kb + rr) * Mp + kb + cc] : 0.0;
        }
        __syncthreads();
        for (int c = 0; c < NB; ++c) {
            if (t == 0) {
                double piv = Ds[c][c];
                if (!(piv > 0.0) || !fin64(piv)) bad = 1, piv = 1.0;
                Ds[c][c] = sqrt(piv);
            }
            __syncthreads();
            if (t > c && t < NB) Ds[t][c] = Ds[t][c] / Ds[c][c];
            __syncthreads();
            for (int e = t; e < NB * NB; e += RB) {
                const int rr = e / NB, cc = e % NB;
                if (cc > c && rr >= cc) Ds[rr][cc] = Ds[rr][cc] - Ds[rr][c] * Ds[cc][c];
            }
            __syncthreads();
        }
        if (bad) {                                                    // uniform: read after a barrier
            if (t == 0) r.status[p] = CODLAD_REWEIGHT_FAILED;
            return;
        }
        for (int e = t; e < NB * NB; e += RB) {
            const int rr = e / NB, cc = e % NB;
            if (cc <= rr) H[(size_t)(kb + rr) * Mp + kb + cc] = Ds[rr][cc];
        }
        for (int i = kb + NB + t; i < Mp; i += RB) {                   // the panel: a row per thread against L11^T
            double x[NB];
            double *Hi = H + (size_t)i * Mp + kb;
#pragma unroll
            for (int c = 0; c < NB; ++c) x[c] = Hi[c];
#pragma unroll
            for (int c = 0; c < NB; ++c) {
                double sacc = x[c];
#pragma unroll
                for (int d = 0; d < c; ++d) sacc -= x[d] * Ds[c][d];
                x[c] = sacc / Ds[c][c];
                asm volatile("" ::: "memory");                        // row c of Ds is read here, not 496 words ahead
            }
#pragma unroll
            for (int c = 0; c < NB; ++c) Hi[c] = x[c];
        }
        __syncthreads();
        const int first = kb + NB, ntr = (Mp - first + TILE - 1) / TILE;
        const int ty = t >> 4, tx = t & 15;
        for (int ib = 0; ib < ntr; ++ib)
            for (int jb = 0; jb <= ib; ++jb) {
                const int i0 = first + ib * TILE, j0 = first + jb * TILE;
                for (int e = t; e < TILE * NB; e += RB) {
                    const int rr = e / NB, cc = e % NB;
                    Li[rr][cc] = i0 + rr < Mp ? H[(size_t)(i0 + rr) * Mp + kb + cc] : 0.0;
                    Lj[rr][cc] = j0 + rr < Mp ? H[(size_t)(j0 + rr) * Mp + kb + cc] : 0.0;
                }
                __syncthreads();
                double acc[4][4];
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int l = 0; l < 4; ++l) acc[i][l] = 0.0;
#pragma unroll 4
                for (int c = 0; c < NB; ++c) {
                    double av[4], bv[4];
#pragma unroll
                    for (int i = 0; i < 4; ++i) av[i] = Li[ty + 16 * i][c], bv[i] = Lj[tx + 16 * i][c];
#pragma unroll
                    for (int i = 0; i < 4; ++i)
#pragma unroll
                        for (int l = 0; l < 4; ++l) acc[i][l] += av[i] * bv[l];
                }
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int l = 0; l < 4; ++l) {
                        const int gr = i0 + ty + 16 * i, gs = j0 + tx + 16 * l;
                        if (gr < Mp && gs <= gr) H[(size_t)gr * Mp + gs] -= acc[i][l];
                    }
                __syncthreads();
            }
    }
    // L y = -g, by blocks of 32 rows: eight threads a row for what lies left of the diagonal block, wave 0 for the block
    const double *g = r.g + (size_t)p * Mp;
    for (int k = t; k < Mp; k += RB) yv[k] = -g[k];
    __syncthreads();
    const int l32 = t & 31;
    for (int kb = 0; kb < Mp; kb += NB) {
        {
            const int row = kb + (t >> 3), sub = t & 7;
            double acc = 0.0;
            for (int c = sub; c < kb; c += 8) acc += H[(size_t)row * Mp + c] * yv[c];
            part[sub][t >> 3] = acc;
        }
        for (int e = t; e < NB * NB; e += RB) {
            const int rr = e / NB, cc = e % NB;
            Ds[rr][cc] = cc <= rr ? H[(size_t)(kb + rr) * Mp + kb + cc] : 0.0;
        }
        __syncthreads();
        if (t < 64) {
            double b = yv[kb + l32];
#pragma unroll
            for (int sgrp = 0; sgrp < 8; ++sgrp) b -= part[sgrp][l32];
            for (int c = 0; c < NB; ++c) {
                const double yc = __shfl(b, c) / Ds[c][c];
                if (l32 == c) b = yc;
                else if (l32 > c) b -= Ds[l32][c] * yc;
            }
            if (t < NB) yv[kb + t] = b;
        }
        __syncthreads();
    }
    // L^T x = y, from the last block up: column kb + (t & 31) of the rows below the block, eight row groups
    for (int kb = Mp - NB; kb >= 0; kb -= NB) {
        {
            const int grp = t >> 5;
            double acc = 0.0;
            for (int c = kb + NB + grp; c < Mp; c += 8) acc += H[(size_t)c * Mp + kb + l32] * yv[c];
            part[grp][l32] = acc;
        }
        for (int e = t; e < NB * NB; e += RB) {
            const int rr = e / NB, cc = e % NB;
            Ds[rr][cc] = cc <= rr ? H[(size_t)(kb + rr) * Mp + kb + cc] : 0.0;
        }
        __syncthreads();
        if (t < 64) {
            double b = yv[kb + l32];
#pragma unroll
            for (int sgrp = 0; sgrp < 8; ++sgrp) b -= part[sgrp][l32];
            for (int c = NB - 1; c >= 0; --c) {
                const double xc = __shfl(b, c) / Ds[c][c];
                if (l32 == c) b = xc;
                else if (l32 < c) b -= Ds[c][l32] * xc;
            }
            if (t < NB) yv[kb + t] = b;
        }
        __syncthreads();
    }
    for (int k = t; k < Mp; k += RB) r.pv[(size_t)p * Mp + k] = yv[k];
}

// the trial logits a_j - t_i s_j of the ladder t_i = 2^-i: the blocks' maxima, then the blocks' sums of exp(. - max_i)
__global__ __launch_bounds__(RB) void ladder_max(Rw r) {
    const int p = blockIdx.y;
    if (r.status[p] != -1) return;
    __shared__ double red[4];
    const int j = blockIdx.x * RB + threadIdx.x;
    const bool use = j < r.N && r.used[j];
    const double a = use ? r.a[(size_t)p * r.N + j] : 0.0, s = use ? r.s[(size_t)p * r.N + j] : 0.0;
    double t = 1.0;
    for (int i = 0; i < NT; ++i, t *= 0.5) {
        const double m = block_max(use ? a - t * s : ninf64(), red);
        if (threadIdx.x == 0) r.lmax[((size_t)p * r.nb + blockIdx.x) * NT + i] = m;
    }
}

__global__ __launch_bounds__(RB) void ladder_sum(Rw r) {
    const int p = blockIdx.y;
    if (r.status[p] != -1) return;
    __shared__ double red[4];
    __shared__ double mx[NT];
    if (threadIdx.x < NT) {
        double m = ninf64();
        for (int b = 0; b < r.nb; ++b) m = max_nan(m, r.lmax[((size_t)p * r.nb + b) * NT + threadIdx.x]);
        mx[threadIdx.x] = m;
    }
    __syncthreads();
    const int j = blockIdx.x * RB + threadIdx.x;
    const bool use = j < r.N && r.used[j];
    const double a = use ? r.a[(size_t)p * r.N + j] : 0.0, s = use ? r.s[(size_t)p * r.N + j] : 0.0;
    double t = 1.0;
    for (int i = 0; i < NT; ++i, t *= 0.5) {
        const double sum = block_sum(use ? exp((a - t * s) - mx[i]) : 0.0, red);
        if (threadIdx.x == 0) r.lsum[((size_t)p * r.nb + blockIdx.x) * NT + i] = sum;
    }
}

// thread i < 16 evaluates Gamma(mu + t_i p) and the Armijo test; the largest passing t moves mu
__global__ __launch_bounds__(RB) void ladder_pick(Rw r) {
    const int p = blockIdx.x;
    if (r.status[p] != -1) return;
    __shared__ int pass[NT];
    const double *par = r.par + (size_t)p * PAR;
    const double theta = par[P_THETA], gamma0 = par[P_GAMMA];
    double *mu = r.mu + (size_t)p * r.M;
    const double *pv = r.pv + (size_t)p * r.Mp, *g = r.g + (size_t)p * r.Mp;
    if (threadIdx.x < NT) {
        const int i = threadIdx.x;
        double t = 1.0;
        for (int h = 0; h < i; ++h) t *= 0.5;
        double m = ninf64(), sum = 0.0, n2 = 0.0, gp = 0.0;
        for (int b = 0; b < r.nb; ++b) {
            m = max_nan(m, r.lmax[((size_t)p * r.nb + b) * NT + i]);
            sum += r.lsum[((size_t)p * r.nb + b) * NT + i];
        }
        for (int k = 0; k < r.M; ++k) {
            const double x = mu[k] + t * pv[k];
            n2 += x * x;
            gp += g[k] * pv[k];
        }
        const double gamma = (m + log(sum)) + (0.5 * theta) * n2;
        const double slack = (8.0 * 0x1p-52) * (1.0 + fabs(gamma0));
        pass[i] = gamma <= (gamma0 + (1e-4 * t) * gp) + slack ? 1 : 0;
    }
    __syncthreads();
    int at = -1;
    for (int i = NT - 1; i >= 0; --i)
        if (pass[i]) at = i;
    if (at < 0) {
        if (threadIdx.x == 0) r.status[p] = CODLAD_REWEIGHT_STALLED;
        return;
    }
    double t = 1.0;
    for (int h = 0; h < at; ++h) t *= 0.5;
    for (int k = threadIdx.x; k < r.M; k += RB) mu[k] = mu[k] + t * pv[k];
    if (threadIdx.x == 0) r.n_iter[p] = r.n_iter[p] + 1;
}

// out[t][d] = sum_s w[t][s] * values[s][d], s ascending; a structure of weight 0 is skipped, whatever its values hold
__global__ __launch_bounds__(RB) void mean_kernel(const double *values, const double *w, int S, int D, double *out) {
    const int d = blockIdx.x * RB + threadIdx.x, t = blockIdx.y;
    if (d >= D) return;
    const double *wt = w + (size_t)t * S;
    double acc = 0.0;
    for (int s = 0; s < S; ++s) {
        const double ws = wt[s];
        if (ws != 0.0) acc += ws * values[(size_t)s * D + d];
    }
    out[(size_t)t * D + d] = acc;
}

struct Dims {
    int Mp, nb, nch, chunk, nt;
    long long shared, per_problem;        // doubles
};
Dims dims(int N, int M) {
    Dims d;
    d.Mp = (M + NB - 1) / NB * NB;
    d.nb = (int)(((long long)N + RB - 1) / RB);
    const Chunks c = chunks_of(N);
    d.chunk = c.chunk, d.nch = c.nch;
    d.nt = tri_tiles_of(M, TILE);
    d.shared = (long long)N * M + 2ll * N + d.nb + 2ll * d.Mp + (long long)d.nb * d.Mp;
    d.per_problem = PAR + 3ll * d.Mp + 2ll * N + 3ll * d.nb + 2ll * d.nb * d.Mp + 2ll * d.nb * NT +
                    (long long)d.nch * d.nt * TILE * TILE + (long long)d.Mp * d.Mp;
    return d;
}
bool good(double x) { return x > 0.0 && x < __builtin_inf(); }          // a positive finite number (false for NaN)
}  // namespace

extern "C" long long codlad_reweight_scratch_bytes(int n_struct, int n_obs, int n_problems) {
    CODLAD_REQUIRE(n_struct > 0 && n_obs > 0 && n_problems > 0, "bad counts");
    CODLAD_REQUIRE(n_obs <= CODLAD_SAXS_MAX_Q, "n_obs above CODLAD_SAXS_MAX_Q");
    CODLAD_REQUIRE(n_problems <= CODLAD_REWEIGHT_MAX_PROBLEMS, "more than CODLAD_REWEIGHT_MAX_PROBLEMS problems");
    const Dims d = dims(n_struct, n_obs);
    return 8ll * (d.shared + (long long)n_problems * d.per_problem);
}

extern "C" int codlad_reweight_solve(const double *Y, const double *y, const double *sigma, const double *w0, int n_struct,
                                     int n_obs, const double *theta, const double *scale, int n_problems, const double *mu0,
                                     double gtol, int max_iter, void *scratch, long long scratch_bytes, double *mu, double *w,
                                     double *mean, double *scalars, int32_t *n_iter, int32_t *status, uint8_t *used,
                                     void *stream) {
    CODLAD_REQUIRE(Y && y && sigma && theta && scale && scratch && mu && w && mean && scalars && n_iter && status && used,
                   "null pointer");
    CODLAD_REQUIRE(n_struct > 0 && n_obs > 0 && n_problems > 0 && max_iter > 0, "bad counts");
    CODLAD_REQUIRE(n_obs <= CODLAD_SAXS_MAX_Q, "n_obs above CODLAD_SAXS_MAX_Q");
    CODLAD_REQUIRE(n_problems <= CODLAD_REWEIGHT_MAX_PROBLEMS, "more than CODLAD_REWEIGHT_MAX_PROBLEMS problems");
    CODLAD_REQUIRE(max_iter <= CODLAD_REWEIGHT_MAX_ITER, "max_iter above CODLAD_REWEIGHT_MAX_ITER");
    CODLAD_REQUIRE(good(gtol), "gtol is not a positive finite number");
    for (int p = 0; p < n_problems; ++p)
        CODLAD_REQUIRE(good(theta[p]) && good(scale[p]), "a theta or a scale is not a positive finite number");
    const Dims d = dims(n_struct, n_obs);
    CODLAD_REQUIRE(scratch_bytes >= 8ll * (d.shared + (long long)n_problems * d.per_problem),
                   "scratch smaller than codlad_reweight_scratch_bytes");
    CODLAD_REQUIRE((long long)d.nch * d.nt < (1ll << 31), "too many workgroups for one launch");
    const int N = n_struct, M = n_obs, P = n_problems;
    Rw r;
    r.N = N, r.M = M, r.Mp = d.Mp, r.P = P, r.nb = d.nb, r.nch = d.nch, r.chunk = d.chunk, r.nt = d.nt, r.max_iter = max_iter;
    r.gtol = gtol;
    r.Y = Y, r.y = y, r.sigma = sigma, r.w0_in = w0, r.mu0 = mu0;
    double *at = (double *)scratch;
    auto take = [&at](long long n) { double *q = at; at += n; return q; };
    r.U = take((long long)N * M), r.w0c = take(N), r.logw0 = take(N), r.w0blk = take(d.nb), r.v = take(d.Mp), r.ubar0 = take(d.Mp);
    r.col0 = take((long long)d.nb * d.Mp);
    r.par = take((long long)P * PAR), r.g = take((long long)P * d.Mp), r.pv = take((long long)P * d.Mp), r.ubar = take((long long)P * d.Mp);
    r.a = take((long long)P * N), r.s = take((long long)P * N);
    r.bmax = take((long long)P * d.nb), r.bsum = take((long long)P * d.nb), r.bsrel = take((long long)P * d.nb);
    r.col = take(2ll * P * d.nb * d.Mp), r.lmax = take((long long)P * d.nb * NT), r.lsum = take((long long)P * d.nb * NT);
    r.cov = take((long long)P * d.nch * d.nt * TILE * TILE), r.H = take((long long)P * d.Mp * d.Mp);
    r.mu = mu, r.w = w, r.mean = mean, r.scal = scalars, r.n_iter = n_iter, r.status = status, r.used = used;
    hipStream_t st = (hipStream_t)stream;
    const dim3 rows((unsigned)d.nb), rows_p((unsigned)d.nb, (unsigned)P), one_p((unsigned)P), wg(RB);
    hipLaunchKernelGGL(prep_kernel, rows, wg, 0, st, r);
    hipLaunchKernelGGL(prior_kernel, rows, wg, 0, st, r);
    hipLaunchKernelGGL(prior_sum, dim3(1), wg, 0, st, r);
    const unsigned init_blocks = (unsigned)(((N > M ? N : M) + RB - 1) / RB);
    for (int p = 0; p < P; ++p) hipLaunchKernelGGL(init_kernel, dim3(init_blocks), wg, 0, st, r, p, theta[p], scale[p]);
    int rc = codlad_check_launch("codlad_reweight_solve");
    if (rc) return rc;
    for (int it = 0; it <= max_iter; ++it) {
        hipLaunchKernelGGL(dot_kernel<0>, rows_p, wg, 0, st, r);
        hipLaunchKernelGGL(exp_kernel, rows_p, wg, 0, st, r);
        hipLaunchKernelGGL(norm_kernel, rows_p, wg, 0, st, r);
        hipLaunchKernelGGL(grad_kernel, one_p, wg, 0, st, r);
        if (it < max_iter) {
            hipLaunchKernelGGL(cov_kernel, dim3((unsigned)(d.nch * d.nt), (unsigned)P), dim3(64), 0, st, r);
            hipLaunchKernelGGL(hess_kernel, dim3((unsigned)d.nt, (unsigned)P), wg, 0, st, r);
            hipLaunchKernelGGL(chol_kernel, one_p, wg, 0, st, r);
            hipLaunchKernelGGL(dot_kernel<1>, rows_p, wg, 0, st, r);
            hipLaunchKernelGGL(ladder_max, rows_p, wg, 0, st, r);
            hipLaunchKernelGGL(ladder_sum, rows_p, wg, 0, st, r);
            hipLaunchKernelGGL(ladder_pick, one_p, wg, 0, st, r);
        }
        rc = codlad_check_launch("codlad_reweight_solve");
        if (rc) return rc;
    }
    return 0;
}

extern "C" int codlad_weighted_mean(const double *values, const double *w, int n_struct, int n_values, int n_sets, double *out,
                                    void *stream) {
    CODLAD_REQUIRE(values && w && out, "null pointer");
    CODLAD_REQUIRE(n_struct > 0 && n_values > 0 && n_sets > 0, "bad counts");
    CODLAD_REQUIRE(n_sets <= 65535, "more than 65535 weight sets");
    hipLaunchKernelGGL(mean_kernel, dim3((unsigned)(((long long)n_values + RB - 1) / RB), (unsigned)n_sets), dim3(RB), 0,
                       (hipStream_t)stream, values, w, n_struct, n_values, out);
    return codlad_check_launch("codlad_weighted_mean");
}
