// Clustering of an ensemble (include/codlad_hip.h, codlad_rmsd_matrix and codlad_cluster_*): which structures of a pool of
// up to 65 536 are the same conformation.
//
// Part one, the all-pairs superposed MSD of one pool.  With the centred float64 coordinates of the selected atoms as the
// matrix X [3 N][n], the correlation matrices S_ij = sum_k (x_ik - c_i)(x_jk - c_j)^T of every pair are the 3 x 3 blocks of
// X X^T: one matrix product on v_mfma_f64_16x16x4_f64, then the per-pair tail of ensemble_math.h (Horn's 4 x 4 by cyclic
// Jacobi; the same text the pair kernels of ensemble_kernels.hip inline), msd = max(Ga + Gb - 2 lambda, 0) / n with Ga,
// Gb from codlad_ens_moments.
//   operand_kernel  fp32 -> float64 exactly, minus the float64 centroid of `mom` (centre first, then products: the
//                   header of ensemble_kernels.hip), written as X [n_pad][3][N_pad] with the conformation fastest, n_pad a
//                   multiple of 4 and N_pad of 64, zeros in the padding and in the row of a conformation that is not
//                   finite.  finite[i] = its centroid and G are finite: a NaN or an infinity among the selected atoms
//                   makes G NaN, and finite fp32 coordinates cannot (G < n * 2^257).
//   matrix_kernel   workgroup (I, J), J >= I, owns the 64 x 64 pairs of conformation blocks I and J, so whole words of the
//                   bitmap.  8 waves; wave w owns the two 16 x 16 wave tiles (ti = w / 2, tj = 2 (w % 2) + {0, 1}).  The
//                   atoms come in ascending order through LDS in chunks of 16 (4 MFMA steps of 4 atoms; chunk and step
//                   depend on n alone), the next chunk's global loads in flight under the current chunk's MFMAs.  An MFMA
//                   operand (row lane & 15, k lane >> 4) is 16 consecutive doubles of a row of X.  With the rows ordered by
//                   component the nine products (a, b) of a tile leave all nine elements of S_ij of the same four pairs
//                   (col = lane & 15, row = (lane >> 4) + 4 reg) in the same lane: the tail runs per lane without a
//                   shuffle.  A tile below the diagonal of a diagonal block is not computed.
// Outputs: element (i, j), i < j, and its mirror are written by the same lane from the same value, the diagonal as 0, a
// non-finite structure's row and column as NaN; one writer per element.  The decision msd <= cut2 (no square root) goes
// through __ballot into 16-bit segments in LDS, one writer per segment, and thread t writes word J of row 64 I + t and
// word I of row 64 J + t (their union in a diagonal block).  No atomics, no scratch memory, one order of summation: a replay
// is bit-identical, and msd_ij depends on the coordinates of i and j alone - not on N, the place in the pool or in a tile,
// or on which of the two is the row (the transposed pair gives the transposed S to the bit, and the tail is handed S or
// its transpose by a rule that does not know the order).  It does NOT return codlad_ens_pair_msd's bits: there a lane adds atoms l, l + 256, .. and a tree adds the
// lanes, here the atoms are added in ascending order by fused multiply-adds.
// What is kept - 8 waves, two tiles a wave - takes 226 VGPRs, no AGPRs and no scratch: two waves per SIMD.  One tile a wave
// (16 waves, four per SIMD) compiles to 128 VGPRs and 60 bytes of scratch per lane and was dropped for that.
//
// Part two, Daura's (GROMOS) clustering from the bitmap: among the active structures the one with the most active
// neighbours (itself included, lowest index first) is the next centre; it and its active neighbours leave the pool.
// Integers only, no host round trip per cluster, no kernel that waits for another (the discipline of
// reweight_kernels.hip): state[ST_PHASE] turns every launch of a finished problem into an immediate return.
//   init_kernel     active = finite & (j < N), labels = -1, the counters                    (only when the state says new)
//   count_kernel    count[i] = popcount(row_i & active), a wave per row                      (only before the first pick)
//   pick_kernel     one workgroup: argmax of count over the active rows; centre, size, labels of row_c & active, the
//                   removed set R, active &= ~R.  When the maximum is 1 every structure left is its own cluster: this
//                   launch numbers them in ascending order and finishes.
//   update_kernel   count[i] -= popcount(row_i & R) for the rows still active, a wave per row, R staged once per workgroup
// The diagonal bit is taken as set and bits at j >= N are masked here, whatever the bitmap holds.
#include "common.h"
#include "ensemble_math.h"
#include "host_util.h"
#include "reduce_math.h"

namespace {
constexpr int MAX_N = CODLAD_CLUSTER_MAX_N;
constexpr int BLK = 64;                     // conformations of a block = bits of a word
constexpr int OP_ATOMS = 16;                // operand kernel: atoms of a workgroup
constexpr int KC = 16;                      // matrix kernel: atoms of a staging chunk
constexpr int ROW = 3 * BLK + 16;           // doubles of one atom of a panel in LDS: the four k of an operand on other banks
constexpr int NW = 8, TJ = 2;               // waves of a workgroup, wave tiles of a wave
constexpr int MT = NW * 64;
constexpr int PANEL = KC * 3 * BLK;         // doubles of a chunk of one block
constexpr int LOADS = 2 * PANEL / MT;       // per thread and chunk
static_assert(2 * PANEL % MT == 0 && NW * TJ == 16, "the chunk is spread evenly; 16 wave tiles");

// grid (N_pad / 64, ceil(n_pad / 16)): 64 conformations x 16 atoms through LDS, read along the atoms, written along the
// conformations
__global__ __launch_bounds__(256) void operand_kernel(const float *x, const double *mom, int N, int n_atoms, const int32_t *sel,
                                                      int m, int n_pad, int N_pad, double *X, uint8_t *finite) {
    __shared__ double tile[OP_ATOMS * 3][BLK + 1];
    __shared__ double cen[BLK][3];
    __shared__ int ok[BLK];
    const int i0 = blockIdx.x * BLK, k0 = blockIdx.y * OP_ATOMS, t = threadIdx.x;
    if (t < BLK) {
        const int i = i0 + t;
        bool f = false;
        if (i < N) {
            const double *mi = mom + 4 * (size_t)i;
            f = fin64(mi[0]) && fin64(mi[1]) && fin64(mi[2]) && fin64(mi[3]);
            cen[t][0] = mi[0], cen[t][1] = mi[1], cen[t][2] = mi[2];
            if (blockIdx.y == 0) finite[i] = f ? 1 : 0;
        }
        ok[t] = f ? 1 : 0;
    }
    __syncthreads();
    for (int e = t; e < BLK * OP_ATOMS * 3; e += 256) {
        const int ci = e / (OP_ATOMS * 3), r = e % (OP_ATOMS * 3), k = k0 + r / 3, c = r % 3;
        double v = 0.0;
        if (ok[ci] && k < m) {
            const int row = sel ? sel[k] : k;
            if ((unsigned)row < (unsigned)n_atoms)
                v = (double)x[((size_t)(i0 + ci) * n_atoms + row) * 3 + c] - cen[ci][c];
        }
        tile[r][ci] = v;
    }
    __syncthreads();
    for (int e = t; e < BLK * OP_ATOMS * 3; e += 256) {
        const int r = e / BLK, ci = e % BLK, k = k0 + r / 3;
        if (k < n_pad) X[((size_t)k * 3 + r % 3) * N_pad + i0 + ci] = tile[r][ci];
    }
}

struct Mat {
    const double *X, *mom;
    const uint8_t *finite;
    int N, N_pad, n_pad, W, squared;
    double n, cut2;
    double *out;
    unsigned long long *bits;
};

// element e of a chunk's 2 * PANEL doubles: rows of 64 consecutive doubles of X, block I's then block J's
__device__ __forceinline__ double chunk_load(const Mat &p, int I, int J, int k0, int e) {
    const int which = e / PANEL, r = (e % PANEL) / BLK, c = e % BLK, k = k0 + r / 3;
    if (k >= p.n_pad) return 0.0;
    return p.X[((size_t)k * 3 + r % 3) * p.N_pad + (which ? J : I) * BLK + c];
}

__global__ __launch_bounds__(MT) void matrix_kernel(Mat p) {
    const int J = blockIdx.x, I = blockIdx.y;
    if (J < I) return;
    __shared__ double panel[2][KC * ROW];
    __shared__ unsigned short rowseg[BLK][4], colseg[BLK][4];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int ti = wave / (4 / TJ), tj0 = (wave % (4 / TJ)) * TJ;
    const int lr = lane & 15, lk = lane >> 4;
    bool on[TJ];
#pragma unroll
    for (int u = 0; u < TJ; ++u) on[u] = I != J || tj0 + u >= ti;          // uniform in the wave
    double4_t acc[TJ][9];
#pragma unroll
    for (int u = 0; u < TJ; ++u)
#pragma unroll
        for (int s = 0; s < 9; ++s) acc[u][s] = double4_t{0.0, 0.0, 0.0, 0.0};
    double stage[LOADS];
#pragma unroll
    for (int l = 0; l < LOADS; ++l) stage[l] = chunk_load(p, I, J, 0, t + l * MT);
    for (int k0 = 0; k0 < p.n_pad; k0 += KC) {
        __syncthreads();                                     // the previous chunk has been read
#pragma unroll
        for (int l = 0; l < LOADS; ++l) {
            const int e = t + l * MT;
            panel[e / PANEL][((e % PANEL) / BLK / 3) * ROW + ((e % PANEL) / BLK % 3) * BLK + e % BLK] = stage[l];
        }
        __syncthreads();
        if (k0 + KC < p.n_pad)
#pragma unroll
            for (int l = 0; l < LOADS; ++l) stage[l] = chunk_load(p, I, J, k0 + KC, t + l * MT);
        const int steps = min(KC, p.n_pad - k0) / 4;
        for (int s4 = 0; s4 < steps; ++s4) {
            const double *pa = &panel[0][(s4 * 4 + lk) * ROW + ti * 16 + lr];
            const double a[3] = {pa[0], pa[BLK], pa[2 * BLK]};
#pragma unroll
            for (int u = 0; u < TJ; ++u) {
                if (!on[u]) continue;
                const double *pb = &panel[1][(s4 * 4 + lk) * ROW + (tj0 + u) * 16 + lr];
                const double b[3] = {pb[0], pb[BLK], pb[2 * BLK]};
#pragma unroll
                for (int r = 0; r < 3; ++r)
#pragma unroll
                    for (int c = 0; c < 3; ++c)
                        acc[u][3 * r + c] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[r], b[c], acc[u][3 * r + c], 0, 0, 0);
            }
        }
    }
    // the tail: pair (row q + 4 reg of tile ti, column lr of tile tj) of this lane, q = lane >> 4
    const int gj_base = J * BLK + lr;
    const double zero3[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int u = 0; u < TJ; ++u) {
        const int tj = tj0 + u, gj = gj_base + tj * 16;
        const bool in_j = gj < p.N;
        const bool fj = in_j && p.finite[gj] != 0;
        const double Gj = in_j ? p.mom[4 * (size_t)gj + 3] : 0.0;
        unsigned colbits = 0;
#pragma unroll 1
        for (int reg = 0; reg < 4; ++reg) {
            const int gi = I * BLK + ti * 16 + lk + 4 * reg;
            const bool valid = on[u] && gi < p.N && in_j, upper = gi < gj, diag = gi == gj;
            const bool fin = valid && fj && p.finite[gi] != 0;
            double msd = nan64();
            if (fin && upper) {
                double S[9];
#pragma unroll
                for (int s = 0; s < 9; ++s) {
                    const double4_t v = acc[u][s];
                    S[s] = reg == 0 ? v.x : reg == 1 ? v.y : reg == 2 ? v.z : v.w;
                }
                // S or its transpose, whichever is the larger in the order (xy, xz, yz): which structure of the pair is the
                // row must not matter, and the Jacobi's choice at tau = +-0 (two equal diagonal elements, planar against
                // collinear) is not mirrored under the transpose
                const bool tr = S[1] != S[3] ? S[1] < S[3] : S[2] != S[6] ? S[2] < S[6] : S[5] < S[7];
                if (tr) {
                    double h;
                    h = S[1], S[1] = S[3], S[3] = h;
                    h = S[2], S[2] = S[6], S[6] = h;
                    h = S[5], S[5] = S[7], S[7] = h;
                }
                msd = ens_solve_pair(S, p.mom[4 * (size_t)gi + 3], Gj, zero3, zero3, p.n, nullptr);
            } else if (fin && diag) {
                msd = 0.0;
            }
            if (p.out && valid && (upper || diag)) {
                const double v = p.squared ? msd : sqrt(msd);
                p.out[(size_t)gi * p.N + gj] = v;
                if (upper) p.out[(size_t)gj * p.N + gi] = v;
            }
            const bool dec = fin && (upper ? msd <= p.cut2 : diag);
            const unsigned long long b = __ballot(dec);
            if (lane < 4) rowseg[ti * 16 + 4 * reg + lane][tj] = (unsigned short)((b >> (16 * lane)) & 0xffffull);
#pragma unroll
            for (int q = 0; q < 4; ++q) colbits |= (unsigned)((b >> (16 * q + lr)) & 1ull) << (4 * reg + q);
        }
        if (lane < 16) colseg[tj * 16 + lane][ti] = (unsigned short)colbits;
    }
    if (!p.bits) return;                                     // uniform
    __syncthreads();
    if (t < BLK) {
        const unsigned long long rw = (unsigned long long)rowseg[t][0] | (unsigned long long)rowseg[t][1] << 16 |
                                      (unsigned long long)rowseg[t][2] << 32 | (unsigned long long)rowseg[t][3] << 48;
        const unsigned long long cw = (unsigned long long)colseg[t][0] | (unsigned long long)colseg[t][1] << 16 |
                                      (unsigned long long)colseg[t][2] << 32 | (unsigned long long)colseg[t][3] << 48;
        if (I == J) {
            if (I * BLK + t < p.N) p.bits[(size_t)(I * BLK + t) * p.W + I] = rw | cw;
        } else {
            if (I * BLK + t < p.N) p.bits[(size_t)(I * BLK + t) * p.W + J] = rw;
            if (J * BLK + t < p.N) p.bits[(size_t)(J * BLK + t) * p.W + I] = cw;
        }
    }
}

// ------------------------------------------------------------------------------------------------------- clustering --
enum { PH_NEW = 0, PH_SET_UP = 1, PH_RUNNING = 2, PH_DONE = 3 };
constexpr int CT = 1024;                    // threads of the one-workgroup kernels: a thread per word of `active`

struct Cl {
    const unsigned long long *bits;
    const uint8_t *finite;
    int N, W;
    int32_t *state, *labels, *centres, *sizes, *count;
    unsigned long long *active, *removed;
};

__device__ inline unsigned long long word_mask(int N, int w) {          // the bits of word w that are structures
    const int left = N - w * 64;
    return left >= 64 ? ~0ull : left <= 0 ? 0ull : (1ull << left) - 1ull;
}

__global__ __launch_bounds__(CT) void init_kernel(Cl c) {
    if (c.state[CODLAD_CLUSTER_ST_PHASE] != PH_NEW) return;
    __shared__ int red[CT / 64];
    const int t = threadIdx.x;
    int n = 0;
    if (t < c.W) {
        unsigned long long a = 0;
        const int left = min(64, c.N - t * 64);
        for (int b = 0; b < left; ++b)
            if (!c.finite || c.finite[t * 64 + b]) a |= 1ull << b;
        c.active[t] = a;
        c.removed[t] = 0;
        n = __popcll(a);
    }
    for (int i = t; i < c.N; i += CT) c.labels[i] = -1;
    n = block_sum(n, red);
    if (t == 0) {
        c.state[CODLAD_CLUSTER_ST_ACTIVE] = n;
        c.state[CODLAD_CLUSTER_ST_CLUSTERS] = 0;
        c.state[CODLAD_CLUSTER_ST_ROUNDS] = 0;
        c.state[CODLAD_CLUSTER_ST_PHASE] = n ? PH_SET_UP : PH_DONE;
    }
}

// MODE 0: count[i] = popcount((row_i | bit i) & active); MODE 1: count[i] -= popcount((row_i | bit i) & removed).  A wave
// per row, 16 rows a wave, the set staged once per workgroup.
template <int MODE> __global__ __launch_bounds__(256) void count_kernel(Cl c) {
    if (c.state[CODLAD_CLUSTER_ST_PHASE] != (MODE == 0 ? PH_SET_UP : PH_RUNNING)) return;
    __shared__ unsigned long long set[MAX_N / 64], act[MAX_N / 64];
    for (int w = threadIdx.x; w < c.W; w += 256) {
        act[w] = c.active[w];
        set[w] = MODE == 0 ? c.active[w] : c.removed[w];
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int rr = 0; rr < 16; ++rr) {
        const int i = blockIdx.x * 64 + wave * 16 + rr;                  // uniform in the wave
        if (i >= c.N) break;
        if (!((act[i >> 6] >> (i & 63)) & 1ull)) {
            if (MODE == 0 && lane == 0) c.count[i] = 0;
            continue;
        }
        const unsigned long long *row = c.bits + (size_t)i * c.W;
        int n = 0;
        for (int w = lane; w < c.W; w += 64) {
            const unsigned long long s = set[w];
            if (!s) continue;
            unsigned long long r = row[w] & word_mask(c.N, w);
            if (w == (i >> 6)) r |= 1ull << (i & 63);
            n += __popcll(r & s);
        }
        n = wave_sum(n);
        if (lane == 0) c.count[i] = MODE == 0 ? n : c.count[i] - n;
    }
}

__global__ __launch_bounds__(CT) void pick_kernel(Cl c) {
    const int phase = c.state[CODLAD_CLUSTER_ST_PHASE];
    if (phase != PH_SET_UP && phase != PH_RUNNING) return;
    __shared__ unsigned long long keys[CT / 64];
    __shared__ int red[CT / 64];
    __shared__ int scan[CT];
    const int t = threadIdx.x;
    // the largest count among the active rows, the lowest index among equals: key = count << 17 | (2^17 - 1 - i)
    unsigned long long key = 0;
    for (int i = t; i < c.N; i += CT)
        if ((c.active[i >> 6] >> (i & 63)) & 1ull) {
            const unsigned long long k = (unsigned long long)c.count[i] << 17 | (unsigned long long)(0x1ffff - i);
            key = k > key ? k : key;
        }
#pragma unroll
    for (int st = 32; st > 0; st >>= 1) {
        const unsigned long long o = __shfl_xor(key, st);
        key = o > key ? o : key;
    }
    if ((t & 63) == 0) keys[t >> 6] = key;
    __syncthreads();
    key = 0;
    for (int k = 0; k < CT / 64; ++k) key = keys[k] > key ? keys[k] : key;
    const int best = (int)(key >> 17), centre = 0x1ffff - (int)(key & 0x1ffffull);
    const int K = c.state[CODLAD_CLUSTER_ST_CLUSTERS], n_active = c.state[CODLAD_CLUSTER_ST_ACTIVE];
    const unsigned long long a = t < c.W ? c.active[t] : 0ull;
    if (best <= 1 || centre >= c.N) {                                    // (a centre is an active row; the second test never holds)
        // every structure left is its own cluster, numbered in ascending order: what the rule does one at a time
        scan[t] = __popcll(a);
        __syncthreads();
        for (int st = 1; st < CT; st <<= 1) {                            // inclusive scan over the words
            const int v = t >= st ? scan[t - st] : 0;
            __syncthreads();
            scan[t] += v;
            __syncthreads();
        }
        int k = K + scan[t] - __popcll(a);
        for (unsigned long long m = a; m; m &= m - 1) {
            const int i = t * 64 + __ffsll((long long)m) - 1;
            c.labels[i] = k;
            c.centres[k] = i;
            c.sizes[k] = 1;
            ++k;
        }
        if (t < c.W) c.active[t] = 0, c.removed[t] = 0;
        if (t == 0) {
            c.state[CODLAD_CLUSTER_ST_CLUSTERS] = K + n_active;
            c.state[CODLAD_CLUSTER_ST_ACTIVE] = 0;
            c.state[CODLAD_CLUSTER_ST_ROUNDS] += 1;
            c.state[CODLAD_CLUSTER_ST_PHASE] = PH_DONE;
        }
        return;
    }
    unsigned long long r = 0;
    if (t < c.W) {
        r = c.bits[(size_t)centre * c.W + t];
        if (t == (centre >> 6)) r |= 1ull << (centre & 63);
        r &= a;                                                          // a holds no bit at j >= N
        c.removed[t] = r;
        c.active[t] = a & ~r;
        for (unsigned long long m = r; m; m &= m - 1) c.labels[t * 64 + __ffsll((long long)m) - 1] = K;
    }
    const int size = block_sum((int)__popcll(r), red);
    if (t == 0) {
        c.centres[K] = centre;
        c.sizes[K] = size;
        c.state[CODLAD_CLUSTER_ST_CLUSTERS] = K + 1;
        c.state[CODLAD_CLUSTER_ST_ACTIVE] = n_active - size;
        c.state[CODLAD_CLUSTER_ST_ROUNDS] += 1;
        c.state[CODLAD_CLUSTER_ST_PHASE] = n_active - size > 0 ? PH_RUNNING : PH_DONE;
    }
}

// pop[k] = the weights of the structures labelled k added to 0 in ascending index; a thread per cluster
__global__ __launch_bounds__(256) void populations_kernel(const int32_t *labels, const double *w, int N, int K, double *pop) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= K) return;
    double acc = 0.0;
    for (int i = 0; i < N; ++i)
        if (labels[i] == k) acc += w[i];
    pop[k] = acc;
}

struct Pads {
    long long n_pad, N_pad;
};
Pads pads(int N, int m) { return Pads{((long long)m + 3) / 4 * 4, ((long long)N + BLK - 1) / BLK * BLK}; }
long long cluster_words(int N) { return ((long long)N + 63) / 64; }
}  // namespace

extern "C" long long codlad_rmsd_matrix_scratch_bytes(int N, int n_sel) {
    CODLAD_REQUIRE(N > 0 && N <= MAX_N && n_sel > 0, "bad sizes (1 <= N <= CODLAD_CLUSTER_MAX_N, n_sel >= 1)");
    const Pads d = pads(N, n_sel);
    return 8ll * d.n_pad * 3 * d.N_pad;
}

extern "C" int codlad_rmsd_matrix(const float *x, const double *mom, int N, int n_atoms, const int32_t *sel, int n_sel,
                                  double cut2, int squared, double *msd, uint64_t *bits, uint8_t *finite,
                                  void *scratch, void *stream) {
    CODLAD_REQUIRE(x && mom && finite && scratch, "null pointer");
    CODLAD_REQUIRE(N > 0 && N <= MAX_N && n_atoms > 0 && n_sel >= 0, "bad sizes (1 <= N <= CODLAD_CLUSTER_MAX_N)");
    const int m = subset_size(sel, n_sel, n_atoms);
    CODLAD_REQUIRE(m > 0, "sel and n_sel disagree (sel with n_sel > 0, or neither)");
    CODLAD_REQUIRE(msd || bits, "neither msd nor bits is asked for");
    CODLAD_REQUIRE(!bits || (cut2 >= 0.0 && cut2 < __builtin_inf()), "cut2 is not a finite number >= 0");
    const Pads d = pads(N, m);
    CODLAD_REQUIRE((d.n_pad + OP_ATOMS - 1) / OP_ATOMS <= 65535, "too many atoms for one call");
    hipStream_t st = (hipStream_t)stream;
    double *X = (double *)scratch;
    const unsigned nblk = (unsigned)(d.N_pad / BLK);
    hipLaunchKernelGGL(operand_kernel, dim3(nblk, (unsigned)((d.n_pad + OP_ATOMS - 1) / OP_ATOMS)), dim3(256), 0, st, x, mom, N,
                       n_atoms, sel, m, (int)d.n_pad, (int)d.N_pad, X, finite);
    Mat p;
    p.X = X, p.mom = mom, p.finite = finite, p.N = N, p.N_pad = (int)d.N_pad, p.n_pad = (int)d.n_pad, p.W = (int)cluster_words(N);
    p.squared = squared != 0, p.n = (double)m, p.cut2 = cut2, p.out = msd, p.bits = (unsigned long long *)bits;
    hipLaunchKernelGGL(matrix_kernel, dim3(nblk, nblk), dim3(MT), 0, st, p);
    return codlad_check_launch("codlad_rmsd_matrix");
}

extern "C" long long codlad_cluster_scratch_bytes(int N) {
    CODLAD_REQUIRE(N > 0 && N <= MAX_N, "bad size (1 <= N <= CODLAD_CLUSTER_MAX_N)");
    return 16ll * cluster_words(N) + 4ll * N;
}

extern "C" int codlad_cluster_daura(const uint64_t *bits, const uint8_t *finite, int N, int rounds, int32_t *state,
                                    int32_t *labels, int32_t *centres, int32_t *sizes, void *scratch, void *stream) {
    CODLAD_REQUIRE(bits && state && labels && centres && sizes && scratch, "null pointer");
    CODLAD_REQUIRE(N > 0 && N <= MAX_N, "bad size (1 <= N <= CODLAD_CLUSTER_MAX_N)");
    CODLAD_REQUIRE(rounds >= 0 && rounds <= CODLAD_CLUSTER_MAX_ROUNDS, "rounds outside 0 .. CODLAD_CLUSTER_MAX_ROUNDS");
    Cl c;
    c.bits = (const unsigned long long *)bits, c.finite = finite, c.N = N, c.W = (int)cluster_words(N);
    c.state = state, c.labels = labels, c.centres = centres, c.sizes = sizes;
    c.active = (unsigned long long *)scratch;
    c.removed = c.active + c.W;
    c.count = (int32_t *)(c.removed + c.W);
    hipStream_t st = (hipStream_t)stream;
    const dim3 rows((unsigned)((N + 63) / 64));
    hipLaunchKernelGGL(init_kernel, dim3(1), dim3(CT), 0, st, c);            // both return at once unless the state says new
    hipLaunchKernelGGL(count_kernel<0>, rows, dim3(256), 0, st, c);
    for (int r = 0; r < rounds; ++r) {
        hipLaunchKernelGGL(pick_kernel, dim3(1), dim3(CT), 0, st, c);
        hipLaunchKernelGGL(count_kernel<1>, rows, dim3(256), 0, st, c);
    }
    return codlad_check_launch("codlad_cluster_daura");
}

extern "C" int codlad_cluster_populations(const int32_t *labels, const double *w, int N, int K, double *pop, void *stream) {
    CODLAD_REQUIRE(labels && w && pop, "null pointer");
    CODLAD_REQUIRE(N > 0 && N <= MAX_N && K > 0 && K <= N, "bad sizes (1 <= K <= N <= CODLAD_CLUSTER_MAX_N)");
    hipLaunchKernelGGL(populations_kernel, dim3((unsigned)((K + 255) / 256)), dim3(256), 0, (hipStream_t)stream, labels, w, N, K,
                       pop);
    return codlad_check_launch("codlad_cluster_populations");
}
