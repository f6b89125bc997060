// Secondary structure of generated structures (codlad_dssp_hbonds, codlad_dssp_assign; include/codlad_hip.h): the
// Kabsch-Sander hydrogen-bond energy between every C=O and every N-H of a structure, held as bitmaps, and the DSSP states
// (H B E G I T S) read off those bitmaps.  All structures of a call share one topology: bb [n_res][4] names N, CA, C, O of
// every residue, an index outside [0, n_atoms) is an absent atom.
//
// Stage 1, two launches on the caller's stream:
//   dssp_prep_kernel    one workgroup per structure: is a coordinate of an atom bb names NaN or +-inf (integer test on the
//                       bit pattern), the link bit of every residue (into LDS and geom), then kappa and the bend bit.
//   dssp_hbond_kernel   one WAVE per (structure, row i), four rows per workgroup.  The wave holds residue i (N, C, O and
//                       its amide H) in registers and walks the n_res partners in chunks of 64, a lane per partner j: the
//                       lane gathers j's N, C, O, forms H_j from residue j - 1 (the amide H is re-derived where it is used
//                       - fifteen operations beside the two hundred of the pair - so no buffer passes between the launches
//                       and the call needs no workspace), and evaluates BOTH directions of the pair with one inlined
//                       function, ks_energy: E(i -> j) from (C_i, O_i, N_j, H_j) and E(j -> i) from (C_j, O_j, N_i, H_i).
//                       Bit j of acc row i and bit i of don row j are therefore the result of the same instruction sequence
//                       on the same operands: don is the transpose of acc bit for bit.  Each 64-bit word is one ballot,
//                       written by lane 0.  A lane keeps the lowest energy it has seen and its partner in registers (a
//                       later equal energy does not replace it: ties go to the lowest j); one xor-shuffle reduction on the
//                       pair (energy, partner) at the end - a total order, so the result does not depend on the tree.
// There is NO pre-filter: every eligible pair is evaluated, because e_best is the minimum over all of them.  (A CA-CA
// cut-off, as other implementations use, is not part of the definition; leaving it out cannot change a decision.)
// Arithmetic: fp32, one rounding per operation in the order written below (-ffp-contract=off), sqrtf and the division the
// correctly rounded ones, acosf the device library's.  No floating-point atomics, no scratch, results bit-identical from
// call to call and independent of the other structures of the call.
//
// Stage 2, dssp_assign_kernel: one workgroup per structure, phases separated by barriers, per-residue state in LDS
// (15 bytes per residue + the link bitmap: 61 KiB at CODLAD_DSSP_MAX_RES).  It reads the bitmaps, geom and finite only
// (PRO and the chain starts of res_kind have already shaped the bitmaps and the link bits).  Every bridge and ladder test works on 64-bit words, 64 partners at a time: for row i and word w
//   parallel     P_i = (acc[i-1] & don[i+1]) | (shl1(don[i]) & shr1(acc[i]))
//   antiparallel A_i = (acc[i] & don[i])     | (shr1(acc[i-1]) & shl1(don[i+1]))
// with shl1 / shr1 the one-bit shifts of a whole row (they carry across word boundaries), masked by link & shl1(link) (the
// partner j has both its links) and by the five bits i-2 .. i+2; a ladder continues where P_i & (shl1(P_{i-1}) | shr1(P_{i+1}))
// or A_i & (shr1(A_{i-1}) | shl1(A_{i+1})) is not zero.  The work items are the (row, word) pairs, dealt over the threads;
// what a row learns from its words is gathered with integer LDS atomics (or, min): order-independent.  The later phases
// are written as GATHERS (a residue looks at the turns that could cover it), so no two threads write one byte.
#include <cmath>

#include "common.h"
#include "structure_math.h"

namespace {
constexpr int WAVE = 64;
constexpr int ROWS = 4;                      // rows (= waves) per workgroup of dssp_hbond_kernel
constexpr int THREADS = 256;
constexpr int MAX_RES = CODLAD_DSSP_MAX_RES;
constexpr float DEG = 57.295779513082320877f;   // 180 / pi
constexpr float KS_Q = 27.888f;                 // 332 * 0.42 * 0.20 kcal/mol A
constexpr float E_MIN = -9.9f, E_BOND = -0.5f, R_MIN = 0.5f, LINK_MAX = 2.5f, BEND_ABOVE = 70.f;

__device__ inline float dist(V3 a, V3 b) {
    const V3 d = sub(a, b);
    return sqrtf(dot(d, d));
}

// E of the C=O (c, o) with the N-H (n, h), kcal/mol; a NaN stays a NaN (fmaxf would swallow it)
__device__ inline float ks_energy(V3 c, V3 o, V3 n, V3 h) {
    const float r_on = dist(o, n), r_ch = dist(c, h), r_oh = dist(o, h), r_cn = dist(c, n);
    float e = KS_Q * (((1.0f / r_on + 1.0f / r_ch) - 1.0f / r_oh) - 1.0f / r_cn);
    if (e < E_MIN) e = E_MIN;
    if (r_on < R_MIN || r_ch < R_MIN || r_oh < R_MIN || r_cn < R_MIN) e = E_MIN;
    return e;
}

__global__ __launch_bounds__(THREADS) void dssp_prep_kernel(const float *xyz, int n_atoms, int n_res, const int4 *bb,
                                                            const uint8_t *res_kind, uint8_t *geom, float *kappa,
                                                            uint8_t *finite) {
    __shared__ uint8_t link[MAX_RES];
    const int s = blockIdx.x;
    const float *x = xyz + (size_t)s * n_atoms * 3;
    const unsigned n = (unsigned)n_atoms;
    int bad = 0;
    for (int r = threadIdx.x; r < n_res; r += THREADS) {
        const int4 b = bb[r];
        const int idx[4] = {b.x, b.y, b.z, b.w};
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if ((unsigned)idx[k] < n) {
                const V3 p = load3(x, idx[k]);
                bad |= non_finite(p.x) | non_finite(p.y) | non_finite(p.z);
            }
        bool lk = false;
        if (r + 1 < n_res && !(res_kind[r + 1] & CODLAD_DSSP_KIND_CHAIN_START)) {
            const int n_next = bb[r + 1].x;
            if ((unsigned)b.z < n && (unsigned)n_next < n) lk = dist(load3(x, b.z), load3(x, n_next)) <= LINK_MAX;
        }
        link[r] = lk;
    }
    bad = __syncthreads_or(bad);
    uint8_t *g = geom + (size_t)s * n_res;
    float *kp = kappa + (size_t)s * n_res;
    for (int r = threadIdx.x; r < n_res; r += THREADS) {
        float k = quiet_nan();
        if (!bad && r >= 2 && r + 2 < n_res && link[r - 2] && link[r - 1] && link[r] && link[r + 1]) {
            const int a = bb[r - 2].y, b = bb[r].y, c = bb[r + 2].y;
            if ((unsigned)a < n && (unsigned)b < n && (unsigned)c < n) {
                const V3 pb = load3(x, b);
                const V3 u = sub(pb, load3(x, a)), v = sub(load3(x, c), pb);
                float cs = dot(u, v) / sqrtf(dot(u, u) * dot(v, v));
                cs = cs > 1.0f ? 1.0f : (cs < -1.0f ? -1.0f : cs);          // a NaN (a zero vector) stays a NaN
                k = acosf(cs) * DEG;
            }
        }
        kp[r] = k;
        g[r] = bad ? 0 : (uint8_t)((link[r] ? CODLAD_DSSP_GEOM_LINK : 0) | (k > BEND_ABOVE ? CODLAD_DSSP_GEOM_BEND : 0));
    }
    if (threadIdx.x == 0) finite[s] = bad ? 0 : 1;
}

// what a pair needs of one residue
struct Res {
    V3 n, c, o, h;
    bool co, has_h, link;
};

// residue r of a FINITE structure (g = its geom row).  An absent atom reads atom 0 and is never used.
__device__ inline Res load_res(const float *x, unsigned n, const int4 *bb, const uint8_t *res_kind, const uint8_t *g, int r) {
    Res q;
    const int4 b = bb[r];
    const bool has_n = (unsigned)b.x < n, has_c = (unsigned)b.z < n, has_o = (unsigned)b.w < n;
    q.n = load3(x, has_n ? b.x : 0);
    q.c = load3(x, has_c ? b.z : 0);
    q.o = load3(x, has_o ? b.w : 0);
    q.co = has_c && has_o;
    q.link = g[r] & CODLAD_DSSP_GEOM_LINK;
    int4 p = b;
    if (r > 0) p = bb[r - 1];
    // an intact link r-1 -> r says: r starts no chain, C of r-1 and N of r are present
    q.has_h = r > 0 && (g[r - 1] & CODLAD_DSSP_GEOM_LINK) && !(res_kind[r] & CODLAD_DSSP_KIND_PRO) && (unsigned)p.w < n;
    const V3 d = sub(load3(x, q.has_h ? p.z : 0), load3(x, q.has_h ? p.w : 0));
    const float len = sqrtf(dot(d, d));
    q.h = {q.n.x + d.x / len, q.n.y + d.y / len, q.n.z + d.z / len};
    return q;
}

// (energy, partner) a is better than b: lower energy, then lower partner
__device__ inline bool better(float ea, int ja, float eb, int jb) { return ea < eb || (ea == eb && ja < jb); }

__global__ __launch_bounds__(WAVE * ROWS) void dssp_hbond_kernel(const float *xyz, int n_atoms, int n_res, int n_words,
                                                                 int row_blocks, const int4 *bb, const uint8_t *res_kind,
                                                                 const uint8_t *geom, const uint8_t *finite,
                                                                 unsigned long long *acc, unsigned long long *don,
                                                                 float *e_best, int32_t *partner) {
    const int s = blockIdx.x / row_blocks, lane = threadIdx.x & (WAVE - 1);
    const int i = (blockIdx.x % row_blocks) * ROWS + (int)(threadIdx.x / WAVE);          // wave-uniform
    if (i >= n_res) return;
    const size_t row = (size_t)s * n_res + i;
    unsigned long long *arow = acc + row * n_words, *drow = don + row * n_words;
    if (!finite[s]) {
        for (int w = lane; w < n_words; w += WAVE) arow[w] = 0, drow[w] = 0;
        if (lane < 2) {
            e_best[2 * row + lane] = quiet_nan();
            partner[2 * row + lane] = -1;
        }
        return;
    }
    const float *x = xyz + (size_t)s * n_atoms * 3;
    const uint8_t *g = geom + (size_t)s * n_res;
    const unsigned n = (unsigned)n_atoms;
    const Res ri = load_res(x, n, bb, res_kind, g, i);
    const float inf = __uint_as_float(INF_BITS);
    float ea = inf, ed = inf;                 // the lane's lowest E(i -> j) and E(j -> i)
    int ja = -1, jd = -1;
    for (int w = 0; w < n_words; ++w) {
        const int j = w * WAVE + lane;
        const bool have = j < n_res;
        const Res rj = load_res(x, n, bb, res_kind, g, have ? j : i);
        const bool pair = have && j != i;
        const bool ok_a = pair && ri.co && rj.has_h && !(j == i + 1 && ri.link);
        const bool ok_d = pair && rj.co && ri.has_h && !(i == j + 1 && rj.link);
        const float e_a = ks_energy(ri.c, ri.o, rj.n, rj.h);
        const float e_d = ks_energy(rj.c, rj.o, ri.n, ri.h);
        const unsigned long long wa = __ballot(ok_a && e_a < E_BOND), wd = __ballot(ok_d && e_d < E_BOND);
        if (lane == 0) arow[w] = wa, drow[w] = wd;
        if (ok_a && e_a < ea) ea = e_a, ja = j;
        if (ok_d && e_d < ed) ed = e_d, jd = j;
    }
#pragma unroll
    for (int st = WAVE / 2; st > 0; st >>= 1) {
        const float oa = __shfl_xor(ea, st), od = __shfl_xor(ed, st);
        const int pa = __shfl_xor(ja, st), pd = __shfl_xor(jd, st);
        if (better(oa, pa, ea, ja)) ea = oa, ja = pa;
        if (better(od, pd, ed, jd)) ed = od, jd = pd;
    }
    if (lane == 0) {
        e_best[2 * row] = ja < 0 ? 0.f : ea;
        e_best[2 * row + 1] = jd < 0 ? 0.f : ed;
        partner[2 * row] = ja;
        partner[2 * row + 1] = jd;
    }
}

// ------------------------------------------------------------------------------------------------------------ stage 2
typedef unsigned long long u64;

__device__ inline u64 word(const u64 *row, int w, int W) { return (unsigned)w < (unsigned)W ? row[w] : 0ull; }
__device__ inline u64 shl1(const u64 *row, int w, int W) { return (word(row, w, W) << 1) | (word(row, w - 1, W) >> 63); }
__device__ inline u64 shr1(const u64 *row, int w, int W) { return (word(row, w, W) >> 1) | (word(row, w + 1, W) << 63); }
__device__ inline bool bit(const u64 *row, int b) { return (row[b >> 6] >> (b & 63)) & 1; }

struct Maps {
    const u64 *acc, *don, *link;     // the structure's bitmaps [R][W]; its link bitmap [W] (LDS)
    int R, W;
};

// word w of the partners j of residue i in a bridge of the kind: every condition of Bridge(i, j) applied
template <bool ANTI>
__device__ inline u64 bridge_word(const Maps &m, int i, int w) {
    if (i < 1 || i > m.R - 2 || (unsigned)w >= (unsigned)m.W) return 0;
    if (!bit(m.link, i - 1) || !bit(m.link, i)) return 0;
    const int W = m.W;
    const u64 *a0 = m.acc + (size_t)(i - 1) * W, *a1 = a0 + W, *d1 = m.don + (size_t)i * W, *d2 = d1 + W;
    u64 v;
    if (ANTI) v = (word(a1, w, W) & word(d1, w, W)) | (shr1(a0, w, W) & shl1(d2, w, W));
    else v = (word(a0, w, W) & word(d2, w, W)) | (shl1(d1, w, W) & shr1(a1, w, W));
    v &= word(m.link, w, W) & shl1(m.link, w, W);
    u64 near = 0;
#pragma unroll
    for (int d = -2; d <= 2; ++d) {
        const int b = i + d;
        if (b >= 0 && (b >> 6) == w) near |= 1ull << (b & 63);
    }
    return v & ~near;
}

// does a bridge of word v (row i, word w) continue in row i - 1 or i + 1
template <bool ANTI>
__device__ inline bool continues(const Maps &m, int i, int w, u64 v) {
    const u64 lo_m = bridge_word<ANTI>(m, i - 1, w - 1), mid_m = bridge_word<ANTI>(m, i - 1, w), hi_m = bridge_word<ANTI>(m, i - 1, w + 1);
    const u64 lo_p = bridge_word<ANTI>(m, i + 1, w - 1), mid_p = bridge_word<ANTI>(m, i + 1, w), hi_p = bridge_word<ANTI>(m, i + 1, w + 1);
    const u64 up_m = (mid_m << 1) | (lo_m >> 63), down_m = (mid_m >> 1) | (hi_m << 63);     // bit j: j - 1 / j + 1 of row i - 1
    const u64 up_p = (mid_p << 1) | (lo_p >> 63), down_p = (mid_p >> 1) | (hi_p << 63);     // ... of row i + 1
    // parallel: (i-1, j-1) or (i+1, j+1); antiparallel: (i-1, j+1) or (i+1, j-1)
    return (v & (ANTI ? (down_m | up_p) : (up_m | down_p))) != 0;
}

constexpr int TURN3 = 1, TURN4 = 2, TURN5 = 4, HAS_BRIDGE = 1, CONTINUES = 2;
constexpr int NO_PARTNER = 0x7fffffff;

__global__ __launch_bounds__(THREADS) void dssp_assign_kernel(const unsigned long long *acc, const unsigned long long *don,
                                                              const uint8_t *geom, const uint8_t *finite, int n_res,
                                                              int n_words, uint8_t *ss, int32_t *bridge, int32_t *counts) {
    __shared__ u64 link[MAX_RES / 64];
    __shared__ int low[2 * MAX_RES];           // lowest parallel / antiparallel partner
    __shared__ int ladder[MAX_RES];            // HAS_BRIDGE | CONTINUES
    __shared__ uint8_t turn[MAX_RES], state[MAX_RES], next[MAX_RES];
    __shared__ int cnt[8];
    const int s = blockIdx.x, tid = threadIdx.x, R = n_res, W = n_words;
    uint8_t *out = ss + (size_t)s * R;
    int32_t *bout = bridge + (size_t)s * R * 2;
    if (!finite[s]) {                          // uniform over the workgroup
        for (int r = tid; r < R; r += THREADS) out[r] = CODLAD_DSSP_UNDEFINED, bout[2 * r] = -1, bout[2 * r + 1] = -1;
        if (tid < 8) counts[8 * (size_t)s + tid] = -1;
        return;
    }
    const uint8_t *g = geom + (size_t)s * R;
    Maps m = {acc + (size_t)s * R * W, don + (size_t)s * R * W, link, R, W};
    // --- phase 1: the link bitmap (one ballot per word; the last residue has no link whatever geom says), clean tables
    for (int w = tid / WAVE; w < W; w += THREADS / WAVE) {
        const int r = w * WAVE + (tid & (WAVE - 1));
        const u64 v = __ballot(r < R - 1 && (g[r] & CODLAD_DSSP_GEOM_LINK));
        if ((tid & (WAVE - 1)) == 0) link[w] = v;
    }
    for (int r = tid; r < R; r += THREADS) low[2 * r] = NO_PARTNER, low[2 * r + 1] = NO_PARTNER, ladder[r] = 0;
    if (tid < 8) cnt[tid] = 0;
    __syncthreads();
    // --- phase 2: turns per residue; bridges per (row, word)
    for (int i = tid; i < R; i += THREADS) {
        int t = 0;
#pragma unroll
        for (int nn = 3; nn <= 5; ++nn) {
            bool ok = i + nn < R && bit(m.acc + (size_t)i * W, i + nn);
            for (int q = 0; ok && q < nn; ++q) ok = bit(link, i + q);
            if (ok) t |= 1 << (nn - 3);
        }
        turn[i] = (uint8_t)t;
    }
    for (int k = tid; k < R * W; k += THREADS) {
        const int i = k / W, w = k % W;
        const u64 p = bridge_word<false>(m, i, w), a = bridge_word<true>(m, i, w);
        int f = 0;
        if (p) {
            f = HAS_BRIDGE | (continues<false>(m, i, w, p) ? CONTINUES : 0);
            atomicMin(&low[2 * i], w * WAVE + __builtin_ctzll(p));
        }
        if (a) {
            f |= HAS_BRIDGE | (continues<true>(m, i, w, a) ? CONTINUES : 0);
            atomicMin(&low[2 * i + 1], w * WAVE + __builtin_ctzll(a));
        }
        if (f) atomicOr(&ladder[i], f);
    }
    __syncthreads();
    // --- phase 3: H (two consecutive 4-turns at i - 1, i cover i .. i + 3), then E / B where there is no H
    for (int r = tid; r < R; r += THREADS) {
        bool h = false;
        for (int i = r - 3; i <= r; ++i) h |= i >= 1 && (turn[i - 1] & TURN4) && (turn[i] & TURN4);
        int c = CODLAD_DSSP_LOOP;
        if (h) c = CODLAD_DSSP_H;
        else if (ladder[r] & CONTINUES) c = CODLAD_DSSP_E;
        else if (ladder[r] & HAS_BRIDGE) c = CODLAD_DSSP_B;
        state[r] = (uint8_t)c;
    }
    __syncthreads();
    // --- phase 4: G where all three residues of two consecutive 3-turns are still loop (a G set by a neighbouring pair does
    // not block: the test is on the state before this phase)
    for (int r = tid; r < R; r += THREADS) {
        bool gg = false;
        for (int i = r - 2; i <= r; ++i)
            gg |= i >= 1 && i + 2 < R && (turn[i - 1] & TURN3) && (turn[i] & TURN3) && state[i] == CODLAD_DSSP_LOOP &&
                  state[i + 1] == CODLAD_DSSP_LOOP && state[i + 2] == CODLAD_DSSP_LOOP;
        next[r] = gg ? CODLAD_DSSP_G : state[r];
    }
    __syncthreads();
    // --- phase 5: I likewise on five residues; then T and S on what is left
    for (int r = tid; r < R; r += THREADS) {
        bool ii = false;
        for (int i = r - 4; i <= r; ++i) {
            bool ok = i >= 1 && i + 4 < R && (turn[i - 1] & TURN5) && (turn[i] & TURN5);
            for (int q = 0; ok && q < 5; ++q) ok = next[i + q] == CODLAD_DSSP_LOOP;
            ii |= ok;
        }
        int c = ii ? CODLAD_DSSP_I : next[r];
        if (c == CODLAD_DSSP_LOOP) {
            bool t = false;
            for (int k = 1; k <= 4; ++k)
                if (r - k >= 0) {
                    const int tb = turn[r - k];
                    t |= (k <= 2 && (tb & TURN3)) || (k <= 3 && (tb & TURN4)) || (tb & TURN5);
                }
            if (t) c = CODLAD_DSSP_T;
            else if (g[r] & CODLAD_DSSP_GEOM_BEND) c = CODLAD_DSSP_S;
        }
        state[r] = (uint8_t)c;                 // own element only: nobody reads state in this phase
    }
    __syncthreads();
    // --- results; the counts are population counts of ballots, added in LDS
    for (int r0 = 0; r0 < R; r0 += THREADS) {
        const int r = r0 + tid;
        const int c = r < R ? state[r] : -1;
        if (r < R) {
            out[r] = (uint8_t)c;
            bout[2 * r] = low[2 * r] == NO_PARTNER ? -1 : low[2 * r];
            bout[2 * r + 1] = low[2 * r + 1] == NO_PARTNER ? -1 : low[2 * r + 1];
        }
#pragma unroll
        for (int code = 0; code < 8; ++code) {
            const int nn = __popcll(__ballot(c == code));
            if ((tid & (WAVE - 1)) == 0 && nn) atomicAdd(&cnt[code], nn);
        }
    }
    __syncthreads();
    if (tid < 8) counts[8 * (size_t)s + tid] = cnt[tid];
}
}  // namespace

extern "C" int codlad_dssp_hbonds(const float *xyz, int n_struct, int n_atoms, const int32_t *bb, const uint8_t *res_kind,
                                  int n_res, uint64_t *acc, uint64_t *don, uint8_t *geom, float *kappa, float *e_best,
                                  int32_t *partner, uint8_t *finite, void *stream) {
    CODLAD_REQUIRE(xyz && bb && res_kind && acc && don && geom && kappa && e_best && partner && finite, "null pointer");
    CODLAD_REQUIRE(n_struct > 0 && n_res > 0 && n_atoms > 0, "bad counts");
    CODLAD_REQUIRE(((uintptr_t)bb & 15) == 0, "bb is not 16-byte aligned");
    CODLAD_REQUIRE(n_res <= MAX_RES, "more than CODLAD_DSSP_MAX_RES residues");
    const int64_t row_blocks = ((int64_t)n_res + ROWS - 1) / ROWS;
    CODLAD_REQUIRE(row_blocks * n_struct < (int64_t)1 << 31 && (int64_t)n_atoms * 3 < (int64_t)1 << 31,
                   "too many workgroups for one launch");
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(dssp_prep_kernel, dim3((unsigned)n_struct), dim3(THREADS), 0, st, xyz, n_atoms, n_res, (const int4 *)bb,
                       res_kind, geom, kappa, finite);
    int rc = codlad_check_launch("codlad_dssp_hbonds");
    if (rc) return rc;
    hipLaunchKernelGGL(dssp_hbond_kernel, dim3((unsigned)(row_blocks * n_struct)), dim3(WAVE * ROWS), 0, st, xyz, n_atoms, n_res,
                       (n_res + WAVE - 1) / WAVE, (int)row_blocks, (const int4 *)bb, res_kind, geom, finite,
                       (unsigned long long *)acc, (unsigned long long *)don, e_best, partner);
    return codlad_check_launch("codlad_dssp_hbonds");
}

extern "C" int codlad_dssp_assign(const uint64_t *acc, const uint64_t *don, const uint8_t *geom, const uint8_t *finite,
                                  int n_struct, int n_res, uint8_t *ss, int32_t *bridge, int32_t *counts, void *stream) {
    CODLAD_REQUIRE(acc && don && geom && finite && ss && bridge && counts, "null pointer");
    CODLAD_REQUIRE(n_struct > 0 && n_res > 0, "bad counts");
    CODLAD_REQUIRE(n_res <= MAX_RES, "more than CODLAD_DSSP_MAX_RES residues");
    CODLAD_REQUIRE((int64_t)n_struct * n_res < (int64_t)1 << 31, "too many residues for one launch");
    hipLaunchKernelGGL(dssp_assign_kernel, dim3((unsigned)n_struct), dim3(THREADS), 0, (hipStream_t)stream,
                       (const unsigned long long *)acc, (const unsigned long long *)don, geom, finite, n_res,
                       (n_res + WAVE - 1) / WAVE, ss, bridge, counts);
    return codlad_check_launch("codlad_dssp_assign");
}
