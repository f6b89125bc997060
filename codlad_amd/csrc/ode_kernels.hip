// The ODE samplers (flow matching), their own small translation unit: the element-wise update of the
// step-wise path (ode_combine_kernel) and the kernels of the fused one - the final layer with the stage update
// (ode_stage_kernel) and, for the adaptive method, the stage times, the deterministic error norm with the step controller
// and the commit.
//
// Built with -ffp-contract=off: every product and sum of the updates rounds separately, as torchdiffeq's tensor ops do.
// The one exception is final_head (final_head.h), shared with final_kernel (sampler_kernels.hip, a unit built with
// contraction on): it asks for contraction itself.
#include "common.h"
#include "ode_args.h"
#include "final_head.h"

// out = y + h * sum_i coef[i] * k[i]: the stage / step update of an explicit Runge-Kutta method
struct OdeCombineArgs {
    const float *y;
    const float *k[7];
    float coef[7];
    int n_k;
    float h;
    float *out;
    size_t n;
};
__global__ void ode_combine_kernel(OdeCombineArgs a) {
#pragma clang fp contract(off)
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n) return;
    // torchdiffeq forms sum_i k_i * (beta_i * dt) left to right and adds it to y: separately rounded ops
    float acc = a.k[0][i] * (a.coef[0] * a.h);
    for (int j = 1; j < a.n_k; ++j) acc = acc + a.k[j][i] * (a.coef[j] * a.h);
    a.out[i] = a.y[i] + acc;
}

extern "C" int codlad_ode_combine(const float *y, const float *const *k_host, const float *coef_host, int n_k, float h,
                                  size_t n, float *out, void *stream) {
    CODLAD_REQUIRE(y && k_host && coef_host && out, "null pointer");
    CODLAD_REQUIRE(n_k >= 1 && n_k <= 7 && n > 0, "1 to 7 stages");
    OdeCombineArgs a = {};
    a.y = y; a.n_k = n_k; a.h = h; a.out = out; a.n = n;
    for (int j = 0; j < n_k; ++j) {
        CODLAD_REQUIRE(k_host[j], "null stage pointer");
        a.k[j] = k_host[j];
        a.coef[j] = coef_host[j];
    }
    hipLaunchKernelGGL(ode_combine_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a);
    return codlad_check_launch("codlad_ode_combine");
}

// ---------------------------------------------------------------------------------------------
// The fused path.
// ---------------------------------------------------------------------------------------------
// 32 lanes per node, 8 nodes per 256-thread block, as final_kernel.  Lane c < 3 of a node owns component c: it stores the
// slope and forms the stage's sum with the slopes of earlier stages, which earlier launches wrote.
__global__ __launch_bounds__(256) void ode_stage_kernel(OdeStageArgs a) {
    const int l = threadIdx.x & 31;
    const int n = blockIdx.x * 8 + (threadIdx.x >> 5);
    const bool live = n < a.n_nodes;
    const int nc = live ? n : a.n_nodes - 1;           // whole half waves stay converged for the shuffles
    float o[3];
    final_head(a, 3, nc, l, o);
    if (!live) return;
    if (a.status && l == 0 && any_nonfinite(o)) atomicOr(a.status, CODLAD_STATUS_NONFINITE);
    if (l < 3) {
        const float mine = l == 0 ? o[0] : (l == 1 ? o[1] : o[2]);
        const size_t i = (size_t)n * 3 + l;
        a.k_out[i] = mine;
        const float h = a.h_dev ? *a.h_dev : a.h;
        // ode_combine_kernel's sum: k_m * (coef_m * h) left to right, then added to y
        float acc = (a.self == 0 ? mine : a.k[0][i]) * (a.coef[0] * h);
#pragma unroll
        for (int j = 1; j < 7; ++j)
            if (j < a.n_k) acc = acc + (a.self == j ? mine : a.k[j][i]) * (a.coef[j] * h);
        a.out[i] = a.y[i] + acc;
    }
}

void launch_ode_stage(const OdeStageArgs &a, hipStream_t st) {
    hipLaunchKernelGGL(ode_stage_kernel, dim3((a.n_nodes + 7) / 8), dim3(256), 0, st, a);
}

// Dormand-Prince 5(4): the stage times, as Python forms them for the step-wise path (double, one rounding per operation)
__constant__ double DP_ALPHA[6] = {1.0 / 5, 3.0 / 10, 4.0 / 5, 8.0 / 9, 1.0, 1.0};

// An attempt's step and stage times from the state block (thread 0), and the first stage's input xin = y + k1 * (beta0 *
// hh) (every thread: each forms hh for itself from the state's t and h, which this kernel only reads, and the argument
// t_end).
__global__ __launch_bounds__(256) void ode_times_kernel(codlad_ode_state *s, double t_end, float beta0, const float *y,
                                                        const float *k1, float *xin, size_t n) {
    const double t = s->t, h = s->h;
    const bool clipped = h >= t_end - t;
    const double hh = clipped ? t_end - t : h;
    const float hf = (float)hh;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i == 0) {
        s->t_end = t_end;
        s->clipped = clipped;
        s->hh = hh;
        s->hh_f = hf;
#pragma unroll
        for (int j = 0; j < 6; ++j) s->tf[j] = (float)(t + DP_ALPHA[j] * hh);
    }
    if (i < n) xin[i] = y[i] + k1[i] * (beta0 * hf);
}

void launch_ode_times(codlad_ode_state *state, double t_end, float beta0, const float *y, const float *k1, float *xin,
                      size_t n, hipStream_t st) {
    hipLaunchKernelGGL(ode_times_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, state, t_end, beta0, y, k1,
                       xin, n);
}

// Sum over the workgroup of one double per thread, a fixed pairwise tree; valid in thread 0.
DEV double block_tree_sum(double v, double *red) {
    red[threadIdx.x] = v;
    __syncthreads();
    for (int s = 128; s >= 1; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] = red[threadIdx.x] + red[threadIdx.x + s];
        __syncthreads();
    }
    return red[0];
}

// First pass of the error norm: workgroup b owns the contiguous chunk b of ceil(n / gridDim.x) elements; its thread j adds
// the squares of elements j, j + 256, ... of the chunk in order.  out[1 + b] = the chunk's sum.
template <bool FROM_K>
__global__ __launch_bounds__(256) void ode_norm_partial_kernel(OdeNormArgs a) {
    __shared__ double red[256];
    const size_t chunk = (a.n + gridDim.x - 1) / gridDim.x;
    const size_t first = (size_t)blockIdx.x * chunk;
    const size_t end = first + chunk < a.n ? first + chunk : a.n;
    float h = 0.f;
    if constexpr (FROM_K) h = *a.h_dev;
    double acc = 0.0;
    for (size_t i = first + threadIdx.x; i < end; i += 256) {
        float err;
        if constexpr (FROM_K) {                         // combine(zeros, ks, c_err, hh)
            float e = a.k[0][i] * (a.c_err[0] * h);
#pragma unroll
            for (int j = 1; j < 7; ++j) e = e + a.k[j][i] * (a.c_err[j] * h);
            err = 0.0f + e;
        } else {
            err = a.err[i];
        }
        const float tol = a.atol + a.rtol * fmaxf(fabsf(a.y[i]), fabsf(a.y1[i]));
        const double q = (double)(err / tol);
        acc = acc + q * q;
    }
    const double sum = block_tree_sum(acc, red);
    if (threadIdx.x == 0) a.out[1 + blockIdx.x] = sum;
}

// Second pass, one workgroup: the partials by the same tree, the norm, and - with a state block - torchdiffeq's controller.
__global__ __launch_bounds__(256) void ode_norm_final_kernel(OdeNormArgs a, int n_partials) {
    __shared__ double red[256];
    const double sum = block_tree_sum((int)threadIdx.x < n_partials ? a.out[1 + threadIdx.x] : 0.0, red);
    if (threadIdx.x != 0) return;
    const double ratio = sqrt(sum / (double)a.n);
    a.out[0] = ratio;
    codlad_ode_state *s = a.state;
    if (!s) return;
    s->ratio = ratio;
    s->status = a.status ? *a.status : 0;
    if (!isfinite(ratio)) {                             // never accepted, and h would be NaN: a reject, flagged
        s->accepted = 0;
        s->n_reject = s->n_reject + 1;
        s->nonfinite = 1;
        return;
    }
    const bool accept = ratio <= 1.0;
    const bool clipped = s->clipped != 0;
    const double hh = s->hh;
    // _optimal_step_size: safety 0.9, ifactor 10, dfactor 0.2 (1 when the step is accepted)
    const double factor = ratio == 0.0 ? 10.0 : fmin(10.0, fmax(0.9 / pow(ratio, 0.2), ratio < 1.0 ? 1.0 : 0.2));
    if (accept) {
        s->t = clipped ? s->t_end : s->t + hh;          // a clipped step lands on the output time exactly
        s->n_accept = s->n_accept + 1;
    } else {
        s->n_reject = s->n_reject + 1;
    }
    // the controller's own step survives an accepted clip at an output time
    s->h = clipped && accept ? fmax(s->h, hh * factor) : hh * factor;
    s->accepted = accept;
}

static int ode_norm_blocks(size_t n) {
    const size_t nb = (n + 255) / 256;
    return (int)(nb < CODLAD_ODE_NORM_BLOCKS ? nb : CODLAD_ODE_NORM_BLOCKS);
}

void launch_ode_norm(const OdeNormArgs &a, hipStream_t st) {
    const int nb = ode_norm_blocks(a.n);
    hipLaunchKernelGGL(a.err ? ode_norm_partial_kernel<false> : ode_norm_partial_kernel<true>, dim3(nb), dim3(256), 0, st, a);
    hipLaunchKernelGGL(ode_norm_final_kernel, dim3(1), dim3(256), 0, st, a, nb);
}

extern "C" int codlad_ode_error_norm(const float *err, const float *y, const float *y1, size_t n, float rtol, float atol,
                                     double *out_double, void *stream) {
    CODLAD_REQUIRE(err && y && y1 && out_double, "null pointer");
    CODLAD_REQUIRE(n > 0, "n must be positive");
    OdeNormArgs a = {};
    a.err = err; a.y = y; a.y1 = y1; a.n = n; a.rtol = rtol; a.atol = atol; a.out = out_double;
    launch_ode_norm(a, (hipStream_t)stream);
    return codlad_check_launch("codlad_ode_error_norm");
}

// accepted: y1 -> y and k7 -> k1 (FSAL)
__global__ __launch_bounds__(256) void ode_commit_kernel(const codlad_ode_state *s, float *y, const float *y1, float *k1,
                                                         const float *k7, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || !s->accepted) return;
    y[i] = y1[i];
    k1[i] = k7[i];
}

void launch_ode_commit(const codlad_ode_state *state, float *y, const float *y1, float *k1, const float *k7, size_t n,
                       hipStream_t st) {
    hipLaunchKernelGGL(ode_commit_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, state, y, y1, k1, k7, n);
}
