// The sampler's tail of a denoiser step: the final layer fused with the step's update (final_kernel), the stand-alone DDPM /
// DDIM / DPM-Solver++ updates around a caller's guidance functions, the timestep embedding with every adaLN head (mods_kernel) and the status
// word.  Built with -fno-honor-nans like the other denoiser units: any_nonfinite (final_head.h) says why that matters here.
#include "sampler_args.h"
#include "final_head.h"

// PIN: residue pinning fused into the update (codlad_sample_loop_pinned): at a node with pin_mask[n] != 0 the step's
// raw pred_xstart is replaced by pin_x0[n] before the clamp.  A template parameter, so that final_kernel<false> (the
// logits mode and the plain loop) carries none of it; the two pointers are then unused arguments.
// STEP: the update of the loop, CODLAD_STEP_* (sampler_args.h).  The DDPM instantiations do not read `mode`.
template <bool PIN, int STEP = CODLAD_STEP_DDPM>
__global__ __launch_bounds__(256) void final_kernel(FinalArgs a, const float *pin_x0, const uint8_t *pin_mask, int mode) {
    const int l = threadIdx.x & 31;
    const int n = blockIdx.x * 8 + (threadIdx.x >> 5);
    const bool live = n < a.n_nodes;
    const int nc = live ? n : a.n_nodes - 1;           // whole half waves stay converged for the shuffles
    float o[6];
    final_head(a, a.n_out, nc, l, o);
    if (!live) return;
    if (a.status && l == 0 && any_nonfinite(o)) atomicOr(a.status, CODLAD_STATUS_NONFINITE);
    if (a.logits) {
        store_logits(a.logits, a.n_out, n, l, o);
        return;
    }
    if (l < 3) {                                        // lane k updates component k
        const float eps = l == 0 ? o[0] : (l == 1 ? o[1] : o[2]);
        const float vv = l == 0 ? o[3] : (l == 1 ? o[4] : o[5]);      // (zeros for a 3-row head: fixed-variance samplers)
        const size_t i = (size_t)n * 3 + l;
        const float *pin = PIN && pin_mask[n] ? pin_x0 + i : nullptr;
        if constexpr (STEP == CODLAD_STEP_DDPM)
            a.x[i] = ddpm_step(a.x[i], eps, vv, a.coef, a.noise[i], a.x_start ? a.x_start + i : nullptr, pin);
        else if constexpr (STEP == CODLAD_STEP_DDIM)
            a.x[i] = ddim_step<false>(a.x[i], eps, a.coef, mode, a.noise[i], a.x_start ? a.x_start + i : nullptr, pin);
        else if constexpr (STEP == CODLAD_STEP_DDIM_REVERSE)
            a.x[i] = ddim_step<true>(a.x[i], eps, a.coef, mode, 0.f, a.x_start ? a.x_start + i : nullptr, pin);
        else
            a.x[i] = dpm_step(a.x[i], eps, a.coef, mode, a.x_start + i, pin);
    }
}

void launch_final(const FinalArgs &fa, int step, const float *pin_x0, const uint8_t *pin_mask, int mode, hipStream_t st) {
    static void (*const kernels[4][2])(FinalArgs, const float *, const uint8_t *, int) = {    // [CODLAD_STEP_*][pinned]
        {final_kernel<false, CODLAD_STEP_DDPM>, final_kernel<true, CODLAD_STEP_DDPM>},
        {final_kernel<false, CODLAD_STEP_DDIM>, final_kernel<true, CODLAD_STEP_DDIM>},
        {final_kernel<false, CODLAD_STEP_DDIM_REVERSE>, final_kernel<true, CODLAD_STEP_DDIM_REVERSE>},
        {final_kernel<false, CODLAD_STEP_DPM>, final_kernel<true, CODLAD_STEP_DPM>}};
    if (step < CODLAD_STEP_DDPM || step > CODLAD_STEP_DPM) __builtin_trap();    // not a CODLAD_STEP_*: a caller's bug
    hipLaunchKernelGGL(kernels[step][pin_x0 != nullptr], dim3((fa.n_nodes + 7) / 8), dim3(256), 0, st, fa, pin_x0, pin_mask, mode);
}

// stand-alone DDPM update on a model output [n][6]
struct DdpmCoef {
    float c[8];
};
static DdpmCoef ddpm_coef(const float *coef_host) {
    DdpmCoef cf;
    for (int k = 0; k < 8; ++k) cf.c[k] = coef_host[k];
    return cf;
}

__global__ void ddpm_kernel(const float *x, const float *out, const float *noise, DdpmCoef cf,
                            int n_nodes, float *x_out, float *x_start) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_nodes * 3) return;
    const int n = i / 3, k = i - 3 * n;
    // a fixed-variance sampler's model has no variance channels (gaussian_diffusion.py:321-334: model_output stays [.., C])
    const bool fixed = ((int)cf.c[7] & CODLAD_DDPM_FIXED_VAR) != 0;
    const float o = fixed ? out[n * 3 + k] : out[n * 6 + k], v = fixed ? 0.f : out[n * 6 + 3 + k];
    x_out[i] = ddpm_step(x[i], o, v, cf.c, noise[i], x_start ? x_start + i : nullptr);
}

// The DDPM update split in two around a caller's denoised_fn / cond_fn (codlad_ddpm_pred_xstart /
// codlad_ddpm_posterior_step): the pieces of ddpm_step, so that a pin applied between them rounds as the fused one.
__global__ void ddpm_pred_xstart_kernel(const float *x, const float *out, DdpmCoef cf, int n_nodes, float *x0_out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_nodes * 3) return;
    const int n = i / 3, k = i - 3 * n;
    const bool fixed = ((int)cf.c[7] & CODLAD_DDPM_FIXED_VAR) != 0;
    x0_out[i] = ddpm_raw_x0(x[i], fixed ? out[n * 3 + k] : out[n * 6 + k], cf.c);
}

__global__ void ddpm_posterior_kernel(const float *x, const float *x0, const float *out, const float *noise,
                                      const float *grad, DdpmCoef cf, float fixed_variance, int n_nodes, float *x_out,
                                      float *x_start) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_nodes * 3) return;
    const int n = i / 3, k = i - 3 * n;
    const bool fixed = ((int)cf.c[7] & CODLAD_DDPM_FIXED_VAR) != 0;
    const float logvar = ddpm_log_variance(fixed ? 0.f : out[n * 6 + 3 + k], cf.c);
    // the variance that scales the gradient: exp(model_log_variance) for the learned range, the table value for
    // fixed variance (gaussian_diffusion.py:318, 320-334)
    const float variance = fixed ? fixed_variance : expf(logvar);
    x_out[i] = ddpm_posterior(x[i], x0[i], logvar, cf.c, noise[i], x_start ? x_start + i : nullptr,
                              grad ? grad + i : nullptr, variance);
}

// The DDIM update after a caller's denoised_fn / cond_fn (codlad_ddim_step): its first half is ddpm_pred_xstart_kernel,
// whose raw pred_xstart is ddim_step's; this is ddim_update, so a pin applied between them rounds as the fused one.
template <bool REVERSE>
__global__ void ddim_update_kernel(const float *x, const float *x0, const float *noise, const float *grad, DdpmCoef cf,
                                   int mode, int n_nodes, float *x_out, float *x_start) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_nodes * 3) return;
    x_out[i] = ddim_update<REVERSE>(x[i], x0[i], cf.c, mode, REVERSE ? 0.f : noise[i], x_start ? x_start + i : nullptr,
                                    grad ? grad + i : nullptr);
}

// The DPM-Solver++(2M) update after a caller's denoised_fn / cond_fn (codlad_dpm_step): dpm_update on the processed
// pred_xstart, as ddim_update_kernel is ddim_update.  x0_prev is null for a row whose C is 0, which does not read it.
__global__ void dpm_update_kernel(const float *x, const float *x0, const float *x0_prev, const float *grad, DdpmCoef cf,
                                  int mode, int n_nodes, float *x_out, float *x_start) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_nodes * 3) return;
    x_out[i] = dpm_update(x[i], x0[i], cf.c, mode, x0_prev ? x0_prev + i : nullptr, x_start ? x_start + i : nullptr,
                          grad ? grad + i : nullptr);
}

// ---------------------------------------------------------------------------------------------
// Timestep embedding + all adaLN heads, one workgroup per timestep (row 3).
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void mods_kernel(codlad_denoiser_weights w, const int64_t *tv, const float *tf,
                                                  float *mods) {
    __shared__ float emb[256];
    __shared__ float hid[HD];
    __shared__ float sc[HD];
    const int tid = threadIdx.x;
    const float t = tv ? (float)tv[blockIdx.x] : tf[blockIdx.x];   // latent_model.py:66: t[:, None].float() * freqs
    {
        const int k = tid & 127;
        const float arg = t * w.freqs[k];
        emb[tid] = tid < 128 ? cosf(arg) : sinf(arg);
    }
    __syncthreads();
    if (tid < HD) {
        float acc = 0.f;
        const float *wr = w.t_w0 + tid * 256;
        for (int k = 0; k < 256; ++k) acc = fmaf(emb[k], wr[k], acc);
        acc += w.t_b0[tid];
        hid[tid] = acc / (1.0f + expf(-acc));
    }
    __syncthreads();
    if (tid < HD) {
        float acc = 0.f;
        const float *wr = w.t_w2 + tid * HD;
        for (int k = 0; k < HD; ++k) acc = fmaf(hid[k], wr[k], acc);
        acc += w.t_b2[tid];
        sc[tid] = acc / (1.0f + expf(-acc));  // SiLU(c) feeds every adaLN head
    }
    __syncthreads();
    float *out = mods + (size_t)blockIdx.x * CODLAD_MODS_PER_STEP;
    int off = 0;
    for (int hd = 0; hd < 7; ++hd) {
        const int rows = hd < 3 ? 9 * HD : (hd < 6 ? 6 * HD : 2 * HD);
        for (int r = tid; r < rows; r += 256) {
            const float *wr = w.ada_w[hd] + (size_t)r * HD;
            float acc = 0.f;
            for (int k = 0; k < HD; ++k) acc = fmaf(sc[k], wr[k], acc);
            out[off + r] = acc + w.ada_b[hd][r];
        }
        off += rows;
    }
}

extern "C" int codlad_step_mods(const codlad_denoiser_weights *w, const int64_t *t_values, int n_t,
                                float *mods, void *stream) {
    CODLAD_REQUIRE(w && t_values && mods, "null pointer");
    CODLAD_REQUIRE(n_t > 0, "n_t must be positive");
    hipLaunchKernelGGL(mods_kernel, dim3(n_t), dim3(256), 0, (hipStream_t)stream, *w, t_values, (const float *)nullptr, mods);
    return codlad_check_launch("codlad_step_mods");
}

extern "C" int codlad_step_mods_f(const codlad_denoiser_weights *w, const float *t_values, int n_t, float *mods,
                                  void *stream) {
    CODLAD_REQUIRE(w && t_values && mods, "null pointer");
    CODLAD_REQUIRE(n_t > 0, "n_t must be positive");
    hipLaunchKernelGGL(mods_kernel, dim3(n_t), dim3(256), 0, (hipStream_t)stream, *w, (const int64_t *)nullptr, t_values, mods);
    return codlad_check_launch("codlad_step_mods_f");
}

extern "C" int codlad_ddpm_update(const float *x, const float *model_out, const float *noise,
                                  const float *coef_host, int n_nodes, float *x_out, float *x_start_out,
                                  void *stream) {
    CODLAD_REQUIRE(x && model_out && noise && coef_host && x_out, "null pointer");
    CODLAD_REQUIRE(n_nodes > 0, "n_nodes must be positive");
    hipLaunchKernelGGL(ddpm_kernel, dim3((n_nodes * 3 + 255) / 256), dim3(256), 0,
                       (hipStream_t)stream, x, model_out, noise, ddpm_coef(coef_host), n_nodes, x_out, x_start_out);
    return codlad_check_launch("codlad_ddpm_update");
}

extern "C" int codlad_ddpm_pred_xstart(const float *x, const float *model_out, const float *coef_host, int n_nodes,
                                      float *pred_xstart, void *stream) {
    CODLAD_REQUIRE(x && model_out && coef_host && pred_xstart, "null pointer");
    CODLAD_REQUIRE(n_nodes > 0, "n_nodes must be positive");
    hipLaunchKernelGGL(ddpm_pred_xstart_kernel, dim3((n_nodes * 3 + 255) / 256), dim3(256), 0, (hipStream_t)stream, x,
                       model_out, ddpm_coef(coef_host), n_nodes, pred_xstart);
    return codlad_check_launch("codlad_ddpm_pred_xstart");
}

extern "C" int codlad_ddpm_posterior_step(const float *x, const float *pred_xstart, const float *model_out,
                                          const float *noise, const float *grad, const float *coef_host,
                                          float fixed_variance, int n_nodes, float *x_out, float *x_start_out,
                                          void *stream) {
    CODLAD_REQUIRE(x && pred_xstart && model_out && noise && coef_host && x_out, "null pointer");
    CODLAD_REQUIRE(n_nodes > 0, "n_nodes must be positive");
    hipLaunchKernelGGL(ddpm_posterior_kernel, dim3((n_nodes * 3 + 255) / 256), dim3(256), 0, (hipStream_t)stream, x,
                       pred_xstart, model_out, noise, grad, ddpm_coef(coef_host), fixed_variance, n_nodes, x_out, x_start_out);
    return codlad_check_launch("codlad_ddpm_posterior_step");
}

extern "C" int codlad_ddim_step(const float *x, const float *pred_xstart, const float *noise, const float *grad,
                                const float *coef_host, int reverse, int n_nodes, float *x_out, float *x_start_out,
                                void *stream) {
    CODLAD_REQUIRE(x && pred_xstart && coef_host && x_out, "null pointer");
    CODLAD_REQUIRE(reverse || noise, "null pointer (noise: only the reverse step runs without it)");
    CODLAD_REQUIRE(n_nodes > 0, "n_nodes must be positive");
    const int mode = (int)coef_host[7];
    const dim3 grid((n_nodes * 3 + 255) / 256);
    hipLaunchKernelGGL(reverse ? ddim_update_kernel<true> : ddim_update_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream,
                       x, pred_xstart, reverse ? nullptr : noise, grad, ddpm_coef(coef_host), mode, n_nodes, x_out, x_start_out);
    return codlad_check_launch("codlad_ddim_step");
}

extern "C" int codlad_dpm_step(const float *x, const float *pred_xstart, const float *prev_xstart, const float *grad,
                               const float *coef_host, int n_nodes, float *x_out, float *x_start_out, void *stream) {
    CODLAD_REQUIRE(x && pred_xstart && coef_host && x_out, "null pointer");
    CODLAD_REQUIRE(n_nodes > 0, "n_nodes must be positive");
    CODLAD_REQUIRE((coef_host[4] != 0.f) == (prev_xstart != nullptr),
                   "prev_xstart is given exactly when the row's C (column 4) is not 0: a second-order row needs the previous "
                   "step's pred_xstart, a first-order row reads none");
    const int mode = (int)coef_host[7];
    hipLaunchKernelGGL(dpm_update_kernel, dim3((n_nodes * 3 + 255) / 256), dim3(256), 0, (hipStream_t)stream, x, pred_xstart,
                       prev_xstart, grad, ddpm_coef(coef_host), mode, n_nodes, x_out, x_start_out);
    return codlad_check_launch("codlad_dpm_step");
}

extern "C" int codlad_status_check(int32_t *status, void *stream) {
    CODLAD_REQUIRE(status, "null pointer");
    int32_t host = 0;
    hipStream_t st = (hipStream_t)stream;
    hipError_t e = hipMemcpyAsync(&host, status, sizeof(host), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e == hipSuccess && host) e = hipMemsetAsync(status, 0, sizeof(host), st);
    if (e != hipSuccess) {
        codlad_set_error("codlad_status_check: %s", hipGetErrorString(e));
        return (int)e;
    }
    if (host & CODLAD_STATUS_NONFINITE) {
        codlad_set_error("denoiser output is not finite: an input, a weight or - in the split-fp16 contraction "
                         "modes - an operand beyond the fp16 range (|x| > 65504) overflowed; rerun with precision f32 to tell them apart");
        return CODLAD_E_NONFINITE;
    }
    return 0;
}
