// Forward-only loss evaluation of the flow-matching models: the probability path of a conditional flow matcher
// (fm_path_kernel: xt and the conditional flow ut) and the regression losses per sample (fm_loss_kernel: the final
// layer's velocity head followed by the reference's loss_fn arithmetic, or that arithmetic on a given model output).
// diffusion_and_flow/flow.py (ConditionalFlowMatcher, TargetConditionalFlowMatcher,
// VariancePreservingConditionalFlowMatcher), utils/train_module.py loss_fn.
//
// Built with -ffp-contract=off: every product, sum and quotient below rounds separately, as the reference's elementwise
// tensor ops do, and the division is the correctly rounded one (no flag relaxes it for this unit).  The one exception is
// final_head (final_head.h), shared with final_kernel (sampler_kernels.hip, a unit built with contraction on): it asks
// for contraction itself.
//
// Reductions: one workgroup per sample, in the fixed order of sample_sum.h (loss_kernel's): a sample's bits depend on its
// length alone.
#include "flow_loss_args.h"
#include "final_head.h"
#include "sample_sum.h"

// One workgroup per sample; the sample's time is uniform over it.
__global__ __launch_bounds__(256) void fm_path_kernel(FmPathArgs a) {
    const int sample = blockIdx.x;
    const float t = a.s.t_of_sample ? a.s.t_of_sample[sample] : a.s.t;
    const int end = a.s.sample_off[sample + 1] * 3;
    if (a.kind == CODLAD_FM_ICFM) {
        const float omt = 1.0f - t;
        for (int i = a.s.sample_off[sample] * 3 + threadIdx.x; i < end; i += 256) {
            const float x0 = a.x0[i], x1 = a.x1[i];
            const float mu = t * x1 + omt * x0;                         // compute_mu_t
            a.xt[i] = a.noisy ? mu + a.sigma_f * a.eps[i] : mu;         // sample_xt; sigma = 0: + 0, skipped
            a.ut[i] = x1 - x0;
        }
    } else if (a.kind == CODLAD_FM_TARGET || a.kind == CODLAD_FM_TARGET_FLOW) {
        const bool given = a.kind == CODLAD_FM_TARGET_FLOW;             // compute_conditional_flow alone, of a given xt
        const float ct = a.c * t;
        const float sigma_t = 1.0f - ct;                                // compute_sigma_t: 1 - (1 - sigma) * t
        for (int i = a.s.sample_off[sample] * 3 + threadIdx.x; i < end; i += 256) {
            const float x1 = a.x1[i];
            const float xt = given ? a.xt[i] : t * x1 + sigma_t * a.eps[i];
            if (!given) a.xt[i] = xt;
            a.ut[i] = (x1 - a.c * xt) / sigma_t;                        // (x1 - (1 - sigma) xt) / (1 - (1 - sigma) t)
        }
    } else {
        const float h = (float)(3.14159265358979323846 / 2);
        const float ht = h * t;
        const float cs = cosf(ht), sn = sinf(ht);
        for (int i = a.s.sample_off[sample] * 3 + threadIdx.x; i < end; i += 256) {
            const float x0 = a.x0[i], x1 = a.x1[i];
            const float mu = cs * x0 + sn * x1;
            a.xt[i] = a.noisy ? mu + a.sigma_f * a.eps[i] : mu;
            a.ut[i] = h * (cs * x1 - sn * x0);
        }
    }
}

#define FM_L2 0
#define FM_L1 1
#define FM_HUBER 2
#define FM_SMOOTH_L1 3
#define FM_LOG_COSH 4

template <bool HEAD>
__global__ __launch_bounds__(256) void fm_loss_kernel(FmLossArgs a) {
    __shared__ float part[5][8];
    const int l = threadIdx.x & 31, hw = threadIdx.x >> 5;
    const int sample = blockIdx.x;
    const int first = a.sample_off[sample], end = a.sample_off[sample + 1];
    if (end <= first) return;                  // an empty (or reversed) range: nothing is read, nothing is written
    float acc[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
    for (int n0 = first; n0 < end; n0 += 8) {
        const int n = n0 + hw;
        const bool live = n < end;
        const int nc = live ? n : end - 1;                 // whole half waves stay converged for the shuffles
        float o[3] = {0.f, 0.f, 0.f};
        if constexpr (HEAD) {
            final_head(a.head, 3, nc, l, o);
            if (live && a.head.status && l == 0 && any_nonfinite(o)) atomicOr(a.head.status, CODLAD_STATUS_NONFINITE);
        }
        if (l < 3) {                                        // lane k: component k
            const size_t i = (size_t)nc * 3 + l;
            float vt;
            if constexpr (HEAD) {
                vt = l == 0 ? o[0] : (l == 1 ? o[1] : o[2]);
                if (live && a.head.logits) a.head.logits[i] = vt;
            } else {
                vt = a.model_out[i];
            }
            const float d = vt - a.ut[i];
            const float ad = fabsf(d), dd = d * d;
            const float hub = ad < 1.0f ? 0.5f * dd : ad - 0.5f;        // delta = beta = 1: huber and smooth_l1 coincide
            const float lc = logf(coshf(d));
            if (live) {
                acc[FM_L2] = acc[FM_L2] + dd;
                acc[FM_L1] = acc[FM_L1] + ad;
                acc[FM_HUBER] = acc[FM_HUBER] + hub;
                acc[FM_SMOOTH_L1] = acc[FM_SMOOTH_L1] + hub;
                acc[FM_LOG_COSH] = acc[FM_LOG_COSH] + lc;
            }
        }
    }
    sample_sum<5>(acc, part);
    if (threadIdx.x == 0) {
        const float count = (float)((end - first) * 3);
        if (a.out.l2) a.out.l2[sample] = acc[FM_L2] / count;
        if (a.out.l1) a.out.l1[sample] = acc[FM_L1] / count;
        if (a.out.huber) a.out.huber[sample] = acc[FM_HUBER] / count;
        if (a.out.smooth_l1) a.out.smooth_l1[sample] = acc[FM_SMOOTH_L1] / count;
        if (a.out.log_cosh) a.out.log_cosh[sample] = acc[FM_LOG_COSH] / count;
    }
}

void launch_fm_path(const FmPathArgs &a, hipStream_t st) {
    hipLaunchKernelGGL(fm_path_kernel, dim3(a.s.n_samples), dim3(256), 0, st, a);
}

void launch_fm_loss(const FmLossArgs &la, hipStream_t st) {
    hipLaunchKernelGGL(la.model_out ? fm_loss_kernel<false> : fm_loss_kernel<true>, dim3(la.n_samples), dim3(256), 0, st, la);
}

const char *fm_path_defect(const float *x0, const float *x1, const float *eps, const float *t_of_sample, float t, int kind,
                           double sigma) {
    if (kind != CODLAD_FM_ICFM && kind != CODLAD_FM_TARGET && kind != CODLAD_FM_VP && kind != CODLAD_FM_TARGET_FLOW)
        return "unknown matcher kind";
    if (!(sigma >= 0.0)) return "sigma must not be negative";
    if (!t_of_sample && !(t >= 0.0f && t <= 1.0f)) return "t outside [0, 1]";
    if (!x1) return "null pointer (x1)";
    const bool target = kind == CODLAD_FM_TARGET || kind == CODLAD_FM_TARGET_FLOW;
    if (!target && !x0) return "null pointer (x0: only the target matcher runs without it)";
    if (kind == CODLAD_FM_TARGET_FLOW) return nullptr;                  // reads x1 and the given xt alone
    if (target ? !eps : (sigma != 0.0 && !eps)) return "null pointer (eps: only sigma = 0 runs without it)";
    return nullptr;
}

FmPathArgs fm_path_args(const float *x0, const float *x1, const float *eps, const FmSamples &s, int kind, double sigma,
                        float *xt, float *ut) {
    FmPathArgs a = {};
    a.x0 = x0; a.x1 = x1; a.eps = eps; a.s = s; a.kind = kind;
    a.noisy = sigma != 0.0;
    a.sigma_f = (float)sigma;
    a.c = (float)(1.0 - sigma);
    a.xt = xt; a.ut = ut;
    return a;
}

// ---------------------------------------------------------------------------------------------
// stand-alone entries (the ones around a denoiser forward are in denoiser_forward.hip)
// ---------------------------------------------------------------------------------------------
extern "C" int codlad_fm_path(const float *x0, const float *x1, const float *eps, const int32_t *sample_off, int n_samples,
                              const float *t_of_sample, float t, int kind, double sigma, float *xt, float *ut, void *stream) {
    CODLAD_REQUIRE(sample_off && xt && ut, "null pointer");
    CODLAD_REQUIRE(n_samples > 0, "n_samples must be positive");
    if (const char *msg = fm_path_defect(x0, x1, eps, t_of_sample, t, kind, sigma)) CODLAD_REQUIRE(false, msg);
    launch_fm_path(fm_path_args(x0, x1, eps, {sample_off, t_of_sample, t, n_samples}, kind, sigma, xt, ut),
                   (hipStream_t)stream);
    return codlad_check_launch("codlad_fm_path");
}

extern "C" int codlad_fm_terms(const float *model_out, const float *ut, const int32_t *sample_off, int n_samples,
                               const codlad_fm_loss_out *terms, void *stream) {
    CODLAD_REQUIRE(model_out && ut && sample_off && terms, "null pointer");
    CODLAD_REQUIRE(n_samples > 0, "n_samples must be positive");
    FmLossArgs la = {};
    la.model_out = model_out; la.ut = ut; la.sample_off = sample_off; la.n_samples = n_samples;
    la.out = *terms;
    launch_fm_loss(la, (hipStream_t)stream);
    return codlad_check_launch("codlad_fm_terms");
}
