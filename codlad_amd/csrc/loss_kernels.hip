// Forward-only loss evaluation: the forward process (q_sample_kernel), the terms of the variational bound and the
// training losses per sample (loss_kernel: the final layer's head followed by the reference's _vb_terms_bpd arithmetic, or
// that arithmetic on a given model output) and the prior term (prior_kernel).  gaussian_diffusion.py:211-260, 549-725,
// diffusion_utils.py:10-88; the bound loop is the IDDPM release's calc_bpd_loop.
//
// Built with -ffp-contract=off: every product, sum and quotient below rounds separately, as the reference's elementwise
// tensor ops do.  The one exception is final_head (final_head.h), shared with final_kernel (sampler_kernels.hip, a unit
// built with contraction on): it asks for contraction itself.
//
// Reductions: one workgroup per sample, in the fixed order of sample_sum.h (shared with flow_loss_kernels.hip): it
// depends on the sample's length alone, not on the grid, not on what else shares the job, and no floating-point atomic
// is involved.
#include "loss_args.h"
#include "final_head.h"
#include "sample_sum.h"

// diffusion_utils.py:10-36, the sum in the reference's order
DEV float normal_kl(float mean1, float logvar1, float mean2, float logvar2) {
    const float d = mean1 - mean2;
    return 0.5f * ((((-1.0f + logvar2) - logvar1) + expf(logvar1 - logvar2)) + (d * d) * expf(-logvar2));
}

// diffusion_utils.py:39-44
DEV float approx_standard_normal_cdf(float x) {
    return 0.5f * (1.0f + tanhf(0.7978845608028654f * (x + 0.044715f * ((x * x) * x))));
}

// diffusion_utils.py:62-88
DEV float discretized_gaussian_log_likelihood(float x, float mean, float log_scale) {
    const float centered = x - mean;
    const float inv_stdv = expf(-log_scale);
    const float cdf_plus = approx_standard_normal_cdf(inv_stdv * (centered + (float)(1.0 / 255.0)));
    const float cdf_min = approx_standard_normal_cdf(inv_stdv * (centered - (float)(1.0 / 255.0)));
    const float log_cdf_plus = logf(fmaxf(cdf_plus, 1e-12f));
    const float log_one_minus_cdf_min = logf(fmaxf(1.0f - cdf_min, 1e-12f));
    const float cdf_delta = cdf_plus - cdf_min;
    return x < -0.999f ? log_cdf_plus : (x > 0.999f ? log_one_minus_cdf_min : logf(fmaxf(cdf_delta, 1e-12f)));
}

#define LOSS_KL 0
#define LOSS_NLL 1
#define LOSS_MSE 2
#define LOSS_XSTART 3
#define LOSS_EPS 4

// One element of _vb_terms_bpd / training_losses / calc_bpd_loop: o = the model's mean output, v = its variance logit
// (not read under the fixed-variance bit), cf = the step's row of Tables.loss_coefficients.  Returns pred_xstart.
DEV float loss_element(float o, float v, float x0, float xt, float noise, const float *cf, float (&term)[5]) {
    const int mode = (int)cf[7];
    const float logvar = ddpm_log_variance(v, cf);
    float pred = ddpm_raw_x0(xt, o, cf);
    if (mode & CODLAD_DDPM_CLIP) pred = fminf(fmaxf(pred, -1.0f), 1.0f);
    const float mean = cf[2] * pred + cf[3] * xt;
    const float true_mean = cf[2] * x0 + cf[3] * xt;
    term[LOSS_KL] = normal_kl(true_mean, cf[6], mean, logvar);
    term[LOSS_NLL] = -discretized_gaussian_log_likelihood(x0, mean, 0.5f * logvar);
    const float dm = ((mode & CODLAD_DDPM_START_X) ? x0 : noise) - o;     // training_losses: target - model_output
    term[LOSS_MSE] = dm * dm;
    const float dx = pred - x0;
    term[LOSS_XSTART] = dx * dx;
    const float de = (cf[0] * xt - pred) / cf[1] - noise;                 // _predict_eps_from_xstart, - noise
    term[LOSS_EPS] = de * de;
    return pred;
}

DEV const float *sample_coef(const LossSamples &s, int sample, int *t_out = nullptr) {
    int t = s.t_of_sample ? s.t_of_sample[sample] : s.t;
    t = t < 0 ? 0 : (t >= s.T ? s.T - 1 : t);                 // the host checks the range; never index outside the table
    if (t_out) *t_out = t;
    return s.coef + (size_t)t * CODLAD_LOSS_COLS;
}

template <bool HEAD>
__global__ __launch_bounds__(256) void loss_kernel(LossArgs a) {
    __shared__ float part[5][8];
    const int l = threadIdx.x & 31, hw = threadIdx.x >> 5;
    const int sample = blockIdx.x;
    const int first = a.s.sample_off[sample], end = a.s.sample_off[sample + 1];
    if (end <= first) return;                  // an empty (or reversed) range: nothing is read, nothing is written
    int t;
    const float *cf = sample_coef(a.s, sample, &t);
    const int width = ((int)cf[7] & CODLAD_DDPM_FIXED_VAR) ? 3 : 6;
    float acc[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
    for (int n0 = first; n0 < end; n0 += 8) {
        const int n = n0 + hw;
        const bool live = n < end;
        const int nc = live ? n : end - 1;                 // whole half waves stay converged for the shuffles
        float o[6];
        if constexpr (HEAD) {
            final_head(a.head, a.head.n_out, nc, l, o);
            if (live && a.head.status && l == 0 && any_nonfinite(o)) atomicOr(a.head.status, CODLAD_STATUS_NONFINITE);
            if (live && a.head.logits) store_logits(a.head.logits, a.head.n_out, n, l, o);
        } else {
#pragma unroll
            for (int k = 0; k < 6; ++k) o[k] = k < width ? a.model_out[(size_t)nc * width + k] : 0.f;
        }
        if (l < 3) {                                        // lane k: component k
            const float out = l == 0 ? o[0] : (l == 1 ? o[1] : o[2]);
            const float vv = l == 0 ? o[3] : (l == 1 ? o[4] : o[5]);
            const size_t i = (size_t)nc * 3 + l;
            float term[5];
            const float pred = loss_element(out, vv, a.x0[i], a.xt[i], a.noise ? a.noise[i] : 0.f, cf, term);
            if (live) {
#pragma unroll
                for (int q = 0; q < 5; ++q) acc[q] = acc[q] + term[q];
                if (a.out.pred_xstart) a.out.pred_xstart[i] = pred;
            }
        }
    }
    sample_sum<5>(acc, part);
    if (threadIdx.x == 0) {
        const float count = (float)((end - first) * 3);
        const float ln2 = 0.6931471805599453f;
        const float kl = (acc[LOSS_KL] / count) / ln2, nll = (acc[LOSS_NLL] / count) / ln2;
        if (a.out.kl) a.out.kl[sample] = kl;
        if (a.out.nll) a.out.nll[sample] = nll;
        if (a.out.vb) a.out.vb[sample] = t == 0 ? nll : kl;
        if (a.out.mse && a.noise) a.out.mse[sample] = acc[LOSS_MSE] / count;
        if (a.out.xstart_mse) a.out.xstart_mse[sample] = acc[LOSS_XSTART] / count;
        if (a.out.eps_mse && a.noise) a.out.eps_mse[sample] = acc[LOSS_EPS] / count;
    }
}

void launch_loss(const LossArgs &la, hipStream_t st) {
    hipLaunchKernelGGL(la.model_out ? loss_kernel<false> : loss_kernel<true>, dim3(la.s.n_samples), dim3(256), 0, st, la);
}

// out = cf[col_a] * a + cf[col_b] * b per element of the sample, cf = the row of the sample's step (b null: cf[col_a] * a);
// variance / log_variance (optional) = cf[col_var] / cf[col_logvar], broadcast as _extract_into_tensor does.
__global__ __launch_bounds__(256) void q_sample_kernel(const float *a, const float *b, int col_a, int col_b, int col_var,
                                                       int col_logvar, LossSamples s, float *out, float *variance,
                                                       float *log_variance) {
    const int sample = blockIdx.x;
    const float *cf = sample_coef(s, sample);
    const float ca = cf[col_a], cb = cf[col_b], cv = cf[col_var], cl = cf[col_logvar];
    const int end = s.sample_off[sample + 1] * 3;
    for (int i = s.sample_off[sample] * 3 + threadIdx.x; i < end; i += 256) {
        out[i] = b ? ca * a[i] + cb * b[i] : ca * a[i];
        if (variance) variance[i] = cv;
        if (log_variance) log_variance[i] = cl;
    }
}

void launch_q_affine(const float *a, const float *b, int col_a, int col_b, int col_var, int col_logvar, const LossSamples &s,
                     float *out, float *variance, float *log_variance, hipStream_t st) {
    hipLaunchKernelGGL(q_sample_kernel, dim3(s.n_samples), dim3(256), 0, st, a, b, col_a, col_b, col_var, col_logvar, s, out,
                       variance, log_variance);
}

// KL(q(x_{T-1} | x_0) || N(0, 1)) per sample in bits per dimension (the IDDPM release's _prior_bpd), and the total bound
__global__ __launch_bounds__(256) void prior_kernel(const float *x0, LossSamples s, const float *vb, float *prior_bpd,
                                                    float *total_bpd) {
    __shared__ float part[1][8];
    const int l = threadIdx.x & 31, hw = threadIdx.x >> 5;
    const int sample = blockIdx.x;
    const int first = s.sample_off[sample], end = s.sample_off[sample + 1];
    if (end <= first) return;
    const float *cf = s.coef + (size_t)(s.T - 1) * CODLAD_LOSS_COLS;
    float acc[1] = {0.f};
    for (int n = first + hw; n < end; n += 8)
        if (l < 3) acc[0] = acc[0] + normal_kl(cf[8] * x0[(size_t)n * 3 + l], cf[11], 0.0f, 0.0f);
    sample_sum<1>(acc, part);
    if (threadIdx.x == 0) {
        const float prior = (acc[0] / (float)((end - first) * 3)) / 0.6931471805599453f;
        prior_bpd[sample] = prior;
        if (total_bpd) {
            float sum = vb[(size_t)(s.T - 1) * s.n_samples + sample];
            for (int i = s.T - 2; i >= 0; --i) sum = sum + vb[(size_t)i * s.n_samples + sample];
            total_bpd[sample] = sum + prior;
        }
    }
}

void launch_prior(const float *x0, const LossSamples &s, const float *vb, float *prior_bpd, float *total_bpd, hipStream_t st) {
    hipLaunchKernelGGL(prior_kernel, dim3(s.n_samples), dim3(256), 0, st, x0, s, vb, prior_bpd, total_bpd);
}

// ---------------------------------------------------------------------------------------------
// stand-alone entries (the ones around a denoiser forward are in denoiser_forward.hip)
// ---------------------------------------------------------------------------------------------
#define LOSS_SAMPLES_REQUIRE()                                                                         \
    CODLAD_REQUIRE(coef && sample_off, "null pointer");                                                \
    CODLAD_REQUIRE(T > 0 && n_samples > 0, "T and n_samples must be positive");                        \
    CODLAD_REQUIRE(t_of_sample || (t >= 0 && t < T), "t outside [0, T)")

extern "C" int codlad_q_sample(const float *x_start, const float *noise, const float *coef, int T, const int32_t *sample_off,
                               int n_samples, const int32_t *t_of_sample, int t, float *x_t, float *variance,
                               float *log_variance, void *stream) {
    CODLAD_REQUIRE(x_start && x_t, "null pointer");
    LOSS_SAMPLES_REQUIRE();
    const LossSamples s = {sample_off, t_of_sample, t, T, n_samples, coef};
    launch_q_affine(x_start, noise, 8, 9, 10, 11, s, x_t, variance, log_variance, (hipStream_t)stream);
    return codlad_check_launch("codlad_q_sample");
}

extern "C" int codlad_q_posterior(const float *x_start, const float *x_t, const float *coef, int T, const int32_t *sample_off,
                                  int n_samples, const int32_t *t_of_sample, int t, float *mean, float *variance,
                                  float *log_variance, void *stream) {
    CODLAD_REQUIRE(x_start && x_t && mean, "null pointer");
    LOSS_SAMPLES_REQUIRE();
    const LossSamples s = {sample_off, t_of_sample, t, T, n_samples, coef};
    launch_q_affine(x_start, x_t, 2, 3, 12, 6, s, mean, variance, log_variance, (hipStream_t)stream);
    return codlad_check_launch("codlad_q_posterior");
}

extern "C" int codlad_vb_terms(const float *model_out, const float *x_start, const float *x_t, const float *noise,
                               const float *coef, int T, const int32_t *sample_off, int n_samples, const int32_t *t_of_sample,
                               int t, const codlad_loss_terms *terms, void *stream) {
    CODLAD_REQUIRE(model_out && x_start && x_t && terms, "null pointer");
    LOSS_SAMPLES_REQUIRE();
    LossArgs la = {};
    la.model_out = model_out; la.x0 = x_start; la.xt = x_t; la.noise = noise;
    la.s = {sample_off, t_of_sample, t, T, n_samples, coef};
    la.out = *terms;
    launch_loss(la, (hipStream_t)stream);
    return codlad_check_launch("codlad_vb_terms");
}

extern "C" int codlad_prior_bpd(const float *x_start, const float *coef, int T, const int32_t *sample_off, int n_samples,
                                float *prior_bpd, void *stream) {
    CODLAD_REQUIRE(x_start && prior_bpd, "null pointer");
    const int32_t *t_of_sample = nullptr;
    const int t = 0;
    LOSS_SAMPLES_REQUIRE();
    const LossSamples s = {sample_off, nullptr, T - 1, T, n_samples, coef};
    launch_prior(x_start, s, nullptr, prior_bpd, nullptr, (hipStream_t)stream);
    return codlad_check_launch("codlad_prior_bpd");
}
