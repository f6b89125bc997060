// Arguments of the loss-evaluation kernels (loss_kernels.hip) and the launchers through which denoiser_forward.hip
// reaches them.  Host-side declarations only: no kernel of another unit sees this file's contents change its code.
#pragma once
#include "sampler_args.h"

#define CODLAD_LOSS_COLS 16     // columns of Tables.loss_coefficients (include/codlad_hip.h, codlad_vb_terms)

// Samples are node ranges [sample_off[s], sample_off[s + 1]); a sample's step is t_of_sample[s], or `t` for all when
// t_of_sample is null.  coef: device [T][CODLAD_LOSS_COLS].
struct LossSamples {
    const int32_t *sample_off;
    const int32_t *t_of_sample;
    int t, T, n_samples;
    const float *coef;
};

struct LossArgs {
    FinalArgs head;             // hV / mods / out_w / out_b / n_out / status / logits (optional copy of the model output)
    const float *model_out;     // stand-alone form: [n][6] or [n][3] instead of the head
    const float *x0, *xt;       // [n][3]
    const float *noise;         // [n][3] or null (then mse / eps_mse are not written)
    LossSamples s;
    codlad_loss_terms out;      // per-sample results, each may be null; pred_xstart [n][3]
};

// q_sample / q_mean_variance / q_posterior_mean_variance: out = coef[col_a] * a + coef[col_b] * b (b null: the first
// product alone); variance / log_variance (may be null) are filled with coef[col_var] / coef[col_logvar]
void launch_q_affine(const float *a, const float *b, int col_a, int col_b, int col_var, int col_logvar, const LossSamples &s,
                     float *out, float *variance, float *log_variance, hipStream_t st);
void launch_loss(const LossArgs &la, hipStream_t st);          // head form when la.model_out is null
// prior_bpd [n_samples]; total (may be null) = sum over i = T-1 .. 0 of vb[i][s], + prior_bpd[s]
void launch_prior(const float *x0, const LossSamples &s, const float *vb, float *prior_bpd, float *total_bpd, hipStream_t st);
