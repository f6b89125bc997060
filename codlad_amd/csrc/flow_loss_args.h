// Arguments of the flow-matching loss kernels (flow_loss_kernels.hip) and the launchers through which
// denoiser_forward.hip reaches them.  Host-side declarations only: no kernel of another unit sees this file's contents
// change its code.
#pragma once
#include "sampler_args.h"

// Samples are node ranges [sample_off[s], sample_off[s + 1]); a sample's time is t_of_sample[s] (device), or `t` for all
// when t_of_sample is null.
struct FmSamples {
    const int32_t *sample_off;
    const float *t_of_sample;
    float t;
    int n_samples;
};

// fm_path_kernel: the probability path of a matcher, xt and its conditional flow ut, each [n][3]
struct FmPathArgs {
    const float *x0, *x1, *eps;     // [n][3]; which may be null depends on the kind (include/codlad_hip.h)
    FmSamples s;
    int kind;                       // CODLAD_FM_*
    int noisy;                      // ICFM / VP: sigma != 0, the noise term is added
    float sigma_f;                  // (float)sigma
    float c;                        // TARGET: (float)(1.0 - sigma)
    float *xt, *ut;
};

struct FmLossArgs {
    FinalArgs head;                 // hV / mods / out_w / out_b / status / logits (optional copy of the model output)
    const float *model_out;         // stand-alone form: [n][3] instead of the head
    const float *ut;                // [n][3]
    const int32_t *sample_off;
    int n_samples;
    codlad_fm_loss_out out;         // per-sample means, each may be null
};

// What is wrong with a path request, or null.  t_of_sample / t as in FmSamples (device times are not read here).
const char *fm_path_defect(const float *x0, const float *x1, const float *eps, const float *t_of_sample, float t, int kind,
                           double sigma);
FmPathArgs fm_path_args(const float *x0, const float *x1, const float *eps, const FmSamples &s, int kind, double sigma,
                        float *xt, float *ut);
void launch_fm_path(const FmPathArgs &a, hipStream_t st);
void launch_fm_loss(const FmLossArgs &la, hipStream_t st);      // head form when la.model_out is null
