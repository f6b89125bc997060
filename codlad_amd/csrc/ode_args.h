// Arguments of the fused ODE sampler's kernels (ode_kernels.hip) and the launchers through which denoiser_forward.hip
// reaches them.  Host-side declarations only: no kernel of another unit sees this file's contents change its code.
#pragma once
#include "sampler_args.h"

static_assert(sizeof(codlad_ode_state) == 96 && sizeof(codlad_ode_dopri5_bufs) == 13 * 8,
              "codlad_ode_state / codlad_ode_dopri5_bufs: the ctypes mirrors of _lib.py assume this layout");

// ode_stage_kernel: the final layer's velocity head on hV, then out = y + sum_m k[m] * (coef[m] * h), m < n_k in order.
struct OdeStageArgs : HeadArgs {     // mods: of the stage's time
    int *status;            // sticky status word or null (CODLAD_STATUS_NONFINITE)
    float *k_out;           // [n][3]: this stage's slope
    const float *y;         // [n][3]
    const float *k[7];      // the slopes in the order the stage sums them; entry `self` is this stage's own (not read)
    float coef[7];
    int n_k, self;          // self = -1: the stage's own slope is not in its sum
    float h;                // the step, unless ...
    const float *h_dev;     // ... this device word holds it (the adaptive method)
    float *out;             // [n][3]: the next stage's input, or the step's result
};

struct OdeNormArgs {
    const float *err;       // [n], or null: err = sum_m k[m] * (c_err[m] * h) over the seven slopes
    const float *y, *y1;
    const float *k[7];
    float c_err[7];
    const float *h_dev;
    size_t n;
    float rtol, atol;
    double *out;            // [CODLAD_ODE_NORM_WORDS]
    codlad_ode_state *state;    // the controller's block, or null: the norm alone
    const int *status;      // copied into the state (may be null)
};

void launch_ode_stage(const OdeStageArgs &a, hipStream_t st);
// the attempt's stage times, its step and xin = y + k1 * (beta0 * hh)
void launch_ode_times(codlad_ode_state *state, double t_end, float beta0, const float *y, const float *k1, float *xin,
                      size_t n, hipStream_t st);
void launch_ode_norm(const OdeNormArgs &a, hipStream_t st);      // both passes; the controller when a.state is set
void launch_ode_commit(const codlad_ode_state *state, float *y, const float *y1, float *k1, const float *k7, size_t n,
                       hipStream_t st);
