// Arguments of final_kernel (sampler_kernels.hip), filled by the loops of denoiser_forward.hip.
#pragma once
#include "final_head.h"    // HeadArgs; HD, host_util.h

// FinalLayer (latent_model.py:31-35) + ancestral DDPM update (gaussian_diffusion.py:303-367,446).
struct FinalArgs : HeadArgs {
    float *logits;      // [n][6] or null
    float *x;           // in/out [n][3] (update mode)
    const float *noise; // [n][3]
    const float *coef;  // device [8]
    float *x_start;     // [n][3] or null: pred_xstart of this step (self-conditioning input of the next)
    int *status;        // sticky status word or null (CODLAD_STATUS_NONFINITE)
    int n_out;          // 6 (eps | variance logits, diffusion) or 3 (velocity, flow matching: logits mode only)
};

// the update final_kernel applies: ddpm_step (mode: the table's column 7), ddim_step (the host's `mode`; reverse reads no noise)
// or dpm_step (DPM-Solver++(2M): no noise; x_start is required, read as the previous step's prediction and then written)
#define CODLAD_STEP_DDPM 0
#define CODLAD_STEP_DDIM 1
#define CODLAD_STEP_DDIM_REVERSE 2
#define CODLAD_STEP_DPM 3

static inline int mods_offset(int head) {  // enc0..2, dec0..2, final
    return head < 3 ? head * 9 * HD : (head < 6 ? 27 * HD + (head - 3) * 6 * HD : 45 * HD);
}
