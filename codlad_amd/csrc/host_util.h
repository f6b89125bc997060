// What the translation units share on the HOST, declared once: the process-wide helpers of host_util.hip, two small inline
// helpers of the analysis entry points (subset_size, align256), the options
// (include/codlad_hip.h says what each means) and the launchers through which denoiser_forward.hip and the encoder reach
// the kernel units.  Kernels need none of this; their argument structs are in edge_args.h / node_args.h / sampler_args.h.
#pragma once
#include <hip/hip_runtime.h>
#include "../../include/codlad_hip.h"

struct EdgeArgs;
struct NodeArgs;
struct FinalArgs;

// host_util.hip
int num_cu();
void set_max_lds(const void *fn, size_t bytes);   // hipFuncSetAttribute; a failure is kept for the next codlad_check_launch
hipError_t codlad_take_attr_error();              // that failure, if any (read once)
int option_value(int opt);    // the value of CODLAD_OPT_<opt>: what codlad_set_option stored, else the environment's, else the default
int edge_cus();               // persistent workgroups of an edge kernel: num_cu() unless CODLAD_OPT_EDGE_CUS says fewer
// api.hip (declared in common.h too, beside codlad_check_launch): the message codlad_last_error returns
void codlad_set_error(const char *fmt, ...);
// a HIP call before a launch (memset, copy) failed: the message codlad_check_launch gives a failed launch, and its code
inline int codlad_hip_failed(const char *what, hipError_t e) {
    codlad_set_error("%s: %s", what, hipGetErrorString(e));
    return (int)e;
}
// the atoms a fit runs over: n_sel with a selection, all n_atoms without one; -1 when sel and n_sel disagree
inline int subset_size(const int32_t *sel, int n_sel, int n_atoms) {
    if (sel) return n_sel > 0 ? n_sel : -1;
    return n_sel == 0 ? n_atoms : -1;
}
// a byte count up to the next multiple of 256: where the next piece of a scratch buffer starts
inline size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }
// denoiser_forward.hip: every launcher below reports the grid it launches to the dispatch record (codlad_dispatch_read);
// node_kernel_h's also its waves per workgroup and whether it takes the XCD-chunked placement
void dispatch_note(int grid, int stream_waves = 0, bool chunked = false);

void launch_edge_f32(bool update, const EdgeArgs &ea, hipStream_t st);   // denoiser_f32_kernels.hip
void launch_node_f32(bool upd, const NodeArgs &na, hipStream_t st);
void launch_edge_tile(int terms, bool update, const EdgeArgs &ea, const int2 *tile_list, int n_tiles, hipStream_t st);   // edge_tile_kernels.hip
void launch_edge_wide(int terms, bool update, const EdgeArgs &ea, const int2 *tile_list, int n_tiles, hipStream_t st);   // edge_wide_kernels.hip
void launch_edge_msg(int terms, const EdgeArgs &ea, hipStream_t st);      // edge_msg_kernel.hip
void launch_edge_upd(int terms, const EdgeArgs &ea, hipStream_t st);      // edge_upd_kernel.hip
void launch_edge_upd1(int terms, const EdgeArgs &ea, hipStream_t st);     // edge_upd1_kernel.hip: one wave per SIMD
void launch_node_wide(int terms, bool upd, const NodeArgs &na, hipStream_t st);   // node_wide_kernels.hip
void launch_node_quad(int terms, const NodeArgs &na, hipStream_t st);             // node_quad_kernels.hip
void launch_node_stream(int terms, int waves, bool upd, const NodeArgs &na, hipStream_t st);   // node_stream_kernel.hip: waves = 4 or 8
// sampler_kernels.hip: final layer (+ the step's update unless fa.logits is set); step = CODLAD_STEP_*, pin_x0 null = no pinning
void launch_final(const FinalArgs &fa, int step, const float *pin_x0, const uint8_t *pin_mask, int mode, hipStream_t st);
void launch_tp_conv_mfma(const codlad_tp_conv_args &a, hipStream_t st);             // encoder_mfma_kernel.hip
void launch_tp_conv_pack(const codlad_tp_conv_args &a, void *image, hipStream_t st);
int tp_conv_image_bytes(int depth);
