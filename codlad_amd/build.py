"""Builds libcodlad_hip.so in-tree with hipcc for gfx950 (cross-compiles without a GPU).

    python -m codlad_amd.build [--force]
"""
import glob
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB = os.path.join(HERE, "libcodlad_hip.so")
SOURCES = ["api.hip", "host_util.hip", "edge_plan.hip", "denoiser_forward.hip", "denoiser_f32_kernels.hip", "node_stream_kernel.hip",
           "sampler_kernels.hip", "loss_kernels.hip", "flow_loss_kernels.hip", "edge_msg_kernel.hip", "edge_upd_kernel.hip", "edge_upd1_kernel.hip", "edge_tile_kernels.hip",
           "edge_wide_kernels.hip",
           "node_wide_kernels.hip", "node_quad_kernels.hip", "ode_kernels.hip", "features_kernels.hip", "decode_kernels.hip",
           "ic_decoder_kernels.hip", "encoder_kernels.hip", "encoder_mfma_kernel.hip", "metrics_kernels.hip", "ensemble_kernels.hip",
           "geometry_kernels.hip", "stereo_kernels.hip", "relax_kernels.hip", "observables_kernels.hip", "dssp_kernels.hip", "saxs_kernels.hip",
           "saxs_hydration_kernels.hip", "pair_hist_kernels.hip", "reweight_kernels.hip", "cluster_kernels.hip",
           "pca_kernels.hip", "compare_kernels.hip", "lddt_kernels.hip", "polymer_kernels.hip",
           "drmsd_kernels.hip", "torsion_kernels.hip"]
# Geometry / VQ kernels must round like the reference's unfused CPU ops (bit-exact neighbour lists
# and code indices): no implicit FMA contraction there; intended FMAs are written as fmaf().
EXTRA_FLAGS = {"features_kernels.hip": ["-ffp-contract=off"], "ode_kernels.hip": ["-ffp-contract=off"], "decode_kernels.hip": ["-ffp-contract=off"],
               "ic_decoder_kernels.hip": ["-ffp-contract=off"],
               # the loss terms round as the reference's unfused tensor ops; the head it shares with final_kernel asks for
               # contraction itself (final_head.h)
               "loss_kernels.hip": ["-ffp-contract=off"],
               "flow_loss_kernels.hip": ["-ffp-contract=off"],      # as loss_kernels.hip; the division stays the correctly rounded one
               # one sum order AND one rounding per operation in every kernel the shared fp64 code is inlined into: the
               # pairwise kernel returns the pair kernel's bits
               "ensemble_kernels.hip": ["-ffp-contract=off"],
               # distances round as bond_graph_kernel's and the clash term's of metrics_kernels.hip
               "geometry_kernels.hip": ["-ffp-contract=off"],
               # one rounding per operation, in the order the header states: the float32 restatement of the tests is the kernel's
               "stereo_kernels.hip": ["-ffp-contract=off"],
               # x' = x - fl32(h / gmax) * g is one multiply and one subtract, and the float32 restatement of the tests is the kernel's
               "relax_kernels.hip": ["-ffp-contract=off"],
               # every burial and contact decision is `fl32 < fl32` on values whose roundings the header states
               "observables_kernels.hip": ["-ffp-contract=off"],
               # both directions of a hydrogen bond round alike and as the header states: don is the transpose of acc
               "dssp_kernels.hip": ["-ffp-contract=off"],
               # the sine is a stated sequence of fp32 operations and the float64 sums have one order: the restatement is the kernel's
               "saxs_kernels.hip": ["-ffp-contract=off"],
               # the tt partial is saxs_kernels.hip's sequence and the fit is restated in numpy: one rounding per operation
               "saxs_hydration_kernels.hip": ["-ffp-contract=off"],
               # the bin of a pair is a stated sequence of fp32 operations and the float64 sums are restated in numpy
               "pair_hist_kernels.hip": ["-ffp-contract=off"],
               # one rounding per operation in every float64 sum; the covariance tile asks for its fused multiply-adds by name
               "reweight_kernels.hip": ["-ffp-contract=off"],
               # the per-pair tail of ensemble_math.h rounds as in ensemble_kernels.hip; the products are MFMA by name
               "cluster_kernels.hip": ["-ffp-contract=off"],
               # one rounding per operation in every float64 sum; the fused multiply-adds and the MFMA are asked for by name
               "pca_kernels.hip": ["-ffp-contract=off"],
               # the bin of a pair is pair_hist_kernels.hip's fp32 sequence; the float64 bin of a value and every divergence sum
               # are restated in numpy: one rounding per operation
               "compare_kernels.hip": ["-ffp-contract=off"],
               # distances round as geometry_kernels.hip's; every decision is `fl32 < fl32` and the float32 restatement is the kernel's
               "lddt_kernels.hip": ["-ffp-contract=off"],
               # the float64 sequence of a pair and the one order of every sum are the header's: one rounding per operation
               "polymer_kernels.hip": ["-ffp-contract=off"],
               # the fp32 distance is pair_hist_kernels.hip's sequence and every float64 sum has one order; the MFMA is asked for by name
               "drmsd_kernels.hip": ["-ffp-contract=off"],
               # the float64 feature sequence is restated in numpy to the bit and every sum has one order; the MFMA and the
               # fused multiply-adds of the mean are asked for by name
               "torsion_kernels.hip": ["-ffp-contract=off"],
               "metrics_kernels.hip": ["-ffp-contract=off"], "encoder_kernels.hip": ["-ffp-contract=off"],
               # the SLP vectoriser pairs multiply-adds of different result blocks into v_pk_fma_f32 and pays for it in register
               # moves (337 -> 80 v_mov at depth 0, 14 scratch accesses -> 0 at depth 2 without it)
               "encoder_mfma_kernel.hip": ["-ffp-contract=off", "-fno-slp-vectorize"],
               # SLP packing of the shuffle-reduction adds blocks their fusion into v_add_f32_dpp;
               # the packed math that pays (GELU) is written out explicitly in common.h
               # -fno-honor-nans: min/max on MFMA results otherwise get a canonicalising v_max x,x
               # each (3 instructions for min(|x|, c)); nothing on this path produces or tests NaN
               "denoiser_f32_kernels.hip": ["-fno-slp-vectorize", "-fno-honor-nans"],
               "node_stream_kernel.hip": ["-fno-slp-vectorize", "-fno-honor-nans"],
               "sampler_kernels.hip": ["-fno-slp-vectorize", "-fno-honor-nans"],     # final_kernel's non-finite test relies on it
               "edge_tile_kernels.hip": ["-fno-slp-vectorize", "-fno-honor-nans"],
               "edge_wide_kernels.hip": ["-fno-slp-vectorize", "-fno-honor-nans"],
               "edge_msg_kernel.hip": ["-fno-slp-vectorize", "-fno-honor-nans"],
               "edge_upd_kernel.hip": ["-fno-slp-vectorize", "-fno-honor-nans"],
               # one wave per SIMD: with a 512-register budget hipcc selects the AGPR form of every MFMA (accumulators in
               # AGPRs, ~450 v_accvgpr_read/write per tile around the vector work on them); the VGPR form keeps the
               # accumulators where GELU / LayerNorm read them, and the register-resident weights are placed in AGPRs by hand
               "edge_upd1_kernel.hip": ["-fno-slp-vectorize", "-fno-honor-nans", "-mllvm", "-amdgpu-mfma-vgpr-form=1"],
               "node_wide_kernels.hip": ["-fno-slp-vectorize", "-fno-honor-nans"],
               "node_quad_kernels.hip": ["-fno-slp-vectorize", "-fno-honor-nans"]}
HEADERS = sorted(glob.glob(os.path.join(CSRC, "*.h"))) + [os.path.join(HERE, "..", "include", "codlad_hip.h")]


def hipcc():
    for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", "hipcc"):
        if c and (os.path.isabs(c) and os.path.exists(c) or not os.path.isabs(c)):
            return c
    raise RuntimeError("hipcc not found")


RESOURCES = os.path.join(CSRC, "kernel_resources.json")


def record_resources(source, remarks):
    """Registers / scratch / occupancy hipcc reports per kernel (-Rpass-analysis=kernel-resource-usage), kept
    beside the objects: the edge kernels sit at the 256-register limit and a few spilled registers in their inner
    loops cost ~10 % (tests/test_host_logic.py holds them to their budget)."""
    import json
    import re
    table = {}
    if os.path.exists(RESOURCES):
        with open(RESOURCES) as f:
            table = json.load(f)
    # this source's old entries go, and those of sources that are no longer built (an experiment's leftovers would be
    # held to the budgets of kernels with similar names)
    table = {k: v for k, v in table.items() if v.get("source") != source and v.get("source") in SOURCES}
    cur = None
    for line in remarks.splitlines():
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            cur = table.setdefault(m.group(1), {"source": source})
            continue
        m = re.search(r"remark:\s+(TotalSGPRs|VGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|VGPRs Spill): (\d+)", line)
        if m and cur is not None:
            cur[m.group(1).split(" [")[0]] = int(m.group(2))
    with open(RESOURCES, "w") as f:
        json.dump(table, f, indent=0, sort_keys=True)


def stale():
    if not os.path.exists(LIB):
        return True
    t = os.path.getmtime(LIB)
    deps = [os.path.join(CSRC, s) for s in SOURCES] + HEADERS
    return any(os.path.getmtime(d) > t for d in deps)


def build(force=False, verbose=True):
    if not force and not stale():
        return LIB
    objs = []
    for s in SOURCES:
        src = os.path.join(CSRC, s)
        obj = os.path.join(CSRC, s.replace(".hip", ".o"))
        if force or not os.path.exists(obj) or os.path.getmtime(obj) < max(
                os.path.getmtime(d) for d in [src] + HEADERS):
            cmd = [hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC"] + EXTRA_FLAGS.get(s, []) + \
                  os.environ.get("CODLAD_CXXFLAGS", "").split() + \
                  ["-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", obj]
            if verbose:
                print(" ".join(cmd), flush=True)
            res = subprocess.run(cmd, stderr=subprocess.PIPE, text=True)
            if res.returncode:
                sys.stderr.write(res.stderr)
                raise subprocess.CalledProcessError(res.returncode, cmd)
            record_resources(s, res.stderr)
        objs.append(obj)
    cmd = [hipcc(), "--offload-arch=gfx950", "-shared", "-fPIC", "-o", LIB] + objs
    if verbose:
        print(" ".join(cmd), flush=True)
    subprocess.check_call(cmd)
    return LIB


if __name__ == "__main__":
    build(force="--force" in sys.argv)
    print(LIB)
