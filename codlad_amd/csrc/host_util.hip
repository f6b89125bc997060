// Process-wide host state shared by every kernel unit (host_util.h): the CU count, the latch for a failed LDS-limit
// attribute and the run-time options.  Host only.
#include "host_util.h"
#include "common.h"
#include <stdlib.h>

int num_cu() {
    static int n_cu = 0;
    if (!n_cu) {
        int dev = 0, n = 0;
        if (hipGetDevice(&dev) != hipSuccess ||
            hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0)
            n = 256;
        n_cu = n;
    }
    return n_cu;
}

// Raising a kernel's dynamic-LDS limit can fail (e.g. a device with less LDS than gfx950's 160 KB); the
// launch that follows would then fail with a less telling error, so the failure is kept for
// codlad_check_launch to report.
static hipError_t g_attr_error = hipSuccess;
void set_max_lds(const void *fn, size_t bytes) {
    const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (e != hipSuccess && g_attr_error == hipSuccess) g_attr_error = e;
}
hipError_t codlad_take_attr_error() {
    const hipError_t e = g_attr_error;
    g_attr_error = hipSuccess;
    return e;
}

// One row per CODLAD_OPT_*, in the header's order: an option is what codlad_set_option stored, else its environment
// variable, else its default - settled at first use, so that a default may ask for the CU count.
struct Option {
    int id;             // CODLAD_OPT_*: the row's own index
    const char *env;
    int (*dflt)();
    int value = -1;     // < 0: not settled yet
};
static Option g_options[] = {
    // jobs of up to this many 32-node tiles take the wide kernel (one tile per 8-wave workgroup)
    {CODLAD_OPT_NODEQ_MAX_TILES, "CODLAD_NODEQ_MAX_TILES", [] { return 256; }},
    {CODLAD_OPT_EDGE_TILE_MAX_NODES, "CODLAD_EDGE_TILE_MAX_NODES", [] { return 1 << 30; }},
    // measured: 87 nodes 202 -> 182 us per step, the cfg-3 shard 476 -> 448, all of cfg 3 (411 tiles, two rounds) 2 316 -> 2 281;
    // cfg 2's half-jobs (553 tiles) lose 1.3 % against the streaming kernel, which reads every block once per 4-8 tiles
    {CODLAD_OPT_NODE_QUAD_MAX_TILES, "CODLAD_NODE_QUAD_MAX_TILES", [] { return 2 * num_cu(); }},
    {CODLAD_OPT_DEC_EDGE_VARIANT, "CODLAD_DEC_EDGE_VARIANT", [] { return 0; }},
    {CODLAD_OPT_TP_CONV_VARIANT, "CODLAD_TP_CONV_VARIANT", [] { return 0; }},
    {CODLAD_OPT_EDGE_UPD_VARIANT, "CODLAD_EDGE_UPD_VARIANT", [] { return 0; }},
    {CODLAD_OPT_EDGE_CUS, "CODLAD_EDGE_CUS", [] { return 0; }},
    // measured (tools/small_job_latency.py --sweep, k x 87 residues): the four-wave tile kernels win or tie up to ~5 600 tiles
    // (2 800 nodes; 87 nodes 375 -> 254 us per step, 1 914 nodes 764 -> 594), beyond that the per-node kernels' reuse wins
    {CODLAD_OPT_EDGE_WIDE_MAX_TILES, "CODLAD_EDGE_WIDE_MAX_TILES", [] { return 22 * num_cu(); }},
    // paired last tiles and cost-balanced XCD chunks in msg_kernel_h / upd_kernel_h (edge_args.h); 0: every node on its own, uniform chunks
    {CODLAD_OPT_EDGE_PAIR, "CODLAD_EDGE_PAIR", [] { return 1; }},
};
static_assert(sizeof(g_options) / sizeof(g_options[0]) == CODLAD_N_OPTIONS, "one row per CODLAD_OPT_*");

int option_value(int opt) {
    Option &o = g_options[opt];
    if (o.id != opt) abort();       // a row out of the header's order
    if (o.value < 0) {
        const char *e = getenv(o.env);
        o.value = e ? atoi(e) : o.dflt();
    }
    return o.value;
}

extern "C" int codlad_set_option(int option, int value) {
    CODLAD_REQUIRE(option >= 0 && option < CODLAD_N_OPTIONS && value >= 0, "unknown option or negative value");
    g_options[option].value = value;
    return 0;
}

int edge_cus() {
    const int v = option_value(CODLAD_OPT_EDGE_CUS);
    return v > 0 && v < num_cu() ? v : num_cu();
}
