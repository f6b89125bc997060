// The tile accounting of the per-node edge kernels on the host (codlad_edge_plan_host): the chunk bounds the kernels
// walk by and what the walk costs, from the same helpers (edge_args.h) the kernels decide with.  Host only.
#include "edge_args.h"
#include <vector>

// Tiles the waves of one XCD run on nodes lo .. hi - 1 (wave w: lo + w, lo + w + stride, ...), and the pairs they form.
static int64_t chunk_walk(const int32_t *K, int lo, int hi, int stride, bool pair, int64_t *pairs) {
    int64_t tiles = 0;
    for (int w = 0; w < stride; ++w)
        for (int n = lo + w; n < hi; n += stride) {
            tiles += K[n] > 32 ? 2 : 1;
            if (pair && n + stride < hi && edge_pair_ok(K[n], K[n + stride])) {
                n += stride;                     // the second node: its tiles, less the one the two share
                tiles += (K[n] > 32 ? 2 : 1) - 1;
                if (pairs) ++*pairs;
            }
        }
    return tiles;
}

extern "C" int codlad_edge_plan_host(const int32_t *K_host, int n_nodes, int n_workgroups, int waves_per_workgroup,
                                     int pair, int32_t *bounds_host, int64_t *stats_host) {
    CODLAD_REQUIRE(K_host && n_nodes > 0 && n_workgroups > 0 && waves_per_workgroup > 0, "bad arguments");
    int32_t bounds[9];
    const int G = XCD_BOUND_GRANULE, ng = (n_nodes + G - 1) / G;
    std::vector<int64_t> upto(ng + 1, 0);       // half tiles of the cost model up to each granule boundary
    int64_t plain = 0;
    for (int n = 0; n < n_nodes; ++n) {
        CODLAD_REQUIRE(K_host[n] >= 1 && K_host[n] <= 64, "K outside 1..64");
        plain += K_host[n] > 32 ? 2 : 1;
        upto[n / G + 1] += pair ? edge_node_cost2(K_host[n]) : (K_host[n] > 32 ? 4 : 2);
    }
    for (int g = 0; g < ng; ++g) upto[g + 1] += upto[g];
    const int64_t total = upto[ng];
    const bool chunked = n_workgroups % 8 == 0;
    const int stride = chunked ? n_workgroups / 8 * waves_per_workgroup : n_workgroups * waves_per_workgroup;
    auto node_of = [&](int g) { return g * G < n_nodes ? g * G : n_nodes; };
    if (pair) {
        // Bound x: the granule boundary where the tiles walked so far are nearest to x eighths of the total, so that a
        // chunk misses the mean by less than one granule.  What a chunk costs is what its waves walk: a wave pairs the
        // eligible nodes it meets in a row and an odd one out costs two tiles, not the 1.5 of the cost model, which
        // therefore only gives the first guess (and the whole answer for a grid that is not dealt over the XCDs).
        double target = total / 16.0;
        for (int pass = 0; pass < (chunked ? 3 : 1); ++pass) {
            bounds[0] = 0;
            int g = 0;
            int64_t done = 0;               // tiles of the chunks closed so far
            for (int x = 1; x < 8; ++x) {
                const int g0 = g;
                if (pass == 0) {
                    while (g < ng && 8 * upto[g + 1] <= total * x) ++g;          // upto[g] <= target < upto[g + 1]
                    if (g < ng && 8 * upto[g + 1] - total * x < total * x - 8 * upto[g]) ++g;
                } else {
                    auto f = [&](int gg) { return (double)(done + chunk_walk(K_host, node_of(g0), node_of(gg), stride, true, nullptr)); };
                    const double want = target * x;
                    while (g < ng && f(g) < want) ++g;
                    while (g > g0 && f(g - 1) >= want) --g;                     // f(g - 1) < want <= f(g)
                    if (g > g0 && want - f(g - 1) < f(g) - want) --g;
                }
                bounds[x] = node_of(g);
                if (chunked) done += chunk_walk(K_host, node_of(g0), node_of(g), stride, true, nullptr);
            }
            bounds[8] = n_nodes;
            if (chunked) target = (done + chunk_walk(K_host, bounds[7], n_nodes, stride, true, nullptr)) / 8.0;
        }
    } else {
        const int chunk = xcd_chunk_nodes(n_nodes);
        for (int x = 0; x <= 8; ++x) bounds[x] = (int64_t)x * chunk < n_nodes ? x * chunk : n_nodes;
    }
    if (bounds_host)
        for (int x = 0; x <= 8; ++x) bounds_host[x] = bounds[x];
    if (stats_host) {
        int64_t walk = 0, pairs = 0;
        for (int x = 0; x < 8; ++x) {
            const int lo = (bounds[x] + G - 1) / G, hi = (bounds[x + 1] + G - 1) / G;
            stats_host[4 + x] = upto[hi] - upto[lo];
            stats_host[12 + x] = chunked ? chunk_walk(K_host, bounds[x], bounds[x + 1], stride, pair != 0, &pairs) : 0;
            walk += stats_host[12 + x];
        }
        if (!chunked) walk = chunk_walk(K_host, 0, n_nodes, stride, pair != 0, &pairs);
        stats_host[0] = plain;
        stats_host[1] = total;
        stats_host[2] = walk;
        stats_host[3] = pairs;
    }
    return 0;
}
