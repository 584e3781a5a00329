// clean.cpp -- edge cleaning: the C ABI around clean.hip's kernels, and the host-only rule ookd_clean_edges
// (include/ookiedokie_amd.h states the rule as a contract).
#include <algorithm>
#include <cstring>
#include <new>
#include <vector>

#include "clean.hpp"

using namespace ookd;

namespace ookd {

struct CleanCtx : EdgePass {
    uint64_t *d_out = nullptr;          // the cleaned list
    uint64_t out_capacity = 0;          // elements of it (grown, never shrunk)
    uint32_t *d_prefix = nullptr;       // [prefix_capacity]
    uint32_t prefix_capacity = 0;
    CleanAgg *d_agg = nullptr;          // [tiles]
    CleanCarry *d_carry = nullptr;      // [tiles]
    uint64_t tiles = 0;
    // of run `serial`
    uint64_t min_on = 0, min_off = 0;
    uint32_t captures = 0;
    std::vector<uint64_t> host;         // [captures][kCleanWords]
    std::vector<uint64_t> prefix;       // [captures + 1]: the cleaned prefix, from the counts

    ~CleanCtx() override {
        if (d_out) (void)hipFree(d_out);
        if (d_prefix) (void)hipFree(d_prefix);
        if (d_agg) (void)hipFree(d_agg);
        if (d_carry) (void)hipFree(d_carry);
    }
};

}  // namespace ookd

namespace {

template <typename T>
bool grow(T *&p, uint64_t want) {
    if (p) (void)hipFree(p);
    p = nullptr;
    return hipMalloc(reinterpret_cast<void **>(&p), (size_t)want * sizeof(T)) == hipSuccess;
}

// the buffers a run of run.num_edges edges in run.captures captures needs
int reserve(CleanCtx &c, const EdgeRun &run) {
    if (hipSetDevice(run.dev) != hipSuccess) {
        set_error("ookd_rx_clean_edges: hipSetDevice failed");
        return OOKD_ERR_HIP;
    }
    const uint64_t edges = std::max<uint64_t>(run.num_edges, 1u), tiles = clean_tiles_of(run.num_edges, run.captures);
    bool ok = true;
    if (c.out_capacity < edges) {
        c.out_capacity = 0;
        ok = grow(c.d_out, edges);
        if (ok) c.out_capacity = edges;
    }
    if (ok && c.tiles < tiles) {
        c.tiles = 0;
        ok = grow(c.d_agg, tiles) && grow(c.d_carry, tiles);
        if (ok) c.tiles = tiles;
    }
    if (ok && c.prefix_capacity < run.captures + 1u) {
        c.prefix_capacity = 0;
        ok = grow(c.d_prefix, run.captures + 1u);
        if (ok) c.prefix_capacity = run.captures + 1u;
    }
    if (!ok) {
        set_error("ookd_rx_clean_edges: device allocation failed: %s", hipGetErrorString(hipGetLastError()));
        return OOKD_ERR_NOMEM;
    }
    return OOKD_OK;
}

// the context's clean pass when it has answered the context's last run, else null
const CleanCtx *answered(const ookd_rx *rx) {
    EdgeRun run;
    ookd_rx_edge_run(rx, &run);
    const CleanCtx *c = static_cast<const CleanCtx *>(ookd_rx_edge_pass(const_cast<ookd_rx *>(rx), kEdgePassClean).get());
    return c && run.serial != 0 && c->serial == run.serial ? c : nullptr;
}

}  // namespace

namespace ookd {

bool clean_run_view(ookd_rx *rx, EdgeRun &run) {
    const CleanCtx *c = static_cast<const CleanCtx *>(ookd_rx_edge_pass(rx, kEdgePassClean).get());
    if (!c || run.serial == 0 || c->serial != run.serial) return false;
    run.d_edges = c->d_out;
    run.edge_capacity = c->out_capacity;
    run.d_blk_offset = c->d_prefix;
    run.blocks_per_cap = 1;
    run.num_edges = c->prefix.empty() ? 0 : c->prefix.back();
    return true;
}

}  // namespace ookd

extern "C" {

int ookd_clean_edges(const uint64_t *edges, uint64_t E, uint64_t min_on, uint64_t min_off, uint64_t *out, uint64_t capacity,
                     uint64_t *num_out) {
    clear_error();
    if (!edges && E) {
        set_error("ookd_clean_edges: NULL argument");
        return OOKD_ERR_ARG;
    }
    const uint64_t min_len[2] = {min_off, min_on};
    uint64_t n = 0;
    bool before = false;                // d(i - 1)
    for (uint64_t i = 0; i < E; ++i) {
        // run i is closed for i < E - 1, and "on" when i is even
        const bool d = i + 1 < E && edges[i + 1] - edges[i] < min_len[(i & 1u) ^ 1u] && !before;
        if (!d && !before) {
            if (out && n < capacity) out[n] = edges[i];
            ++n;
        }
        before = d;
    }
    if (num_out) *num_out = n;
    return OOKD_OK;
}

int ookd_rx_clean_edges(ookd_rx *rx, uint64_t min_on, uint64_t min_off) {
    clear_error();
    if (!rx) {
        set_error("ookd_rx_clean_edges: NULL argument");
        return OOKD_ERR_ARG;
    }
    EdgeRun run;
    if (const int rc = edge_run_check("ookd_rx_clean_edges", rx, 0, run); rc != OOKD_OK) return rc;
    std::unique_ptr<EdgePass> &slot = ookd_rx_edge_pass(rx, kEdgePassClean);
    if (!slot) slot.reset(new (std::nothrow) CleanCtx());
    CleanCtx *ctx = static_cast<CleanCtx *>(slot.get());
    if (!ctx) {
        set_error("ookd_rx_clean_edges: out of memory");
        return OOKD_ERR_NOMEM;
    }
    if (ctx->serial == run.serial && ctx->min_on == min_on && ctx->min_off == min_off) return OOKD_OK;
    // another list from here on: what the clean readers keep is about the one before
    for (EdgePassId id : {kEdgePassCleanPulse, kEdgePassCleanSymbol}) {
        if (EdgePass *reader = ookd_rx_edge_pass(rx, id).get()) {
            reader->serial = 0;
            reader->kernel_ms = 0.0f;
        }
    }
    ctx->serial = 0;
    ctx->kernel_ms = 0.0f;
    ctx->host.assign((size_t)run.captures * kCleanWords, 0);
    if (run.n_out != 0) {               // (no buffer was processed otherwise: nothing was written for the kernels to read)
        if (const int rc = reserve(*ctx, run); rc != OOKD_OK) return rc;
        CleanParams p{};
        p.list = edge_list_view(run);
        p.min_len[0] = min_off;
        p.min_len[1] = min_on;
        p.num_tiles_cap = (uint32_t)std::min<uint64_t>(ctx->tiles, UINT32_MAX);
        p.out_capacity = ctx->out_capacity;
        p.agg = ctx->d_agg;
        p.carry = ctx->d_carry;
        p.out = ctx->d_out;
        p.out_prefix = ctx->d_prefix;
        const int rc = ctx->run("ookd_rx_clean_edges", run, ctx->host.size(), ctx->host.data(), [&](unsigned long long *d) {
            p.result = d;
            return launch_clean_edges(p, run.num_edges, run.stream);
        });
        if (rc != OOKD_OK) return rc;
    }
    ctx->serial = run.serial;
    ctx->min_on = min_on;
    ctx->min_off = min_off;
    ctx->captures = run.captures;
    ctx->prefix.assign((size_t)run.captures + 1u, 0);
    for (uint32_t c = 0; c < run.captures; ++c)
        ctx->prefix[c + 1u] = ctx->prefix[c] + ctx->host[(size_t)c * kCleanWords + kCleanWordOut];
    return OOKD_OK;
}

int ookd_rx_get_clean_info(const ookd_rx *rx, uint32_t capture, ookd_clean_info *out) {
    clear_error();
    if (!rx || !out) {
        set_error("ookd_rx_get_clean_info: NULL argument");
        return OOKD_ERR_ARG;
    }
    const CleanCtx *c = answered(rx);
    if (!c) {
        set_error("ookd_rx_get_clean_info: no cleaned list of the last run");
        return OOKD_ERR_ARG;
    }
    if (capture >= c->captures) {
        set_error("ookd_rx_get_clean_info: capture %u of %u", capture, c->captures);
        return OOKD_ERR_ARG;
    }
    const uint64_t *r = c->host.data() + (size_t)capture * kCleanWords;
    memset(out, 0, sizeof *out);
    out->edges_in = r[kCleanWordIn];
    out->edges_out = r[kCleanWordOut];
    out->deleted[0] = r[kCleanWordDel];
    out->deleted[1] = r[kCleanWordDel + 1u];
    out->min_on = c->min_on;
    out->min_off = c->min_off;
    return OOKD_OK;
}

int ookd_rx_get_clean_edges(const ookd_rx *rx, uint32_t capture, uint64_t *edges, uint64_t capacity, uint64_t *num_edges) {
    clear_error();
    if (!rx) {
        set_error("ookd_rx_get_clean_edges: NULL argument");
        return OOKD_ERR_ARG;
    }
    const CleanCtx *c = answered(rx);
    if (!c) {
        set_error("ookd_rx_get_clean_edges: no cleaned list of the last run");
        return OOKD_ERR_ARG;
    }
    if (capture >= c->captures) {
        set_error("ookd_rx_get_clean_edges: capture %u of %u", capture, c->captures);
        return OOKD_ERR_ARG;
    }
    const uint64_t lo = c->prefix[capture], n = c->prefix[capture + 1u] - lo;
    if (num_edges) *num_edges = n;
    const uint64_t take = std::min<uint64_t>(n, capacity);
    if (edges && take && lo + take <= c->out_capacity) {
        EdgeRun run;
        ookd_rx_edge_run(rx, &run);
        if (hipSetDevice(run.dev) != hipSuccess ||
            hipMemcpy(edges, c->d_out + lo, take * 8, hipMemcpyDeviceToHost) != hipSuccess) {
            set_error("ookd_rx_get_clean_edges: HIP failure: %s", hipGetErrorString(hipGetLastError()));
            return OOKD_ERR_HIP;
        }
    }
    return OOKD_OK;
}

float ookd_rx_clean_kernel_ms(const ookd_rx *rx) { return edge_pass_kernel_ms(rx, kEdgePassClean); }

}  // extern "C"
