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
    uint32_t *d_blk_prefix = nullptr;   // [blk_prefix_capacity]: the debounced decode's per-block prefix (clean_chain_reserve)
    uint32_t blk_prefix_capacity = 0;
    // of run `serial`
    uint64_t min_on = 0, min_off = 0;
    uint32_t captures = 0;
    bool counts_pending = false;        // the pass ran in the run's chain and nobody has fetched its counts yet
    std::vector<uint64_t> host;         // [captures][kCleanWords]
    std::vector<uint64_t> prefix;       // [captures + 1]: the cleaned prefix, from the counts

    ~CleanCtx() override {
        if (d_out) (void)hipFree(d_out);
        if (d_prefix) (void)hipFree(d_prefix);
        if (d_agg) (void)hipFree(d_agg);
        if (d_carry) (void)hipFree(d_carry);
        if (d_blk_prefix) (void)hipFree(d_blk_prefix);
    }

    void set_prefix() {
        prefix.assign((size_t)captures + 1u, 0);
        for (uint32_t c = 0; c < captures; ++c) prefix[c + 1u] = prefix[c] + host[(size_t)c * kCleanWords + kCleanWordOut];
    }
    // The counts of a pass that ran in the run's chain, on the first call that needs them (the run has been waited
    // for: its stream is idle and the words are final).  false: the run did not finish, or the copy failed.
    bool fetch_counts(const EdgeRun &run) {
        if (!counts_pending) return true;
        if (run.in_flight || !run.valid || run.overflow) return false;
        if (hipSetDevice(run.dev) != hipSuccess ||
            hipMemcpy(host.data(), d_result, host.size() * 8, hipMemcpyDeviceToHost) != hipSuccess) {
            return false;
        }
        counts_pending = false;
        set_prefix();
        return true;
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

// the buffers a run of num_edges edges in `captures` captures needs
int reserve(CleanCtx &c, const char *who, int dev, uint64_t num_edges, uint32_t captures) {
    if (hipSetDevice(dev) != hipSuccess) {
        set_error("%s: hipSetDevice failed", who);
        return OOKD_ERR_HIP;
    }
    const uint64_t edges = std::max<uint64_t>(num_edges, 1u), tiles = clean_tiles_of(num_edges, captures);
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
    if (ok && c.prefix_capacity < captures + 1u) {
        c.prefix_capacity = 0;
        ok = grow(c.d_prefix, captures + 1u);
        if (ok) c.prefix_capacity = captures + 1u;
    }
    if (!ok) {
        set_error("%s: device allocation failed: %s", who, hipGetErrorString(hipGetLastError()));
        return OOKD_ERR_NOMEM;
    }
    return OOKD_OK;
}

CleanCtx *clean_ctx(ookd_rx *rx) {
    std::unique_ptr<EdgePass> &slot = ookd_rx_edge_pass(rx, kEdgePassClean);
    if (!slot) slot.reset(new (std::nothrow) CleanCtx());
    return static_cast<CleanCtx *>(slot.get());
}

CleanParams clean_params(const CleanCtx &c, const EdgeRun &run, uint64_t min_on, uint64_t min_off) {
    CleanParams p{};
    p.list = edge_list_view(run);
    p.min_len[0] = min_off;
    p.min_len[1] = min_on;
    p.num_tiles_cap = (uint32_t)std::min<uint64_t>(c.tiles, UINT32_MAX);
    p.out_capacity = c.out_capacity;
    p.agg = c.d_agg;
    p.carry = c.d_carry;
    p.out = c.d_out;
    p.out_prefix = c.d_prefix;
    return p;
}

// the context's clean pass when it has answered the context's last run, else null
const CleanCtx *answered(const ookd_rx *rx) {
    EdgeRun run;
    ookd_rx_edge_run(rx, &run);
    CleanCtx *c = static_cast<CleanCtx *>(ookd_rx_edge_pass(const_cast<ookd_rx *>(rx), kEdgePassClean).get());
    return c && run.serial != 0 && c->serial == run.serial && c->fetch_counts(run) ? c : nullptr;
}

}  // namespace

namespace ookd {

bool clean_run_view(ookd_rx *rx, EdgeRun &run) {
    CleanCtx *c = static_cast<CleanCtx *>(ookd_rx_edge_pass(rx, kEdgePassClean).get());
    if (!c || run.serial == 0 || c->serial != run.serial || !c->fetch_counts(run)) return false;
    run.d_edges = c->d_out;
    run.edge_capacity = c->out_capacity;
    run.d_blk_offset = c->d_prefix;
    run.blocks_per_cap = 1;
    run.num_edges = c->prefix.empty() ? 0 : c->prefix.back();
    return true;
}

int clean_chain_reserve(ookd_rx *rx, int dev, uint64_t edge_capacity, uint32_t captures, uint32_t blocks, CleanChainView &view) {
    const char *who = "ookd_rx_set_debounce";
    CleanCtx *c = clean_ctx(rx);
    if (!c) {
        set_error("%s: out of memory", who);
        return OOKD_ERR_NOMEM;
    }
    // (by the capacities: a buffer that was replaced may come back at the address of the one that was freed)
    const uint64_t had_out = c->out_capacity;
    const uint32_t had_prefix = c->prefix_capacity;
    const size_t had_result = c->capacity;
    int rc = reserve(*c, who, dev, edge_capacity, captures);
    if (rc == OOKD_OK) rc = c->reserve_result(who, dev, (size_t)captures * kCleanWords);
    const uint64_t words = (uint64_t)captures * blocks + 1u;
    if (rc == OOKD_OK && c->blk_prefix_capacity < words) {
        c->blk_prefix_capacity = 0;
        if (words > UINT32_MAX || !grow(c->d_blk_prefix, words)) {
            set_error("%s: device allocation failed: %s", who, hipGetErrorString(hipGetLastError()));
            rc = OOKD_ERR_NOMEM;
        } else {
            c->blk_prefix_capacity = (uint32_t)words;
        }
    }
    if (c->out_capacity != had_out || c->prefix_capacity != had_prefix || c->capacity != had_result) {
        // the list, its prefix or the counts of the pass that answered the last run lay in a buffer that is gone: that
        // run has no cleaned list any more, and what the clean readers kept was about it
        c->serial = 0;
        c->kernel_ms = 0.0f;
        c->counts_pending = false;
        for (EdgePassId id : {kEdgePassCleanPulse, kEdgePassCleanSymbol, kEdgePassCleanLevels, kEdgePassCleanBursts, kEdgePassCleanMoments}) {
            if (EdgePass *reader = ookd_rx_edge_pass(rx, id).get()) {
                reader->serial = 0;
                reader->kernel_ms = 0.0f;
            }
        }
    }
    if (rc == OOKD_OK) {
        // (the run's path then only assigns within these: clean_chain_queue allocates nothing)
        c->host.reserve((size_t)captures * kCleanWords);
        c->prefix.reserve((size_t)captures + 1u);
    }
    view.edges = c->d_out;
    view.blk_prefix = c->d_blk_prefix;
    return rc;
}

hipError_t clean_chain_queue(ookd_rx *rx, const EdgeRun &run, uint64_t min_on, uint64_t min_off) {
    CleanCtx *c = static_cast<CleanCtx *>(ookd_rx_edge_pass(rx, kEdgePassClean).get());
    const size_t words = (size_t)run.captures * kCleanWords;
    if (!c || c->capacity < words || c->prefix_capacity < run.captures + 1u ||
        c->blk_prefix_capacity < (uint64_t)run.captures * run.blocks_per_cap + 1u) {
        return hipErrorInvalidValue;            // (clean_chain_reserve sized them for every run the context takes)
    }
    c->serial = run.serial;
    c->kernel_ms = 0.0f;                        // part of the chain: not timed on its own
    c->min_on = min_on;
    c->min_off = min_off;
    c->captures = run.captures;
    c->host.assign(words, 0);
    c->set_prefix();
    c->counts_pending = false;
    if (run.n_out == 0) return hipSuccess;      // (no buffer was processed: nothing to read, every count is zero)
    CleanParams p = clean_params(*c, run, min_on, min_off);
    p.blk_prefix = c->d_blk_prefix;
    p.blk_prefix_capacity = c->blk_prefix_capacity;
    p.result = c->d_result;
    hipError_t e = hipMemsetAsync(c->d_result, 0, words * 8, run.stream);
    if (e != hipSuccess) return e;
    // the grids by what the list can hold: the run's edge count is not known on the host before the run has ended
    e = launch_clean_edges(p, run.edge_capacity, run.stream);
    if (e == hipSuccess) c->counts_pending = true;
    return e;
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
    CleanCtx *ctx = clean_ctx(rx);
    if (!ctx) {
        set_error("ookd_rx_clean_edges: out of memory");
        return OOKD_ERR_NOMEM;
    }
    if (ctx->serial == run.serial && ctx->min_on == min_on && ctx->min_off == min_off) return OOKD_OK;
    // another list from here on: what the clean readers keep is about the one before
    for (EdgePassId id : {kEdgePassCleanPulse, kEdgePassCleanSymbol, kEdgePassCleanLevels, kEdgePassCleanBursts, kEdgePassCleanMoments}) {
        if (EdgePass *reader = ookd_rx_edge_pass(rx, id).get()) {
            reader->serial = 0;
            reader->kernel_ms = 0.0f;
        }
    }
    ctx->serial = 0;
    ctx->kernel_ms = 0.0f;
    ctx->counts_pending = false;
    ctx->host.assign((size_t)run.captures * kCleanWords, 0);
    if (run.n_out != 0) {               // (no buffer was processed otherwise: nothing was written for the kernels to read)
        if (const int rc = reserve(*ctx, "ookd_rx_clean_edges", run.dev, run.num_edges, run.captures); rc != OOKD_OK) return rc;
        CleanParams p = clean_params(*ctx, run, min_on, min_off);
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
    ctx->set_prefix();
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
