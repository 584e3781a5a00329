// bursts.cpp -- burst extraction: the C ABI around bursts.hip's table pass and copy, and the host-only rule
// ookd_find_bursts (include/ookiedokie_amd.h states the rule as a contract).
#include <algorithm>
#include <cstring>
#include <new>
#include <vector>

#include "bursts.hpp"
#include "clean.hpp"
#include "front_plan.hpp"
#include "run_levels.hpp"

using namespace ookd;

namespace ookd {

struct BurstCtx : EdgePass {
    BurstDev *d_table = nullptr;        // [table_slots] (grown, never shrunk)
    uint64_t table_slots = 0;
    BurstAgg *d_agg = nullptr;          // [tiles]
    BurstCarry *d_carry = nullptr;      // [tiles]
    uint64_t tiles = 0;
    hipEvent_t c0 = nullptr, c1 = nullptr;      // around the copy kernel
    float copy_ms = 0.0f;               // of the last copy about run `serial`
    // of run `serial`
    uint64_t pre = 0, post = 0, max_gap = 0;
    uint64_t asked = 0;                 // orders the raw and the clean form: the later ookd_rx_bursts call has the larger
    uint64_t made = 0;                  // which table this is, of all that were made (BurstTableRef::made)
    uint32_t captures = 0;
    std::vector<uint64_t> host;         // [captures][kBurstWords]
    std::vector<BurstDev> table;        // the captures' entries one after the other
    std::vector<uint64_t> table_at;     // [captures + 1]: capture c's are table[table_at[c] .. table_at[c + 1])

    ~BurstCtx() override {
        if (d_table) (void)hipFree(d_table);
        if (d_agg) (void)hipFree(d_agg);
        if (d_carry) (void)hipFree(d_carry);
        if (c0) (void)hipEventDestroy(c0);
        if (c1) (void)hipEventDestroy(c1);
    }
};

}  // namespace ookd

namespace {

uint64_t g_asked = 0, g_made = 0;

template <typename T>
bool grow(T *&p, uint64_t want) {
    if (p) (void)hipFree(p);
    p = nullptr;
    return hipMalloc(reinterpret_cast<void **>(&p), (size_t)want * sizeof(T)) == hipSuccess;
}

// the buffers a run of num_edges edges in `captures` captures needs
int reserve(BurstCtx &c, const char *who, int dev, uint64_t num_edges, uint32_t captures) {
    if (hipSetDevice(dev) != hipSuccess) {
        set_error("%s: hipSetDevice failed", who);
        return OOKD_ERR_HIP;
    }
    const uint64_t slots = burst_table_slots(num_edges, captures), tiles = burst_tiles_of(num_edges, captures);
    bool ok = true;
    if (c.table_slots < slots) {
        c.table_slots = 0;
        ok = grow(c.d_table, slots);
        if (ok) c.table_slots = slots;
    }
    if (ok && c.tiles < tiles) {
        c.tiles = 0;
        ok = grow(c.d_agg, tiles) && grow(c.d_carry, tiles);
        if (ok) c.tiles = tiles;
    }
    if (!ok) {
        set_error("%s: device allocation failed: %s", who, hipGetErrorString(hipGetLastError()));
        return OOKD_ERR_NOMEM;
    }
    return OOKD_OK;
}

// The context's burst table of its last run: of the raw and the clean form the one ookd_rx_bursts was last called
// with, or null.  `run` receives the last run.
BurstCtx *answered(const ookd_rx *rx, EdgeRun &run) {
    ookd_rx_edge_run(rx, &run);
    if (run.serial == 0 || run.in_flight) return nullptr;
    BurstCtx *best = nullptr;
    for (EdgePassId id : {kEdgePassBursts, kEdgePassCleanBursts}) {
        BurstCtx *c = static_cast<BurstCtx *>(ookd_rx_edge_pass(const_cast<ookd_rx *>(rx), id).get());
        if (c && c->serial == run.serial && (!best || c->asked > best->asked)) best = c;
    }
    return best;
}

BurstCtx *table_of(const char *who, const ookd_rx *rx, uint32_t capture, EdgeRun &run) {
    BurstCtx *c = answered(rx, run);
    if (!c) {
        set_error("%s: no burst table of the last run (ookd_rx_bursts first)", who);
        return nullptr;
    }
    if (capture >= c->captures) {
        set_error("%s: capture %u of %u", who, capture, c->captures);
        return nullptr;
    }
    return c;
}

}  // namespace

namespace ookd {

bool burst_table_ref(const char *who, const ookd_rx *rx, uint32_t capture, EdgeRun &run, BurstTableRef &out) {
    const BurstCtx *c = table_of(who, rx, capture, run);
    if (!c) return false;
    const uint64_t *r = c->host.data() + (size_t)capture * kBurstWords;
    out.num_bursts = c->table_at[capture + 1u] - c->table_at[capture];
    out.total = r[kBurstWordTotal];
    out.d_table = c->d_table ? c->d_table + burst_table_base(r[kBurstWordLo], capture) : nullptr;
    out.table = c->table.data() + c->table_at[capture];
    out.made = c->made;
    out.clean = ookd_rx_edge_pass(const_cast<ookd_rx *>(rx), kEdgePassCleanBursts).get() == c;
    return true;
}

}  // namespace ookd

namespace {

uint32_t cut_sample_bytes(const ookd_rx *rx) {
    RunLevelSource src;
    ookd_rx_level_source(rx, &src);
    return sample_bytes(src.plan->fp.sample_fmt);
}

int copy_bursts(const char *who, ookd_rx *rx, uint32_t capture, void *out, uint64_t capacity_samples, bool to_host) {
    clear_error();
    if (!rx) {
        set_error("%s: NULL argument", who);
        return OOKD_ERR_ARG;
    }
    EdgeRun run;
    BurstCtx *ctx = table_of(who, rx, capture, run);
    if (!ctx) return OOKD_ERR_ARG;
    const uint64_t *r = ctx->host.data() + (size_t)capture * kBurstWords;
    const uint64_t total = r[kBurstWordTotal], bursts = ctx->table_at[capture + 1u] - ctx->table_at[capture];
    if (capacity_samples < total) {
        set_error("%s: the cut holds %llu samples, capacity %llu", who, (unsigned long long)total, (unsigned long long)capacity_samples);
        return OOKD_ERR_CAPACITY;
    }
    ctx->copy_ms = 0.0f;
    if (total == 0 || bursts == 0) return OOKD_OK;
    if (!out) {
        set_error("%s: NULL argument", who);
        return OOKD_ERR_ARG;
    }
    RunLevelSource src;
    ookd_rx_level_source(rx, &src);
    const uint32_t bytes = sample_bytes(src.plan->fp.sample_fmt);
    const uint32_t from = src.plan->carrier_context() ? 0u : capture;      // every carrier's list cuts the one capture
    if (!src.iq || hipSetDevice(run.dev) != hipSuccess) {
        set_error("%s: the run's capture is not at hand", who);
        return OOKD_ERR_HIP;
    }
    if (!ctx->c0 && (hipEventCreate(&ctx->c0) != hipSuccess || hipEventCreate(&ctx->c1) != hipSuccess)) {
        set_error("%s: hipEventCreate failed", who);
        return OOKD_ERR_HIP;
    }
    void *d_out = out;
    if (to_host && hipMalloc(&d_out, (size_t)total * bytes) != hipSuccess) {
        set_error("%s: device allocation failed: %s", who, hipGetErrorString(hipGetLastError()));
        return OOKD_ERR_NOMEM;
    }
    BurstCopyParams p{};
    p.table = ctx->d_table + burst_table_base(r[kBurstWordLo], capture);
    p.num_bursts = bursts;
    p.total = total;
    p.src = static_cast<const char *>(src.iq) + (size_t)from * src.stride * bytes;
    p.n = src.n_valid;
    p.dst = d_out;
    p.sample_bytes = bytes;
    bool ok = hipEventRecord(ctx->c0, run.stream) == hipSuccess;
    ok = ok && launch_burst_copy(p, run.stream) == hipSuccess;
    ok = ok && hipEventRecord(ctx->c1, run.stream) == hipSuccess;
    if (ok && to_host) ok = hipMemcpyAsync(out, d_out, (size_t)total * bytes, hipMemcpyDeviceToHost, run.stream) == hipSuccess;
    ok = hipStreamSynchronize(run.stream) == hipSuccess && ok;
    if (ok) ok = hipEventElapsedTime(&ctx->copy_ms, ctx->c0, ctx->c1) == hipSuccess;
    if (!ok) {
        set_error("%s: HIP failure: %s", who, hipGetErrorString(hipGetLastError()));
        ctx->copy_ms = 0.0f;
    }
    if (to_host) (void)hipFree(d_out);
    return ok ? OOKD_OK : OOKD_ERR_HIP;
}

}  // namespace

extern "C" {

static_assert(sizeof(ookd_burst) == sizeof(BurstDev), "the device entry converts in place");

int ookd_find_bursts(const uint64_t *edges, uint64_t E, uint64_t n_out, uint64_t D, uint64_t n, uint64_t pre, uint64_t post,
                     uint64_t max_gap, ookd_burst *table, uint64_t capacity, uint64_t *num_bursts, uint64_t *total) {
    clear_error();
    if (!edges && E) {
        set_error("ookd_find_bursts: NULL argument");
        return OOKD_ERR_ARG;
    }
    if (D == 0) {
        set_error("ookd_find_bursts: the decimation must be at least 1");
        return OOKD_ERR_ARG;
    }
    if (pre > max_gap || post > max_gap - pre) {
        set_error("ookd_find_bursts: max_gap %llu is below pre + post (%llu + %llu): bursts could overlap",
                  (unsigned long long)max_gap, (unsigned long long)pre, (unsigned long long)post);
        return OOKD_ERR_ARG;
    }
    const uint64_t R = (E + 1u) / 2u;
    uint64_t count = 0, sum = 0;
    for (uint64_t r0 = 0; r0 < R;) {
        uint64_t r1 = r0;               // the burst's last run: the first whose off-run is longer than max_gap
        while (2 * r1 + 2 < E && edges[2 * r1 + 2] - edges[2 * r1 + 1] <= max_gap) ++r1;
        const uint64_t a = edges[2 * r0], f = 2 * r1 + 1 < E ? edges[2 * r1 + 1] : n_out;
        const uint64_t first = burst_scale(a - std::min(a, pre), D, n), end = burst_scale(burst_hi(f, post, n_out), D, n);
        if (table && count < capacity) {
            table[count] = ookd_burst{first, end - first, sum, r0, r1 - r0 + 1};
        }
        sum += end - first;
        ++count;
        r0 = r1 + 1;
    }
    if (num_bursts) *num_bursts = count;
    if (total) *total = sum;
    return OOKD_OK;
}

int ookd_rx_bursts(ookd_rx *rx, uint64_t pre, uint64_t post, uint64_t max_gap, uint32_t flags) {
    const char *who = "ookd_rx_bursts";
    clear_error();
    if (!rx) {
        set_error("%s: NULL argument", who);
        return OOKD_ERR_ARG;
    }
    if (flags & ~(uint32_t)OOKD_BURSTS_CLEAN) {
        set_error("%s: unknown flags 0x%x", who, flags);
        return OOKD_ERR_ARG;
    }
    if (pre > max_gap || post > max_gap - pre) {
        set_error("%s: max_gap %llu is below pre + post (%llu + %llu): bursts could overlap", who,
                  (unsigned long long)max_gap, (unsigned long long)pre, (unsigned long long)post);
        return OOKD_ERR_ARG;
    }
    const bool clean = (flags & OOKD_BURSTS_CLEAN) != 0;
    EdgeRun run;
    if (const int rc = edge_run_check(who, rx, 0, run); rc != OOKD_OK) return rc;
    if (clean && !clean_run_view(rx, run)) {
        set_error("%s: no cleaned list of the last run (ookd_rx_clean_edges first)", who);
        return OOKD_ERR_ARG;
    }
    std::unique_ptr<EdgePass> &slot = ookd_rx_edge_pass(rx, clean ? kEdgePassCleanBursts : kEdgePassBursts);
    if (!slot) slot.reset(new (std::nothrow) BurstCtx());
    BurstCtx *ctx = static_cast<BurstCtx *>(slot.get());
    if (!ctx) {
        set_error("%s: out of memory", who);
        return OOKD_ERR_NOMEM;
    }
    if (ctx->serial == run.serial && ctx->pre == pre && ctx->post == post && ctx->max_gap == max_gap) {
        ctx->asked = ++g_asked;
        return OOKD_OK;
    }
    ctx->serial = 0;
    ctx->kernel_ms = 0.0f;
    ctx->copy_ms = 0.0f;
    ctx->captures = run.captures;
    ctx->host.assign((size_t)run.captures * kBurstWords, 0);
    ctx->table.clear();
    ctx->table_at.assign((size_t)run.captures + 1u, 0);
    if (run.n_out != 0) {               // (no buffer was processed otherwise: nothing was written for the kernels to read)
        if (const int rc = reserve(*ctx, who, run.dev, run.num_edges, run.captures); rc != OOKD_OK) return rc;
        RunLevelSource src;
        ookd_rx_level_source(rx, &src);
        BurstParams p{};
        p.list = edge_list_view(run);
        p.n_out = run.n_out;
        p.D = std::max<uint32_t>(src.plan->total_decim, 1u);
        p.n = src.n_valid;
        p.pre = pre;
        p.post = post;
        p.max_gap = max_gap;
        p.num_tiles_cap = (uint32_t)std::min<uint64_t>(ctx->tiles, UINT32_MAX);
        p.table_slots = ctx->table_slots;
        p.agg = ctx->d_agg;
        p.carry = ctx->d_carry;
        p.table = ctx->d_table;
        int rc = ctx->run(who, run, ctx->host.size(), ctx->host.data(), [&](unsigned long long *d) {
            p.result = d;
            return launch_burst_table(p, run.num_edges, run.stream);
        });
        if (rc != OOKD_OK) return rc;
        // the entries that were written, capture by capture (the stream is idle)
        uint64_t entries = 0;
        for (uint32_t c = 0; c < run.captures; ++c) {
            uint64_t *r = ctx->host.data() + (size_t)c * kBurstWords;
            const uint64_t base = burst_table_base(r[kBurstWordLo], c);
            if (r[kBurstWordCount] > (r[kBurstWordEdges] + 1u) / 2u || base + r[kBurstWordCount] > ctx->table_slots) {
                r[kBurstWordCount] = r[kBurstWordTotal] = 0;    // (not of a list the host accepted)
            }
            entries += r[kBurstWordCount];
            ctx->table_at[c + 1u] = entries;
        }
        ctx->table.resize(entries);
        for (uint32_t c = 0; c < run.captures && rc == OOKD_OK; ++c) {
            const uint64_t *r = ctx->host.data() + (size_t)c * kBurstWords;
            if (r[kBurstWordCount] &&
                hipMemcpy(ctx->table.data() + ctx->table_at[c], ctx->d_table + burst_table_base(r[kBurstWordLo], c),
                          r[kBurstWordCount] * sizeof(BurstDev), hipMemcpyDeviceToHost) != hipSuccess) {
                set_error("%s: HIP failure: %s", who, hipGetErrorString(hipGetLastError()));
                rc = OOKD_ERR_HIP;
            }
        }
        if (rc != OOKD_OK) {
            ctx->serial = 0;
            ctx->kernel_ms = 0.0f;
            return rc;
        }
    }
    ctx->serial = run.serial;
    ctx->pre = pre;
    ctx->post = post;
    ctx->max_gap = max_gap;
    ctx->asked = ++g_asked;
    ctx->made = ++g_made;
    return OOKD_OK;
}

int ookd_rx_get_burst_info(const ookd_rx *rx, uint32_t capture, ookd_burst_info *out) {
    clear_error();
    if (!rx || !out) {
        set_error("ookd_rx_get_burst_info: NULL argument");
        return OOKD_ERR_ARG;
    }
    EdgeRun run;
    const BurstCtx *c = table_of("ookd_rx_get_burst_info", rx, capture, run);
    if (!c) return OOKD_ERR_ARG;
    const uint64_t *r = c->host.data() + (size_t)capture * kBurstWords;
    RunLevelSource src;
    ookd_rx_level_source(rx, &src);
    memset(out, 0, sizeof *out);
    out->num_bursts = r[kBurstWordCount];
    out->total_samples = r[kBurstWordTotal];
    out->num_runs = (r[kBurstWordEdges] + 1u) / 2u;
    out->pre = c->pre;
    out->post = c->post;
    out->max_gap = c->max_gap;
    out->flags = ookd_rx_edge_pass(const_cast<ookd_rx *>(rx), kEdgePassCleanBursts).get() == c ? OOKD_BURSTS_CLEAN : 0u;
    out->sample_bytes = cut_sample_bytes(rx);
    out->tile_edges = kBurstTile;
    out->decimation = std::max<uint32_t>(src.plan->total_decim, 1u);
    return OOKD_OK;
}

int ookd_rx_get_bursts(const ookd_rx *rx, uint32_t capture, ookd_burst *table, uint64_t capacity, uint64_t *num_bursts) {
    clear_error();
    if (!rx) {
        set_error("ookd_rx_get_bursts: NULL argument");
        return OOKD_ERR_ARG;
    }
    EdgeRun run;
    const BurstCtx *c = table_of("ookd_rx_get_bursts", rx, capture, run);
    if (!c) return OOKD_ERR_ARG;
    const uint64_t lo = c->table_at[capture], n = c->table_at[capture + 1u] - lo;
    if (num_bursts) *num_bursts = n;
    const uint64_t take = table ? std::min<uint64_t>(n, capacity) : 0;
    for (uint64_t b = 0; b < take; ++b) {
        const BurstDev &d = c->table[lo + b];
        table[b] = ookd_burst{d.first_sample, d.end_offset - d.offset, d.offset, d.first_run, d.end_run - d.first_run};
    }
    return OOKD_OK;
}

int ookd_rx_copy_bursts_device(ookd_rx *rx, uint32_t capture, void *d_out, uint64_t capacity_samples) {
    return copy_bursts("ookd_rx_copy_bursts_device", rx, capture, d_out, capacity_samples, false);
}

int ookd_rx_copy_bursts_host(ookd_rx *rx, uint32_t capture, void *out, uint64_t capacity_samples) {
    return copy_bursts("ookd_rx_copy_bursts_host", rx, capture, out, capacity_samples, true);
}

float ookd_rx_bursts_kernel_ms(const ookd_rx *rx) {
    if (!rx) return 0.0f;
    EdgeRun run;
    const BurstCtx *c = answered(rx, run);
    return c ? c->kernel_ms : 0.0f;
}

float ookd_rx_burst_copy_kernel_ms(const ookd_rx *rx) {
    if (!rx) return 0.0f;
    EdgeRun run;
    const BurstCtx *c = answered(rx, run);
    return c ? c->copy_ms : 0.0f;
}

}  // extern "C"
