// burst_baseband.cpp -- burst basebands: the C ABI around burst_baseband.hip's kernels, the table rule
// ookd_baseband_bursts and the contract on the host given the filter's output, ookd_baseband_of
// (include/ookiedokie_amd.h states all three as a contract).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <new>
#include <vector>

#include "burst_baseband.hpp"
#include "edge_pass.hpp"
#include "front_plan.hpp"
#include "run_levels.hpp"

#pragma clang fp contract(off)

using namespace ookd;

static_assert(sizeof(ookd_baseband_burst) == sizeof(BasebandDev), "three 64-bit words");
static_assert(sizeof(ookd_baseband_info) == 56, "ookd_baseband_info layout");
static_assert(OOKD_BASEBAND_CF32 == kBasebandCf32 && OOKD_BASEBAND_SC16Q11 == kBasebandSc16, "the formats");

namespace ookd {

struct BasebandCtx : EdgePass {
    // the filter as the pass's kernel reads it, made by the first call that launches (constant for the context)
    bool built = false;
    SurveyParams sv{};
    size_t lds_bytes = 0;
    float *d_taps = nullptr, *d_ctaps = nullptr;
    uint32_t ctap_floats = 0;
    // the derived table of capture `table_capture` of burst table `table_made` (BurstTableRef::made; 0: none)
    BasebandDev *d_table = nullptr;     // [table_slots] (grown, never shrunk)
    uint64_t table_slots = 0, table_made = 0;
    uint32_t table_capture = 0;
    // of the last pass about run `serial`
    uint64_t pass_made = 0, tiles_filtered = 0;
    uint32_t pass_capture = 0;
    uint64_t asked = 0;                 // orders the raw and the clean form's context, as BurstCtx::asked

    ~BasebandCtx() override {
        if (d_taps) (void)hipFree(d_taps);
        if (d_ctaps) (void)hipFree(d_ctaps);
        if (d_table) (void)hipFree(d_table);
    }
};

}  // namespace ookd

namespace {

uint64_t g_asked = 0;

uint32_t element_bytes(uint32_t format) { return format == kBasebandCf32 ? 8u : 4u; }

// the table rule over the entries of a burst table in either form; -> total_outputs
template <typename Entry, typename First, typename Count>
uint64_t derive(const Entry *table, uint64_t num_bursts, uint64_t D, ookd_baseband_burst *out, uint64_t capacity, First first, Count count) {
    uint64_t sum = 0;
    for (uint64_t b = 0; b < num_bursts; ++b) {
        const uint64_t lo = baseband_ceil(first(table[b]), D), hi = baseband_ceil(first(table[b]) + count(table[b]), D);
        if (out && b < capacity) out[b] = ookd_baseband_burst{lo, hi - lo, sum};
        sum += hi - lo;
    }
    return sum;
}

uint64_t derive_dev(const BurstTableRef &t, uint64_t D, ookd_baseband_burst *out, uint64_t capacity) {
    return derive(t.table, t.num_bursts, D, out, capacity, [](const BurstDev &e) { return e.first_sample; },
                  [](const BurstDev &e) { return e.end_offset - e.offset; });
}

// The context's filter in the survey's layout, as run_levels.cpp builds it (survey_tile's LDS geometry).
int build_filter(const char *who, BasebandCtx &ctx, const EdgeRun &run, const RunLevelSource &src) {
    const FrontPlan &plan = *src.plan;
    const FrontParams &fp = plan.fp;
    SurveyParams p{};
    p.sample_fmt = fp.sample_fmt;
    p.num_stages = fp.num_stages;
    std::vector<float> taps;
    for (uint32_t s = 0; s < fp.num_stages && s < (uint32_t)kMaxStages; ++s) {
        FirStageDev d{};
        d.decim = fp.stage[s].decim;
        d.ntaps = d.ntaps_pad = fp.stage[s].ntaps;
        d.tap_off = (uint32_t)taps.size();
        taps.insert(taps.end(), plan.taps.begin() + fp.stage[s].tap_off, plan.taps.begin() + fp.stage[s].tap_off + fp.stage[s].ntaps);
        p.stage[s] = d;
    }
    const bool tuned = !plan.carriers.empty() && fp.num_stages != 0;
    std::vector<float> ctaps;
    if (tuned) {
        for (const CarrierPlan &c : plan.carriers) {
            for (uint32_t s = 0; s < fp.num_stages; ++s) {
                const float *from = plan.ctaps.data() + c.tap_off + 2 * (size_t)fp.stage[s].tap_off;
                ctaps.insert(ctaps.end(), from, from + 2 * (size_t)fp.stage[s].ntaps);
            }
        }
    }
    if (!survey_tile(p, &ctx.lds_bytes, tuned ? 2u : 1u)) {
        set_error("%s: the filter's history does not fit the kernel's LDS window", who);
        return OOKD_ERR_ARG;
    }
    if (hipSetDevice(run.dev) != hipSuccess) {
        set_error("%s: hipSetDevice failed", who);
        return OOKD_ERR_HIP;
    }
    if ((!taps.empty() &&
         (hipMalloc(reinterpret_cast<void **>(&ctx.d_taps), taps.size() * sizeof(float)) != hipSuccess ||
          hipMemcpy(ctx.d_taps, taps.data(), taps.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess)) ||
        (!ctaps.empty() &&
         (hipMalloc(reinterpret_cast<void **>(&ctx.d_ctaps), ctaps.size() * sizeof(float)) != hipSuccess ||
          hipMemcpy(ctx.d_ctaps, ctaps.data(), ctaps.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess))) {
        set_error("%s: device allocation failed: %s", who, hipGetErrorString(hipGetLastError()));
        if (ctx.d_taps) (void)hipFree(ctx.d_taps);
        if (ctx.d_ctaps) (void)hipFree(ctx.d_ctaps);
        ctx.d_taps = ctx.d_ctaps = nullptr;
        return OOKD_ERR_NOMEM;
    }
    p.taps = ctx.d_taps;
    ctx.ctap_floats = plan.carrier_context() ? 2u * p.num_taps : 0u;
    ctx.sv = p;
    ctx.built = true;
    return OOKD_OK;
}

EdgePassId pass_of(const BurstTableRef &t) { return t.clean ? kEdgePassCleanBaseband : kEdgePassBaseband; }

// The tile of the pass for the context's filter without building anything on the device (0: no LDS window).
uint32_t tile_of(const RunLevelSource &src) {
    const FrontParams &fp = src.plan->fp;
    SurveyParams p{};
    p.num_stages = fp.num_stages;
    for (uint32_t s = 0; s < fp.num_stages && s < (uint32_t)kMaxStages; ++s) {
        p.stage[s].decim = fp.stage[s].decim;
        p.stage[s].ntaps = p.stage[s].ntaps_pad = fp.stage[s].ntaps;
    }
    const bool tuned = !src.plan->carriers.empty() && fp.num_stages != 0;
    return survey_tile(p, nullptr, tuned ? 2u : 1u);
}

int baseband(const char *who, ookd_rx *rx, uint32_t capture, uint32_t format, void *out, uint64_t capacity, bool to_host) {
    clear_error();
    if (!rx) {
        set_error("%s: NULL argument", who);
        return OOKD_ERR_ARG;
    }
    if (format != kBasebandCf32 && format != kBasebandSc16) {
        set_error("%s: unknown format %u", who, format);
        return OOKD_ERR_ARG;
    }
    EdgeRun run;
    if (const int rc = edge_run_check(who, rx, capture, run); rc != OOKD_OK) return rc;
    BurstTableRef t;
    if (!burst_table_ref(who, rx, capture, run, t)) return OOKD_ERR_ARG;
    RunLevelSource src;
    ookd_rx_level_source(rx, &src);
    const uint64_t D = std::max<uint32_t>(src.plan->total_decim, 1u);
    const uint64_t total = derive_dev(t, D, nullptr, 0);
    if (capacity < total) {
        set_error("%s: the cut holds %llu outputs, capacity %llu", who, (unsigned long long)total, (unsigned long long)capacity);
        return OOKD_ERR_CAPACITY;
    }
    const uint32_t bytes = element_bytes(format);
    if (!to_host && out && (reinterpret_cast<uintptr_t>(out) & (bytes - 1u)) != 0) {
        set_error("%s: d_out is not aligned to its element of %u bytes", who, bytes);
        return OOKD_ERR_ARG;
    }
    std::unique_ptr<EdgePass> &slot = ookd_rx_edge_pass(rx, pass_of(t));
    if (!slot) slot.reset(new (std::nothrow) BasebandCtx());
    BasebandCtx *ctx = static_cast<BasebandCtx *>(slot.get());
    if (!ctx) {
        set_error("%s: out of memory", who);
        return OOKD_ERR_NOMEM;
    }
    ctx->asked = ++g_asked;
    if (total == 0 || t.num_bursts == 0 || run.n_out == 0) {    // nothing to launch
        ctx->serial = run.serial;
        ctx->kernel_ms = 0.0f;
        ctx->pass_made = 0;
        ctx->tiles_filtered = 0;
        return OOKD_OK;
    }
    if (!out) {
        set_error("%s: NULL argument", who);
        return OOKD_ERR_ARG;
    }
    if (!ctx->built) {
        if (const int rc = build_filter(who, *ctx, run, src); rc != OOKD_OK) return rc;
    }
    if (!src.iq || !t.d_table || hipSetDevice(run.dev) != hipSuccess) {
        set_error("%s: the run's capture is not at hand", who);
        return OOKD_ERR_HIP;
    }
    if (ctx->table_slots < t.num_bursts) {
        if (ctx->d_table) (void)hipFree(ctx->d_table);
        ctx->d_table = nullptr;
        ctx->table_slots = ctx->table_made = 0;
        if (hipMalloc(reinterpret_cast<void **>(&ctx->d_table), (size_t)t.num_bursts * sizeof(BasebandDev)) != hipSuccess) {
            set_error("%s: device allocation failed: %s", who, hipGetErrorString(hipGetLastError()));
            return OOKD_ERR_NOMEM;
        }
        ctx->table_slots = t.num_bursts;
    }
    void *d_out = out;
    if (to_host && hipMalloc(&d_out, (size_t)total * bytes) != hipSuccess) {
        set_error("%s: device allocation failed: %s", who, hipGetErrorString(hipGetLastError()));
        return OOKD_ERR_NOMEM;
    }
    ctx->pass_made = 0;
    ctx->tiles_filtered = 0;
    int rc = OOKD_OK;
    // the derived table, in front of the timed pass on the same stream (stale: another table, or another capture's)
    if (ctx->table_made != t.made || ctx->table_capture != capture) {
        ctx->table_made = 0;
        if (launch_baseband_table(t.d_table, t.num_bursts, D, ctx->d_table, run.stream) != hipSuccess) {
            set_error("%s: HIP failure: %s", who, hipGetErrorString(hipGetLastError()));
            rc = OOKD_ERR_HIP;
        }
    }
    if (rc == OOKD_OK) {
        BasebandParams p{};
        p.sv = ctx->sv;
        p.sv.iq = src.iq;
        p.sv.cap_stride = src.stride;
        p.sv.n_out = run.n_out;
        p.sv.num_tiles = (run.n_out + p.sv.tile - 1) / p.sv.tile;
        p.n_valid = src.n_valid;
        p.capture = capture;
        p.one_source = src.plan->carrier_context() ? 1u : 0u;
        p.ctap_floats = ctx->ctap_floats;
        p.format = format;
        p.ctaps = ctx->d_ctaps;
        p.table = ctx->d_table;
        p.num_bursts = t.num_bursts;
        p.total = total;
        p.out = d_out;
        const size_t lds_bytes = ctx->lds_bytes;
        uint64_t words[kBasebandWords] = {0};
        rc = ctx->run(who, run, kBasebandWords, words, [&](unsigned long long *d) {
            p.result = d;
            return launch_burst_baseband(p, lds_bytes, run.stream);
        });
        if (rc == OOKD_OK) {
            ctx->table_made = t.made;
            ctx->table_capture = capture;
            ctx->pass_made = t.made;
            ctx->pass_capture = capture;
            ctx->tiles_filtered = words[0];
            if (to_host && hipMemcpy(out, d_out, (size_t)total * bytes, hipMemcpyDeviceToHost) != hipSuccess) {
                set_error("%s: HIP failure: %s", who, hipGetErrorString(hipGetLastError()));
                rc = OOKD_ERR_HIP;
            }
        } else {
            ctx->table_made = 0;
        }
    }
    if (to_host) (void)hipFree(d_out);
    return rc;
}

// The baseband table of `capture`'s burst table, or an error code + error.
int table_of(const char *who, ookd_rx *rx, uint32_t capture, EdgeRun &run, BurstTableRef &t, uint64_t &D) {
    if (!rx) {
        set_error("%s: NULL argument", who);
        return OOKD_ERR_ARG;
    }
    if (!burst_table_ref(who, rx, capture, run, t)) return OOKD_ERR_ARG;
    RunLevelSource src;
    ookd_rx_level_source(rx, &src);
    D = std::max<uint32_t>(src.plan->total_decim, 1u);
    return OOKD_OK;
}

}  // namespace

extern "C" {

int ookd_baseband_bursts(const ookd_burst *table, uint64_t num_bursts, uint64_t D, ookd_baseband_burst *out, uint64_t capacity,
                         uint64_t *total_outputs) {
    clear_error();
    if (!table && num_bursts) {
        set_error("ookd_baseband_bursts: NULL argument");
        return OOKD_ERR_ARG;
    }
    if (D == 0) {
        set_error("ookd_baseband_bursts: the decimation must be at least 1");
        return OOKD_ERR_ARG;
    }
    const uint64_t total = derive(table, num_bursts, D, out, capacity, [](const ookd_burst &e) { return e.first_sample; },
                                  [](const ookd_burst &e) { return e.num_samples; });
    if (total_outputs) *total_outputs = total;
    return OOKD_OK;
}

int ookd_baseband_of(const float *y, uint64_t n_out, const ookd_baseband_burst *table, uint64_t num_bursts, uint32_t format,
                     void *out, uint64_t capacity_outputs) {
    clear_error();
    if (format != kBasebandCf32 && format != kBasebandSc16) {
        set_error("ookd_baseband_of: unknown format %u", format);
        return OOKD_ERR_ARG;
    }
    if ((!table && num_bursts) || (!y && n_out)) {
        set_error("ookd_baseband_of: NULL argument");
        return OOKD_ERR_ARG;
    }
    uint64_t total = 0;
    for (uint64_t b = 0; b < num_bursts; ++b) {
        if (table[b].first_output > n_out || table[b].num_outputs > n_out - table[b].first_output) {
            set_error("ookd_baseband_of: burst %llu reaches beyond n_out", (unsigned long long)b);
            return OOKD_ERR_ARG;
        }
        total += table[b].num_outputs;
    }
    if (capacity_outputs < total) {
        set_error("ookd_baseband_of: the cut holds %llu outputs, capacity %llu", (unsigned long long)total,
                  (unsigned long long)capacity_outputs);
        return OOKD_ERR_CAPACITY;
    }
    if (total && !out) {
        set_error("ookd_baseband_of: NULL argument");
        return OOKD_ERR_ARG;
    }
    uint64_t at = 0;                    // dense: burst after burst (offset_b of the rule)
    for (uint64_t b = 0; b < num_bursts; ++b) {
        for (uint64_t i = 0; i < table[b].num_outputs; ++i, ++at) {
            const float *v = y + 2 * (table[b].first_output + i);
            if (format == kBasebandCf32) {
                memcpy(static_cast<float *>(out) + 2 * at, v, 2 * sizeof(float));
            } else {
                int16_t *to = static_cast<int16_t *>(out) + 2 * at;
                to[0] = (int16_t)baseband_q16(v[0]);
                to[1] = (int16_t)baseband_q16(v[1]);
            }
        }
    }
    return OOKD_OK;
}

int ookd_rx_get_baseband_info(ookd_rx *rx, uint32_t capture, ookd_baseband_info *out) {
    const char *who = "ookd_rx_get_baseband_info";
    clear_error();
    if (!out) {
        set_error("%s: NULL argument", who);
        return OOKD_ERR_ARG;
    }
    EdgeRun run;
    BurstTableRef t;
    uint64_t D = 1;
    if (const int rc = table_of(who, rx, capture, run, t, D); rc != OOKD_OK) return rc;
    RunLevelSource src;
    ookd_rx_level_source(rx, &src);
    const uint32_t tile = tile_of(src);
    if (tile == 0) {
        set_error("%s: the filter's history does not fit the kernel's LDS window", who);
        return OOKD_ERR_ARG;
    }
    memset(out, 0, sizeof *out);
    out->num_bursts = t.num_bursts;
    out->total_outputs = derive_dev(t, D, nullptr, 0);
    out->tile_outputs = tile;
    out->tiles_total = (run.n_out + tile - 1) / tile;
    out->decimation = (uint32_t)D;
    const BasebandCtx *c = static_cast<const BasebandCtx *>(ookd_rx_edge_pass(rx, pass_of(t)).get());
    if (c && c->serial == run.serial && c->pass_made == t.made && c->pass_capture == capture) out->tiles_filtered = c->tiles_filtered;
    const std::vector<CarrierPlan> &carriers = src.plan->carriers;
    if (!carriers.empty() && src.plan->fp.num_stages != 0) {
        out->nu = carriers[src.plan->carrier_context() && capture < carriers.size() ? capture : 0].nu;
    }
    const double x = out->nu * (double)D;
    out->turn = x - std::rint(x);
    return OOKD_OK;
}

int ookd_rx_get_baseband_bursts(ookd_rx *rx, uint32_t capture, ookd_baseband_burst *table, uint64_t capacity, uint64_t *num_bursts) {
    const char *who = "ookd_rx_get_baseband_bursts";
    clear_error();
    EdgeRun run;
    BurstTableRef t;
    uint64_t D = 1;
    if (const int rc = table_of(who, rx, capture, run, t, D); rc != OOKD_OK) return rc;
    if (num_bursts) *num_bursts = t.num_bursts;
    (void)derive_dev(t, D, table, capacity);
    return OOKD_OK;
}

int ookd_rx_burst_baseband_device(ookd_rx *rx, uint32_t capture, uint32_t format, void *d_out, uint64_t capacity_outputs) {
    return baseband("ookd_rx_burst_baseband_device", rx, capture, format, d_out, capacity_outputs, false);
}

int ookd_rx_burst_baseband_host(ookd_rx *rx, uint32_t capture, uint32_t format, void *out, uint64_t capacity_outputs) {
    return baseband("ookd_rx_burst_baseband_host", rx, capture, format, out, capacity_outputs, true);
}

float ookd_rx_baseband_kernel_ms(const ookd_rx *rx) {
    if (!rx) return 0.0f;
    EdgeRun run;
    ookd_rx_edge_run(rx, &run);
    if (run.serial == 0) return 0.0f;
    const BasebandCtx *best = nullptr;
    for (EdgePassId id : {kEdgePassBaseband, kEdgePassCleanBaseband}) {
        const BasebandCtx *c = static_cast<const BasebandCtx *>(ookd_rx_edge_pass(const_cast<ookd_rx *>(rx), id).get());
        if (c && c->serial == run.serial && (!best || c->asked > best->asked)) best = c;
    }
    return best ? best->kernel_ms : 0.0f;
}

}  // extern "C"
