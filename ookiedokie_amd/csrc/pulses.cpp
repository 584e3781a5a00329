// pulses.cpp -- pulse survey: the C ABI around pulses.hip's histogram kernel, and the host-only half -- the bin rule
// and the timing classes (include/ookiedokie_amd.h states both as a contract).
#include <algorithm>
#include <cstring>
#include <new>
#include <vector>

#include "clean.hpp"
#include "pulses.hpp"

using namespace ookd;

static_assert(OOKD_PULSE_BINS == kPulseBins, "OOKD_PULSE_BINS");
static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "histogram word");

namespace ookd {

struct PulseCtx : EdgePass {
    std::vector<uint64_t> host;     // the results of run `serial`: [captures][kPulseWords]
};

}  // namespace ookd

namespace {

struct ClassAcc {
    uint32_t first = 0, last = 0;
    uint64_t runs = 0;
    unsigned __int128 sum = 0;
};

double to_us(double x, double rate) { return rate > 0.0 ? x / rate * 1e6 : 0.0; }

// ookd_rx_pulse_hist (clean = false: the run's own edge list, pass kEdgePassPulse) and ookd_rx_pulse_hist_clean (the
// cleaned list, pass kEdgePassCleanPulse): the same kernel and the same contract over an EdgeListView of either
int pulse_hist(const char *who, bool clean, ookd_rx *rx, uint32_t capture, ookd_pulse_hist *out) {
    clear_error();
    if (!rx || !out) {
        set_error("%s: NULL argument", who);
        return OOKD_ERR_ARG;
    }
    EdgeRun run;
    if (const int rc = edge_run_check(who, rx, capture, run); rc != OOKD_OK) return rc;
    if (clean && !clean_run_view(rx, run)) {
        set_error("%s: no cleaned list of the last run (ookd_rx_clean_edges first)", who);
        return OOKD_ERR_ARG;
    }
    std::unique_ptr<EdgePass> &slot = ookd_rx_edge_pass(rx, clean ? kEdgePassCleanPulse : kEdgePassPulse);
    if (!slot) slot.reset(new (std::nothrow) PulseCtx());
    PulseCtx *ctx = static_cast<PulseCtx *>(slot.get());
    if (!ctx) {
        set_error("%s: out of memory", who);
        return OOKD_ERR_NOMEM;
    }
    if (ctx->serial != run.serial) {    // one launch for all captures of the run; ctx->host keeps them until the next run
        ctx->host.assign((size_t)run.captures * kPulseWords, 0);
        if (run.n_out == 0) {           // no buffer was processed: nothing was written for the kernel to read
            ctx->serial = run.serial;
            ctx->kernel_ms = 0.0f;
        } else {
            const int rc = ctx->run(who, run, ctx->host.size(), ctx->host.data(), [&](unsigned long long *d) {
                return launch_pulse_hist(PulseParams{edge_list_view(run), d}, run.num_edges, run.stream);
            });
            if (rc != OOKD_OK) return rc;
        }
    }
    const uint64_t *r = ctx->host.data() + (size_t)capture * kPulseWords;
    memset(out, 0, sizeof *out);
    for (uint32_t lv = 0; lv < 2; ++lv) {
        for (uint32_t b = 0; b < (uint32_t)kPulseBins; ++b) {
            out->count[lv][b] = r[2u * (lv * kPulseBins + b)];
            out->sum[lv][b] = r[2u * (lv * kPulseBins + b) + 1u];
            out->runs[lv] += out->count[lv][b];
        }
    }
    const uint64_t E = r[kPulseMetaWord];
    out->num_edges = E;
    out->samples = run.n_out;
    out->open_head = E ? r[kPulseMetaWord + 1] : run.n_out;
    out->open_tail = E ? run.n_out - r[kPulseMetaWord + 2] : 0;
    out->tail_level = (uint32_t)(E & 1u);
    return OOKD_OK;
}

}  // namespace

extern "C" {

uint32_t ookd_pulse_bin(uint64_t length) { return pulse_bin_of(length); }

uint64_t ookd_pulse_bin_lower(uint32_t bin) {
    if (bin < 32u) return bin;
    const uint64_t m = 16u + (bin - 32u) % 16u;         // five significant bits
    const uint32_t sh = 1u + (bin - 32u) / 16u;
    return sh > 59u ? UINT64_MAX : m << sh;
}

int ookd_rx_pulse_hist(ookd_rx *rx, uint32_t capture, ookd_pulse_hist *out) {
    return pulse_hist("ookd_rx_pulse_hist", false, rx, capture, out);
}

int ookd_rx_pulse_hist_clean(ookd_rx *rx, uint32_t capture, ookd_pulse_hist *out) {
    return pulse_hist("ookd_rx_pulse_hist_clean", true, rx, capture, out);
}

float ookd_rx_pulse_kernel_ms(const ookd_rx *rx) { return edge_pass_kernel_ms(rx, kEdgePassPulse); }

int ookd_suggest_pulses(const ookd_pulse_hist *h, double sample_rate, ookd_pulse_suggestion *out) {
    clear_error();
    if (!h || !out) {
        set_error("ookd_suggest_pulses: NULL argument");
        return OOKD_ERR_ARG;
    }
    memset(out, 0, sizeof *out);
    bool both = true;
    for (uint32_t lv = 0; lv < 2; ++lv) {
        std::vector<ClassAcc> cls;                      // ascending in length
        for (uint32_t b = 0; b < (uint32_t)kPulseBins; ++b) {
            if (!h->count[lv][b]) continue;
            if (cls.empty() || b - cls.back().last >= (uint32_t)OOKD_PULSE_CLASS_GAP) {
                cls.emplace_back();
                cls.back().first = b;
            }
            ClassAcc &c = cls.back();
            c.last = b;
            c.runs += h->count[lv][b];
            c.sum += h->sum[lv][b];
        }
        std::vector<uint32_t> keep(cls.size());
        for (uint32_t i = 0; i < keep.size(); ++i) keep[i] = i;
        if (keep.size() > (size_t)OOKD_PULSE_MAX_CLASSES) {
            // most runs first, the shorter class on a tie; then back into ascending order
            std::stable_sort(keep.begin(), keep.end(), [&](uint32_t a, uint32_t b) { return cls[a].runs > cls[b].runs; });
            for (size_t i = OOKD_PULSE_MAX_CLASSES; i < keep.size(); ++i) out->dropped_runs[lv] += cls[keep[i]].runs;
            keep.resize(OOKD_PULSE_MAX_CLASSES);
            std::sort(keep.begin(), keep.end());
        }
        bool two = false;
        for (uint32_t i = 0; i < keep.size(); ++i) {
            const ClassAcc &c = cls[keep[i]];
            ookd_pulse_class &o = out->classes[lv][i];
            o.first_bin = c.first;
            o.last_bin = c.last;
            o.runs = c.runs;
            o.mean = (double)c.sum / (double)c.runs;
            o.lower = ookd_pulse_bin_lower(c.first);
            o.upper = ookd_pulse_bin_lower(c.last + 1u) - 1u;
            o.mean_us = to_us(o.mean, sample_rate);
            o.lower_us = to_us((double)o.lower, sample_rate);
            o.upper_us = to_us((double)o.upper, sample_rate);
            two = two || c.runs >= 2;
        }
        out->num_classes[lv] = (uint32_t)keep.size();
        both = both && two;
    }
    out->found = both ? 1 : 0;
    return OOKD_OK;
}

}  // extern "C"
