// symbols.cpp -- symbol survey: the C ABI around symbols.hip's kernels, and the host-only half -- the class table,
// the coding rule, the device rule and the device JSON (include/ookiedokie_amd.h states all of them as a contract).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "clean.hpp"
#include "symbols.hpp"

using namespace ookd;

static_assert(OOKD_SYMBOL_MAX_CLASSES == kSymClasses && OOKD_SYMBOL_KINDS == kSymSide, "OOKD_SYMBOL_*");
static_assert(OOKD_FRAME_BINS == kFrameBins, "OOKD_FRAME_BINS");
static_assert(OOKD_SYMBOL_MAX_CLASSES == OOKD_PULSE_MAX_CLASSES, "a class table holds a pulse suggestion's classes");
static_assert(OOKD_ROLE_OTHER == kRoleOther && OOKD_ROLE_SYNC == kRoleSync && OOKD_ROLE_ZERO == kRoleZero &&
              OOKD_ROLE_ONE == kRoleOne, "OOKD_ROLE_*");
static_assert(sizeof(ookd_symbol_roles) == kSymKinds + 7u, "roles by key");

namespace ookd {

struct SymbolCtx : EdgePass {
    SymAgg *d_agg = nullptr;        // [tiles]
    SymCarry *d_carry = nullptr;    // [tiles]
    uint32_t tiles = 0;             // what d_agg / d_carry hold: every tile the context's edge list can have
    ~SymbolCtx() override {
        if (d_agg) (void)hipFree(d_agg);
        if (d_carry) (void)hipFree(d_carry);
    }
};

}  // namespace ookd

namespace {

bool table_ok(const ookd_symbol_table &t) {
    for (uint32_t lv = 0; lv < 2; ++lv) {
        if (t.num_classes[lv] > kSymClasses) return false;
        for (uint32_t k = 0; k < t.num_classes[lv]; ++k) {
            if (t.lower[lv][k] > t.upper[lv][k]) return false;
            if (k && t.lower[lv][k] <= t.upper[lv][k - 1]) return false;
        }
    }
    return true;
}

// the capture's pass: d_agg / d_carry on the first call, then the kernels' parameters and the timed sequence.
// list_capacity: the edges the context's own list holds -- a cleaned list is never longer
int compute(const char *who, SymbolCtx &c, const EdgeRun &run, uint64_t list_capacity, uint32_t capture,
            const ookd_symbol_table &table, const ookd_symbol_roles *roles, std::vector<uint64_t> &host) {
    if (!c.d_agg) {
        if (hipSetDevice(run.dev) != hipSuccess) {
            set_error("%s: hipSetDevice failed", who);
            return OOKD_ERR_HIP;
        }
        const uint32_t tiles = std::max<uint32_t>(sym_tiles_of(list_capacity), 1u);
        bool ok = hipMalloc(reinterpret_cast<void **>(&c.d_agg), (size_t)tiles * sizeof(SymAgg)) == hipSuccess;
        ok = ok && hipMalloc(reinterpret_cast<void **>(&c.d_carry), (size_t)tiles * sizeof(SymCarry)) == hipSuccess;
        if (!ok) {
            set_error("%s: device allocation failed: %s", who, hipGetErrorString(hipGetLastError()));
            if (c.d_agg) (void)hipFree(c.d_agg);
            c.d_agg = nullptr;
            c.d_carry = nullptr;
            return OOKD_ERR_NOMEM;
        }
        c.tiles = tiles;
    }
    SymParams p{};
    p.list = edge_list_view(run);
    p.capture = capture;
    p.num_tiles_cap = c.tiles;
    p.agg = c.d_agg;
    p.carry = c.d_carry;
    for (uint32_t lv = 0; lv < 2; ++lv) {
        p.num_classes[lv] = table.num_classes[lv];
        for (uint32_t k = 0; k < table.num_classes[lv]; ++k) {
            p.lower[lv][k] = table.lower[lv][k];
            p.upper[lv][k] = table.upper[lv][k];
        }
    }
    if (roles) memcpy(p.role, roles->role, kSymKinds);
    return c.run(who, run, host.size(), host.data(), [&](unsigned long long *d_result) {
        p.result = d_result;
        return launch_symbol_survey(p, roles != nullptr, run.num_edges, run.stream);
    });
}

// ookd_rx_symbol_survey (clean = false: the run's own edge list, pass kEdgePassSymbol) and ookd_rx_symbol_survey_clean
// (the cleaned list, pass kEdgePassCleanSymbol): the same kernels and the same contract over an EdgeListView of either
int symbol_survey(const char *who, bool clean, ookd_rx *rx, uint32_t capture, const ookd_symbol_table *table,
                  const ookd_symbol_roles *roles, ookd_symbol_survey *out) {
    const EdgePassId id = clean ? kEdgePassCleanSymbol : kEdgePassSymbol;
    clear_error();
    if (!table || !out) {
        set_error("%s: NULL argument", who);
        return OOKD_ERR_ARG;
    }
    if (rx) {                   // whatever happens below, the last call's time is no finished pass's
        if (EdgePass *c = ookd_rx_edge_pass(rx, id).get()) {
            c->serial = 0;
            c->kernel_ms = 0.0f;
        }
    }
    // the table and the roles first: they are judged without a context (and without a GPU)
    if (!table_ok(*table)) {
        set_error("%s: the class table needs at most %u ranges per level, lower <= upper, ascending and disjoint", who,
                  kSymClasses);
        return OOKD_ERR_ARG;
    }
    if (roles) {
        for (uint32_t i = 0; i < kSymKinds; ++i) {
            if ((&roles->role[0][0])[i] > OOKD_ROLE_ONE) {
                set_error("%s: role %u of kind (%u, %u)", who, (&roles->role[0][0])[i], i / kSymSide, i % kSymSide);
                return OOKD_ERR_ARG;
            }
        }
    }
    if (!rx) {
        set_error("%s: NULL argument", who);
        return OOKD_ERR_ARG;
    }
    EdgeRun run;
    if (const int rc = edge_run_check(who, rx, capture, run); rc != OOKD_OK) return rc;
    const uint64_t list_capacity = run.edge_capacity;
    if (clean && !clean_run_view(rx, run)) {
        set_error("%s: no cleaned list of the last run (ookd_rx_clean_edges first)", who);
        return OOKD_ERR_ARG;
    }
    memset(out, 0, sizeof *out);
    if (run.n_out == 0) return OOKD_OK;         // no buffer was processed: nothing was written for the kernels to read
    std::unique_ptr<EdgePass> &slot = ookd_rx_edge_pass(rx, id);
    if (!slot) slot.reset(new (std::nothrow) SymbolCtx());
    SymbolCtx *ctx = static_cast<SymbolCtx *>(slot.get());
    if (!ctx) {
        set_error("%s: out of memory", who);
        return OOKD_ERR_NOMEM;
    }
    std::vector<uint64_t> host(kSymWords, 0);
    const int rc = compute(who, *ctx, run, list_capacity, capture, *table, roles, host);
    if (rc != OOKD_OK) return rc;
    out->num_symbols = host[kSymWordS];
    memcpy(out->kinds, host.data() + kSymWordKinds, sizeof out->kinds);
    if (roles) {
        out->num_syncs = host[kSymWordSyncs];
        out->head_symbols = host[kSymWordSyncs + 1];
        out->tail_symbols = host[kSymWordSyncs + 2];
        memcpy(out->frames, host.data() + kSymWordFrames, sizeof out->frames);
    }
    return OOKD_OK;
}

struct Kind {
    uint32_t on, off;
    uint64_t count;
};

uint64_t to_us(double mean, double rate) { return (uint64_t)std::llround(mean / rate * 1e6); }

void put(std::string &s, const char *fmt, ...) __attribute__((format(printf, 2, 3)));
void put(std::string &s, const char *fmt, ...) {
    char buf[256];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    s += buf;
}

// the six states of the header's rule 7, as ookd_device_create takes them
struct SuggestedTables {
    uint64_t state_duration_us[6], state_timeout_us[6];
    uint32_t trig_begin[7];
    uint8_t trig_cond[12], trig_action[12];
    uint32_t trig_next[12];
    uint64_t trig_duration_us[12];
};
enum { kAlways = 1, kPulseStart, kPulseEnd, kTimeout, kMsgComplete };
enum { kNone = 1, kAppend0, kAppend1, kOutput };
const char *const kStateNames[6] = {"reset", "idle", "sync_pulse", "sync_gap", "bit_pulse", "bit_gap"};
const char *const kCondNames[6] = {"", "always", "pulse_start", "pulse_end", "timeout", "msg_complete"};
const char *const kActionNames[5] = {"", "none", "append_0", "append_1", "output_data"};

void suggested_tables(const ookd_device_suggestion &s, SuggestedTables &t) {
    const uint64_t dur[6] = {0, 0, s.sync_on_us, s.sync_off_us, s.bit_on_us, 0};
    const uint64_t to[6] = {0, 0, 2 * s.sync_on_us, 2 * s.sync_off_us, 2 * s.bit_on_us, 2 * s.one_off_us};
    memcpy(t.state_duration_us, dur, sizeof dur);
    memcpy(t.state_timeout_us, to, sizeof to);
    struct Trig {
        uint8_t cond, action;
        uint32_t next;
        uint64_t duration;
    };
    const Trig trigs[12] = {
        {kAlways, kNone, 1, 0},                                                                 // reset
        {kPulseStart, kNone, 2, 0},                                                             // idle
        {kPulseEnd, kNone, 3, 0}, {kTimeout, kNone, 0, 0},                                      // sync_pulse
        {kPulseStart, kNone, 4, 0}, {kTimeout, kNone, 0, 0},                                    // sync_gap
        {kMsgComplete, kOutput, 0, 0}, {kPulseEnd, kNone, 5, 0}, {kTimeout, kNone, 0, 0},       // bit_pulse
        {kPulseStart, kAppend0, 4, s.zero_off_us}, {kPulseStart, kAppend1, 4, s.one_off_us},    // bit_gap
        {kTimeout, kNone, 0, 0}};
    const uint32_t begin[7] = {0, 1, 2, 4, 6, 9, 12};
    memcpy(t.trig_begin, begin, sizeof begin);
    for (int i = 0; i < 12; ++i) {
        t.trig_cond[i] = trigs[i].cond;
        t.trig_action[i] = trigs[i].action;
        t.trig_next[i] = trigs[i].next;
        t.trig_duration_us[i] = trigs[i].duration;
    }
}

}  // namespace

extern "C" {

int ookd_symbol_table_from_pulses(const ookd_pulse_suggestion *pulses, ookd_symbol_table *out) {
    clear_error();
    if (!pulses || !out) {
        set_error("ookd_symbol_table_from_pulses: NULL argument");
        return OOKD_ERR_ARG;
    }
    memset(out, 0, sizeof *out);
    for (uint32_t lv = 0; lv < 2; ++lv) {
        const uint32_t n = std::min<uint32_t>(pulses->num_classes[lv], kSymClasses);
        out->num_classes[lv] = n;
        for (uint32_t k = 0; k < n; ++k) {
            out->lower[lv][k] = pulses->classes[lv][k].lower;
            out->upper[lv][k] = pulses->classes[lv][k].upper;
        }
    }
    return OOKD_OK;
}

int ookd_rx_symbol_survey(ookd_rx *rx, uint32_t capture, const ookd_symbol_table *table, const ookd_symbol_roles *roles,
                          ookd_symbol_survey *out) {
    return symbol_survey("ookd_rx_symbol_survey", false, rx, capture, table, roles, out);
}

int ookd_rx_symbol_survey_clean(ookd_rx *rx, uint32_t capture, const ookd_symbol_table *table, const ookd_symbol_roles *roles,
                                ookd_symbol_survey *out) {
    return symbol_survey("ookd_rx_symbol_survey_clean", true, rx, capture, table, roles, out);
}

float ookd_rx_symbol_kernel_ms(const ookd_rx *rx) { return edge_pass_kernel_ms(rx, kEdgePassSymbol); }

int ookd_suggest_coding(const ookd_pulse_suggestion *pulses, const ookd_symbol_survey *survey, ookd_symbol_roles *roles,
                        ookd_coding *out) {
    clear_error();
    if (!pulses || !survey || !roles || !out) {
        set_error("ookd_suggest_coding: NULL argument");
        return OOKD_ERR_ARG;
    }
    memset(roles, 0, sizeof *roles);
    memset(out, 0, sizeof *out);
    std::vector<Kind> kinds;                    // ascending (on, off): a stable sort keeps that order among equal counts
    for (uint32_t on = 0; on < kSymClasses; ++on)
        for (uint32_t off = 0; off < kSymClasses; ++off)
            if (survey->kinds[on][off]) kinds.push_back({on, off, survey->kinds[on][off]});
    std::stable_sort(kinds.begin(), kinds.end(), [](const Kind &a, const Kind &b) { return a.count > b.count; });
    if (kinds.size() < 3) {
        out->reason = OOKD_CODING_KINDS;
        return OOKD_OK;
    }
    Kind zero = kinds[0], one = kinds[1];
    if (zero.on != one.on) {
        out->reason = OOKD_CODING_NOT_DISTANCE;
        return OOKD_OK;
    }
    if (zero.off > one.off) std::swap(zero, one);       // classes ascend in length
    const double t0 = pulses->classes[0][zero.off].mean_us, t1 = pulses->classes[0][one.off].mean_us;
    out->data_on_class = zero.on;
    out->zero_off_class = zero.off;
    out->one_off_class = one.off;
    out->zero_count = zero.count;
    out->one_count = one.count;
    out->t0_us = t0;
    out->t1_us = t1;
    if (!(1.15 * t0 < 0.85 * t1)) {
        out->reason = OOKD_CODING_AMBIGUOUS;
        return OOKD_OK;
    }
    if (kinds[2].count < 2) {                   // (descending: no later kind has more)
        out->reason = OOKD_CODING_NO_SYNC;
        return OOKD_OK;
    }
    out->sync_on_class = kinds[2].on;
    out->sync_off_class = kinds[2].off;
    out->sync_count = kinds[2].count;
    roles->role[zero.on][zero.off] = OOKD_ROLE_ZERO;
    roles->role[one.on][one.off] = OOKD_ROLE_ONE;
    roles->role[kinds[2].on][kinds[2].off] = OOKD_ROLE_SYNC;
    out->found = 1;
    return OOKD_OK;
}

int ookd_suggest_device(const ookd_pulse_suggestion *pulses, const ookd_symbol_survey *survey, const ookd_coding *coding,
                        double sample_rate, ookd_device_suggestion *out) {
    clear_error();
    if (!pulses || !survey || !coding || !out || !(sample_rate > 0.0)) {
        set_error("ookd_suggest_device: needs pulses, a survey, a coding, an output and a sample rate > 0");
        return OOKD_ERR_ARG;
    }
    memset(out, 0, sizeof *out);
    out->num_syncs = survey->num_syncs;
    if (!coding->found) {
        out->reason = coding->reason ? coding->reason : (uint32_t)OOKD_CODING_KINDS;
        return OOKD_OK;
    }
    if (coding->data_on_class >= kSymClasses || coding->zero_off_class >= kSymClasses || coding->one_off_class >= kSymClasses ||
        coding->sync_on_class >= kSymClasses || coding->sync_off_class >= kSymClasses) {
        set_error("ookd_suggest_device: the coding names a class beyond %u", kSymClasses - 1u);
        return OOKD_ERR_ARG;
    }
    uint64_t all = 0, counted = 0;
    for (uint32_t c = 0; c < 2; ++c) {
        for (uint32_t d = 0; d < kFrameBins; ++d) {
            all += survey->frames[c][d];
            if (d >= 3u && d < kFrameBins - 1u) counted += survey->frames[c][d];
        }
    }
    uint32_t L = 3;
    for (uint32_t d = 3; d < kFrameBins - 1u; ++d)
        if (survey->frames[1][d] > survey->frames[1][L]) L = d;
    out->frames_seen = all;
    out->frames_counted = counted;
    out->frames_clean = survey->frames[1][L];
    if (out->frames_clean < 1 || 2 * out->frames_clean < counted) {
        out->reason = OOKD_CODING_NO_FRAMES;
        return OOKD_OK;
    }
    out->frame_symbols = L;
    out->num_bits = L - 2u;
    out->sync_on_us = to_us(pulses->classes[1][coding->sync_on_class].mean, sample_rate);
    out->sync_off_us = to_us(pulses->classes[0][coding->sync_off_class].mean, sample_rate);
    out->bit_on_us = to_us(pulses->classes[1][coding->data_on_class].mean, sample_rate);
    out->zero_off_us = to_us(pulses->classes[0][coding->zero_off_class].mean, sample_rate);
    out->one_off_us = to_us(pulses->classes[0][coding->one_off_class].mean, sample_rate);
    if (out->num_bits > 8u * OOKD_MAX_PAYLOAD_BYTES) {
        out->reason = OOKD_CODING_TOO_LONG;
        return OOKD_OK;
    }
    out->found = 1;
    return OOKD_OK;
}

ookd_device *ookd_device_from_suggestion(const ookd_device_suggestion *s, uint32_t sample_rate) {
    clear_error();
    if (!s || !s->found) {
        set_error("ookd_device_from_suggestion: no suggestion (found = 0)");
        return nullptr;
    }
    SuggestedTables st;
    suggested_tables(*s, st);
    ookd_fsm_tables t;
    memset(&t, 0, sizeof t);
    t.num_states = 6;
    t.max_bits = s->num_bits;
    t.sample_rate = sample_rate;
    t.num_triggers = 12;
    t.state_duration_us = st.state_duration_us;
    t.state_timeout_us = st.state_timeout_us;
    t.trig_begin = st.trig_begin;
    t.trig_cond = st.trig_cond;
    t.trig_action = st.trig_action;
    t.trig_next = st.trig_next;
    t.trig_duration_us = st.trig_duration_us;
    return ookd_device_create(&t);
}

size_t ookd_device_suggestion_json(const ookd_device_suggestion *s, const char *name, char *buf, size_t size) {
    clear_error();
    if (buf && size) buf[0] = '\0';
    if (!s || !name || !s->found) {
        set_error("ookd_device_suggestion_json: needs a suggestion with found = 1 and a name");
        return 0;
    }
    SuggestedTables st;
    suggested_tables(*s, st);
    std::string safe;
    for (const char *c = name; *c; ++c) {
        if (*c == '"' || *c == '\\') safe += '\\';
        safe += (unsigned char)*c < 0x20 ? ' ' : *c;
    }
    std::string j = "{ \"device\": {\n";
    put(j, "    \"name\": \"%s\",\n", safe.c_str());
    put(j, "    \"description\": \"suggested from a capture: %u bits, sync %llu / %llu us, bit %llu us + %llu or %llu us\",\n",
        s->num_bits, (unsigned long long)s->sync_on_us, (unsigned long long)s->sync_off_us, (unsigned long long)s->bit_on_us,
        (unsigned long long)s->zero_off_us, (unsigned long long)s->one_off_us);
    put(j, "    \"num_bits\": %u,\n    \"states\": [\n", s->num_bits);
    for (uint32_t i = 0; i < 6; ++i) {
        put(j, "        { \"name\": \"%s\",", kStateNames[i]);
        if (st.state_duration_us[i]) put(j, " \"duration_us\": %llu,", (unsigned long long)st.state_duration_us[i]);
        if (st.state_timeout_us[i]) put(j, " \"timeout_us\": %llu,", (unsigned long long)st.state_timeout_us[i]);
        j += "\n          \"triggers\": [\n";
        for (uint32_t k = st.trig_begin[i]; k < st.trig_begin[i + 1]; ++k) {
            put(j, "            { \"condition\": \"%s\",", kCondNames[st.trig_cond[k]]);
            if (st.trig_duration_us[k]) put(j, " \"duration_us\": %llu,", (unsigned long long)st.trig_duration_us[k]);
            put(j, " \"state\": \"%s\"", kStateNames[st.trig_next[k]]);
            if (st.trig_action[k] != kNone) put(j, ", \"action\": \"%s\"", kActionNames[st.trig_action[k]]);
            put(j, " }%s\n", k + 1 < st.trig_begin[i + 1] ? "," : "");
        }
        put(j, "          ] }%s\n", i + 1 < 6 ? "," : "");
    }
    j += "    ],\n    \"fields\": [\n";
    const uint32_t fields = (s->num_bits + 63u) / 64u;
    for (uint32_t f = 0; f < fields; ++f) {
        const uint32_t lo = 64u * f, hi = std::min(lo + 63u, s->num_bits - 1u);
        if (fields == 1) put(j, "        { \"name\": \"Payload\",");
        else put(j, "        { \"name\": \"Payload%u\",", f);
        put(j, " \"default\": \"0x0\", \"start_bit\": %u, \"end_bit\": %u, \"endianness\": \"big\", \"format\": \"hex\" }%s\n",
            lo, hi, f + 1 < fields ? "," : "");
    }
    j += "    ]\n}}\n";
    if (buf && size) {
        const size_t n = std::min(j.size(), size - 1);
        memcpy(buf, j.data(), n);
        buf[n] = '\0';
    }
    return j.size();
}

}  // extern "C"
