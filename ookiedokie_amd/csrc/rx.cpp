// rx.cpp -- rx context: HBM buffers, kernel sequencing, C ABI of the fused
// demodulation entry (replaces the body of the reference loop,
// src/ookiedokie.c:243-288, for whole captures resident in HBM).
#include <algorithm>
#include <atomic>
#include <cerrno>
#include <chrono>
#include <cinttypes>
#include <cmath>
#include <cstddef>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <utility>

#include "common.hpp"
#include "front_plan.hpp"
#include "ingest.hpp"
#include "kernels.hpp"
#include "edge_pass.hpp"
#include "run_levels.hpp"
#include "clean.hpp"

using namespace ookd;

namespace {

#define HIPCHK(expr)                                                              \
    do {                                                                          \
        hipError_t _e = (expr);                                                   \
        if (_e != hipSuccess) {                                                   \
            set_error("HIP error %d (%s) at %s:%d: %s", (int)_e,                  \
                      hipGetErrorString(_e), __FILE__, __LINE__, #expr);          \
            return OOKD_ERR_HIP;                                                  \
        }                                                                         \
    } while (0)

constexpr uint32_t kIterBatch = 4;      // FSM fix-point rounds queued per host sync

constexpr uint64_t kHostMsgFirst = 2048;    // messages copied with the header
constexpr uint64_t kErrListMax = 1ull << 25;    // entries (256 MiB) an error list is allowed: it is sized by the buffers of
                                                // the largest run, this only stops a tiny samples_per_buffer on a huge context

struct ResultHeader {
    uint32_t changed[kIterBatch];
    uint32_t flags;
    uint32_t edge_overflow;
    uint64_t totals[2];
    unsigned long long recompute;
    uint32_t total_edges;
    uint32_t scan_fallback;
    uint32_t sync_fail;         // the scan's walk from synchronising spans gave up (the composing kernels ran)
    uint32_t publish_done;      // workgroups of the scan's publishing kernel that are through
};

// one chunk of a pipelined single-capture run
struct Chunk {
    uint64_t out0, nout;        // decimated samples [out0, out0 + nout) of the capture
    uint32_t blk0, nblk;        // 4096-output blocks
    uint64_t edge_off, edge_cap;        // its region of the edge list
};
constexpr int kMaxChunks = 256;
constexpr uint64_t kPipeDefaultChunk = 1ull << 28;      // input samples
constexpr uint64_t kPipeTailChunk = 1ull << 25;         // the last chunks shrink down to this: a short exposed chain

}  // namespace

// Front-end kernels of contexts that share a gate take turns: they are HBM bound, so running two
// at once only makes both slower, while everything after them (edges, state machine: latency
// bound) overlaps the next context's front end.  The gate remembers the stop event of the
// front-end launch queued last (it rides on that kernel's dispatch: launch_front); a context
// makes its stream wait for it before launching its own -- no marker packets.  An explicit
// object handed to ookd_rx_create by the caller: there is no process-wide state.
struct ookd_rx_gate {
    std::mutex m;
    hipEvent_t last = nullptr;
};

namespace {

// A device allocation, freed with its owner.
template <typename T>
struct DevBuf {
    T *p = nullptr;
    size_t n = 0;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    DevBuf(DevBuf &&o) noexcept : p(std::exchange(o.p, nullptr)), n(std::exchange(o.n, 0)) {}
    DevBuf &operator=(DevBuf &&o) noexcept {
        std::swap(p, o.p);
        std::swap(n, o.n);
        return *this;
    }
    ~DevBuf() {
        if (p) (void)hipFree(p);
    }
    int alloc(size_t count) {
        n = count;
        if (count == 0) return OOKD_OK;
        hipError_t e = hipMalloc(reinterpret_cast<void **>(&p), count * sizeof(T));
        if (e != hipSuccess) {
            set_error("hipMalloc of %zu bytes failed: %s", count * sizeof(T), hipGetErrorString(e));
            p = nullptr;
            return OOKD_ERR_NOMEM;
        }
        return OOKD_OK;
    }
    // allocates and fills from host memory (an empty vector leaves the buffer empty)
    int upload(const std::vector<T> &v) {
        const int rc = alloc(v.size());
        if (rc != OOKD_OK || v.empty()) return rc;
        if (hipMemcpy(p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice) != hipSuccess) {
            set_error("upload of %zu bytes failed", v.size() * sizeof(T));
            return OOKD_ERR_HIP;
        }
        return OOKD_OK;
    }
};

// The scan's tables (fsm_scan.hip: build_scan_tables) and their device copies, uploaded once per context
struct ScanTablesDev {
    ScanTables h{};                 // host side: the domain D, S, max_bits, leaf_block and the reach counts are read here
    DevBuf<uint32_t> d_lt_off, d_lt_n0, d_lt_pk;    // span tables (empty = the scan simulates)
    DevBuf<uint32_t> d_lt_merged;   // their merged rows + the sync walk's tables
    DevBuf<uint16_t> d_reach;       // abstract codes a span can be entered in, then the per-level lists (empty = all)
    DevBuf<uint4> d_ltab;           // the scan kernels' LDS table image

    int upload(ScanTables &&t) {
        h = std::move(t);
        std::vector<uint16_t> reach = h.reach;
        reach.insert(reach.end(), h.reach_by_level.begin(), h.reach_by_level.end());
        int rc = d_reach.upload(reach);
        if (!h.n0.empty()) rc |= d_lt_off.upload(h.off) | d_lt_n0.upload(h.n0) | d_lt_pk.upload(h.pk);
        return rc | d_lt_merged.upload(h.merged) | d_ltab.upload(h.ltab);
    }
    void fill(FsmScanArgs &a) const {
        a.D = h.D;
        a.S = h.S;
        a.SNB = h.SNB;
        a.leaf_block = h.leaf_block;
        a.lt_off = d_lt_off.p;
        a.lt_n0 = d_lt_n0.p;
        a.lt_pk = d_lt_pk.p;
        a.lt_words = (uint32_t)(d_lt_off.n + d_lt_n0.n + d_lt_pk.n);
        a.lt_merged = d_lt_merged.p;
        a.lt_merged_words = h.merged_rows_words;
        a.lt_sync_words = (uint32_t)d_lt_merged.n;
        a.ltab = d_ltab.p;
        a.reach = d_reach.p;
        a.nreach = (uint32_t)h.reach.size();
        a.nreach_base = h.reach_base;
        a.nreach_lv[0] = h.reach_lv[0];
        a.nreach_lv[1] = h.reach_lv[1];
    }
};

// The front end's plan (front_plan.hpp: plan_front) and its device copies, uploaded once per context
struct FrontDev {
    FrontPlan plan;
    DevBuf<float> d_taps;
    DevBuf<uint16_t> d_mfma_a;      // A-fragment image of the matrix-core form (empty = packed-VALU form)
    DevBuf<float> d_ctaps;          // every carrier's complex taps
    DevBuf<TunedCarrierDev> d_carriers;     // the fused carrier kernel's table
    FrontParams base{};             // plan.fp with the device pointers: what does not change from run to run

    int upload(FrontPlan &&p) {
        plan = std::move(p);
        const int rc = d_taps.upload(plan.taps) | d_mfma_a.upload(plan.mfma.image) | d_ctaps.upload(plan.ctaps) |
                       d_carriers.upload(plan.carrier_tab);
        base = plan.fp;
        base.taps = d_taps.p;
        base.mfma_a = d_mfma_a.p;
        base.ctaps = d_ctaps.p;
        if (const char *dbg = dev_getenv("OOKD_MFMA_DEBUG")) base.mfma_debug = (uint32_t)atoi(dbg);
        return rc;
    }
};

// Which state does every trajectory settle in while the input stays low?
// Walks the tables from reset with no edges: only always / timeout /
// msg_complete triggers can fire.  Used only as the ASSUMED incoming state of
// a state machine segment (a wrong guess costs fix-point rounds, never
// correctness).
uint32_t quiet_state(const ookd_device &d) {
    const uint64_t NONE = ~0ull;
    uint32_t cur = 0, nbits = 0;
    uint64_t k = 0;
    const size_t ns = d.state_duration_us.size();
    for (size_t step = 0; step < 4 * ns + 8; ++step) {
        int fire = -1;
        uint64_t best = NONE;
        for (uint32_t t = d.trig_begin[cur]; t < d.trig_begin[cur + 1]; ++t) {
            uint64_t lo = d.trig_kmin[t];
            const uint8_t c = d.trig_cond[t];
            if (c == 4) {               // timeout
                if (d.state_kto[cur] == NONE) continue;
                lo = std::max(lo, d.state_kto[cur]);
            } else if (c == 5) {        // msg_complete
                if (nbits < d.num_bits) continue;
            } else if (c != 1) {        // pulse triggers need an edge
                continue;
            }
            const uint64_t first = std::max(k, lo);
            if (first > d.trig_kmax[t]) continue;
            if (first - k < best) {     // earliest in time, then first in file order
                best = first - k;
                fire = (int)t;
            }
        }
        if (fire < 0) return cur;
        const uint8_t act = d.trig_action[fire];
        if (act == 2 || act == 3) nbits++;
        cur = d.trig_next[fire];
        if (cur == 0) nbits = 0;
        k = 0;
    }
    return 0;
}

// kernels.hpp: kMaxStatesBig -- the packed tables of a device with more than 64 states / triggers
std::vector<uint32_t> big_tables(const ookd_device &d, uint32_t quiet) {
    const uint64_t NONE = ~0ull;
    auto c32 = [&](uint64_t v) { return v == NONE ? 0xffffffffu : (uint32_t)v; };       // finite bounds are < 2^31
    const size_t ns = d.state_duration_us.size(), nt = d.trig_cond.size();
    std::vector<uint32_t> w(kBigHeaderWords + kBigStateWords * ns + kBigTrigWords * nt);
    w[0] = (uint32_t)ns;
    w[1] = d.num_bits;
    w[2] = (uint32_t)nt;
    w[3] = quiet;
    for (size_t s = 0; s < ns; ++s) {
        uint32_t *r = &w[kBigHeaderWords + kBigStateWords * s];
        r[0] = c32(d.state_kmin[s]);
        r[1] = c32(d.state_kmax[s]);
        r[2] = c32(d.state_kto[s]);
        r[3] = d.trig_begin[s];
        r[4] = d.trig_begin[s + 1];
        bool irrelevant = d.state_kmin[s] == 0 && d.state_kmax[s] == NONE;
        for (uint32_t i = d.trig_begin[s]; i < d.trig_begin[s + 1]; ++i) {
            if (d.trig_kmin[i] != 0 || d.trig_kmax[i] != NONE) irrelevant = false;
            if (d.trig_cond[i] == 4 && d.state_kto[s] != NONE) irrelevant = false;
        }
        r[5] = irrelevant ? 1u : 0u;
    }
    for (size_t i = 0; i < nt; ++i) {
        uint32_t *r = &w[kBigHeaderWords + kBigStateWords * ns + kBigTrigWords * i];
        r[0] = c32(d.trig_kmin[i]);
        r[1] = c32(d.trig_kmax[i]);
        r[2] = (uint32_t)d.trig_cond[i] | ((uint32_t)d.trig_action[i] << 8) | ((uint32_t)d.trig_next[i] << 16);
    }
    return w;
}

void fill_fsm_tables(const ookd_device &d, FsmTablesDev &t) {
    const uint64_t NONE = ~0ull;
    const size_t ns = d.state_duration_us.size();
    const size_t nt = d.trig_cond.size();
    t.num_states = (uint32_t)ns;
    t.max_bits = d.num_bits;
    t.num_triggers = (uint32_t)nt;
    for (size_t i = 0; i < (size_t)kMaxTriggers; ++i) {
        t.trig_kmin[i] = 1;             // empty window: never matches
        t.trig_kmax[i] = 0;
    }
    for (size_t s = 0; s < (size_t)kMaxStates; ++s) {
        t.state_kmax[s] = NONE;
        t.state_kto[s] = NONE;
    }
    t.quiet_state = quiet_state(d);
    if (ns > (size_t)kMaxStates || nt > (size_t)kMaxTriggers) return;    // a big device: only the counts (its tables: big_tables)
    for (size_t s = 0; s < ns; ++s) {
        t.state_kmin[s] = d.state_kmin[s];
        t.state_kmax[s] = d.state_kmax[s];
        t.state_kto[s] = d.state_kto[s];
        t.state_tbeg[s] = d.trig_begin[s];
        t.state_tend[s] = d.trig_begin[s + 1];
        // k is irrelevant in a state with no duration, no live timeout and no
        // trigger duration windows
        bool irrelevant = d.state_kmin[s] == 0 && d.state_kmax[s] == NONE;
        for (uint32_t i = d.trig_begin[s]; i < d.trig_begin[s + 1]; ++i) {
            if (d.trig_kmin[i] != 0 || d.trig_kmax[i] != NONE) irrelevant = false;
            if (d.trig_cond[i] == 4 && d.state_kto[s] != NONE) irrelevant = false;
        }
        t.state_flags[s] = irrelevant ? 1u : 0u;
    }
    for (size_t i = 0; i < nt; ++i) {
        t.trig_kmin[i] = d.trig_kmin[i];
        t.trig_kmax[i] = d.trig_kmax[i];
        t.trig_info[i] = (uint32_t)d.trig_cond[i] | ((uint32_t)d.trig_action[i] << 8) |
                         ((uint32_t)d.trig_next[i] << 16);
    }
    t.quiet_state = quiet_state(d);
}

uint64_t gcd64(uint64_t a, uint64_t b) {
    while (b) {
        uint64_t t = a % b;
        a = b;
        b = t;
    }
    return a;
}

// The streams, events and pinned buffers of a context.  A base of ookd_rx, so that it is destroyed after
// ookd_rx's members: every device buffer is freed while the streams still exist (with the streams destroyed
// first, contexts created and destroyed in quick succession hung in their destruction).
struct RxHandles {
    int dev = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
    hipStream_t s_front = nullptr, s_chain = nullptr;   // chunk pipeline
    hipEvent_t ev_start = nullptr, ev_end = nullptr;
    std::vector<hipEvent_t> ev_c0, ev_c1;       // per chunk: front-end kernel start / stop
    ResultHeader *h_hdr = nullptr;  // pinned
    MsgDev *h_msgs = nullptr;       // pinned, msg_capacity
    Ingest ingest;                  // process_host's pinned double buffer (lazy)
    ~RxHandles() {
        for (hipEvent_t e : ev_c0) if (e) (void)hipEventDestroy(e);
        for (hipEvent_t e : ev_c1) if (e) (void)hipEventDestroy(e);
        if (ev_start) (void)hipEventDestroy(ev_start);
        if (ev_end) (void)hipEventDestroy(ev_end);
        if (s_front) (void)hipStreamDestroy(s_front);
        if (s_chain) (void)hipStreamDestroy(s_chain);
        if (h_hdr) (void)hipHostFree(h_hdr);
        if (h_msgs) (void)hipHostFree(h_msgs);
        for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e);
        if (own_stream && stream) (void)hipStreamDestroy(stream);
    }
};

}  // namespace

struct ookd_rx : RxHandles {
    ookd_rx_config cfg{};

    // the front end: filter, bands and bounds, the form that runs (constant for the life of the context)
    FrontDev front;
    uint32_t total_decim() const { return front.plan.total_decim; }
    uint64_t halo_needed() const { return front.plan.halo_needed; }
    uint32_t tile_bits() const { return front.plan.tile_bits; }     // bits per wave tile of the front-end kernel, 0 = generic kernel
    // carriers of a carrier context (ookd_rx_create_carriers), 0 for every other: K carriers of ONE capture, their
    // results where the K captures of a batched run would be (run_caps == K behind the front end)
    uint32_t num_carriers() const { return front.plan.carrier_context() ? (uint32_t)front.plan.carriers.size() : 0u; }
    hipError_t launch_carriers(const FrontParams &fp, hipEvent_t t0, hipEvent_t t1, uint64_t tile_begin, uint64_t tile_count);
    bool count_quiet = false;
    DevBuf<uint32_t> d_quiet;       // kQuietCounters spread counters (diagnostics), running totals
    std::vector<uint32_t> quiet_prev;       // what they held after the run before
    DevBuf<uint32_t> d_tile_info;   // per wave tile edge counts written by the tuned front-end kernels
    // sparse front-end output: quiet tiles store nothing; the tile infos carry the run's stamp and tiles
    // without it read as quiet (kernels.hpp: tile_live).  Extents of the previous run: a change of the
    // geometry zeroes them first.
    bool sparse = false;
    uint64_t dirty_tiles = 0, dirty_words_per_cap = 0;
    uint32_t dirty_tiles_per_cap = 0;
    uint32_t tile_stamp = 0;            // of the current run's front end, 1 .. kTileStampMax
    mutable bool bits_dense = false;    // stale tiles of the current run were zeroed (ookd_rx_get_bits)
    int densify_bits() const;
    // chunk pipeline (single-capture runs): front end on s_front, edges + state machine on s_chain, each
    // on its own half of the CUs
    bool pipe_ok = false;
    uint64_t pipe_chunk_in = 0;     // target input samples per chunk
    std::vector<Chunk> chunks;      // of the last run (empty: not pipelined)
    DevBuf<SegState> d_carry;       // [2] state handed from chunk to chunk
    DevBuf<uint64_t> d_chunk_totals;    // [2][2] messages / errors so far
    DevBuf<unsigned long long> d_fin_tickets;   // [kMaxChunks + 1] the finish kernel's stamped work counters: one per
                                                // chunk of a pipelined run, the last one for whole runs
    const void *last_iq = nullptr;  // arguments of the last run (a refused pipelined run is redone whole)
    uint64_t last_stride = 0;
    bool no_pipeline_once = false;
    uint32_t front_launches = 1;    // of the last run
    DevBuf<uint32_t> d_cap_fallback;        // [captures] the scan's per-capture refusal bits (batched runs)
    DevBuf<uint16_t> d_pre, d_blk_in;       // entry code of every leaf / block (scan_entry_kernel)
    DevBuf<uint16_t> d_rowz;                // merged-rows interval of every leaf (scan_entry_kernel)
    DevBuf<uint32_t> d_skipc;               // every leaf applied to the two skip codes (leaf kernel -> entry walk)
    DevBuf<uint32_t> d_sync_rec;            // the block records of the walk from synchronising spans
    uint64_t pre_plane = 0;                 // elements per plane of d_pre (4 planes when that walk can run)
    bool scan_sync = false;                 // try the walk from synchronising spans first
    // How the next scan is queued.  The walk alone while it works (the composing kernels behind it would only return
    // at once: five launches, ~25 us of the chain).  A run where it gives up is refused and queued again with the
    // composing kernels only; so are the next kSyncBackoff - 1 runs, then one run carries both, and its verdict
    // decides (a stream of captures of one kind settles in one form or the other).
    static constexpr uint32_t kSyncBackoff = 8;
    uint32_t sync_backoff = 0;              // runs left in the composing form
    uint64_t sync_min_edges = 20000;        // edge lists expected shorter than this are composed (OOKD_SYNC_MIN_EDGES: tests)
    uint32_t sync_mode = 0;                 // of the scan in flight: FsmScanArgs::sync_try
    std::vector<uint64_t> mixed_errs;       // error positions of a run whose refused captures were redone (host side)
    bool mixed_valid = false;
    uint64_t front_launch_outputs = 1ull << 29;    // decimated samples per front-end grid launch (all captures together)

    // device (state machine)
    bool have_fsm = false;
    uint32_t num_bits = 0;
    DevBuf<FsmTablesDev> d_tables;
    DevBuf<uint32_t> d_big;         // packed tables of a device with more than 64 states / triggers (kernels.hpp)
    bool big_device = false;

    // capacity
    uint64_t max_samples = 0;
    uint32_t max_captures = 1;
    uint64_t max_n_in = 0, max_n_out = 0, max_words = 0;
    uint32_t max_blocks = 0, max_segs_per_cap = 0;
    uint64_t seg_len = 0;
    uint32_t msg_slots = 0, err_slots = 0;
    uint64_t edge_capacity = 0, msg_capacity = 0;

    DevBuf<uint64_t> d_bits;
    DevBuf<float> d_fir;
    DevBuf<int16_t> d_halo;
    DevBuf<uint32_t> d_blk_count, d_blk_offset, d_group_total;
    DevBuf<uint64_t> d_edges, d_seg_bounds;
    DevBuf<SegState> d_state_in, d_state_out;
    DevBuf<MsgDev> d_seg_msgs, d_msgs;
    DevBuf<uint32_t> d_seg_msg_count, d_seg_err_count;
    DevBuf<uint64_t> d_seg_errs;
    DevBuf<ResultHeader> d_hdr;
    DevBuf<uint64_t> d_debug;

    // scan form of the state machine (fsm_scan.hip)
    bool scan_ok = false;           // device fits the scan's tables and it was not disabled
    std::unique_ptr<FsmTablesDev> h_tables;     // host copy of the device tables
    bool scan_used = false;         // the results of the last run come from the scan
    bool scan_pending = false;      // a scan is queued; its verdict is read with the results
    bool pending_first_valid = false;
    FsmStateDev pending_first{};
    ScanTablesDev scan_tab;         // its tables and what they say about the domain
    uint32_t scan_blocks_cap = 0;
    DevBuf<uint16_t> d_block_tab;
    DevBuf<uint32_t> d_cap_group_off, d_cap_super_off;
    DevBuf<uint16_t> d_group_tab, d_super_tab, d_super_in, d_cap_end;
    DevBuf<uint32_t> d_cap_block_off;
    DevBuf<LeafEvDev> d_events;
    DevBuf<uint32_t> d_ev_hot;
    DevBuf<uint8_t> d_app_vals;
    DevBuf<uint64_t> d_scan_errs;
    DevBuf<SegState> d_final_state;
    DevBuf<uint32_t> d_fin_off;
    DevBuf<uint64_t> d_fsum;                // 32 B per finish block: stamped aggregates
    uint32_t scan_fin_cap = 0;
    uint32_t scan_stamp = 0;        // stamps the finish kernel's block aggregates, never 0
    DevBuf<int16_t> d_stage_in;     // process_host staging (lazy)
    // 8-bit contexts, forms without a fused 8-bit kernel: the capture and the halo widened to SC16Q11
    // (allocated by the first run that takes such a form: widen_for_form)
    DevBuf<int16_t> d_widen, d_halo_w;

    ResultHeader *h_hdr_dev = nullptr;      // the same two through the device's mapping
    MsgDev *h_msgs_dev = nullptr;
    bool hdr_dirty = true;          // device header needs zeroing before the next run
    uint64_t num_msgs = 0;

    // geometry of the last run
    uint32_t run_caps = 0;
    uint64_t run_n_valid = 0, run_n_in = 0, run_n_out = 0, run_words = 0;
    uint32_t run_blocks = 0, run_segs_per_cap = 0;
    // what the edge-list readers (pulses.cpp, symbols.cpp) ask about the last run, and their passes (edge_pass.hpp)
    uint64_t run_serial = 0;        // runs started so far
    bool run_shard = false, run_overflow = false;
    bool run_edges_valid = false;   // collect_results has read this run's edge count: the prefix and the list are its own
    std::unique_ptr<EdgePass> edge_pass[kEdgePasses];   // each made by its reader's first call
    // debounce (ookd_rx_set_debounce): with a minimum above 1 every run cleans its edge list in the
    // chain (clean.hip) and the state machine reads the cleaned list and its per-block prefix in the place of the
    // run's own -- fsm_params hands them out, and with them the scan, the round form and the redo of refused captures
    uint64_t debounce_on = 0, debounce_off = 0;
    CleanChainView debounce_view;       // the clean pass's buffers, allocated by the setter for the context's capacity
    bool debounce() const { return debounce_on > 1 || debounce_off > 1; }
    uint32_t iter_next = 0;         // next FSM iteration number (parity continues)
    uint32_t final_parity = 0;
    ookd_rx_stats stats{};

    ookd_rx_gate *gate = nullptr;   // shared with other contexts by the caller, or null
    ~ookd_rx() {
        if (gate) {
            std::lock_guard<std::mutex> lock(gate->m);
            if (gate->last == ev[1]) gate->last = nullptr;      // ev[1] is destroyed with RxHandles
        }
        (void)hipSetDevice(dev);        // for what is freed after this body: the members, then RxHandles
    }

    void geometry(uint64_t n_valid, bool pad_to_buffer, uint64_t &n_in, uint64_t &n_out,
                  uint64_t &words, uint32_t &blocks, uint32_t &segs) const {
        const uint64_t spb = cfg.samples_per_buffer;
        n_in = pad_to_buffer ? ((n_valid + spb - 1) / spb) * spb : n_valid;
        n_out = n_in / total_decim();
        const uint64_t tiles = (n_out + kFirTile - 1) / kFirTile;
        words = tiles * (kFirTile / 64);
        blocks = (uint32_t)(words / kBlockWords);
        segs = (uint32_t)((n_out + seg_len - 1) / seg_len);
        if (segs == 0 && n_out > 0) segs = 1;
    }

    FrontParams front_params(const void *d_iq, uint64_t stride) const {
        FrontParams p = front.base;
        p.iq = static_cast<const int16_t *>(d_iq);
        p.cap_stride = stride;
        p.n_valid = run_n_valid;
        p.n_in = run_n_in;
        p.n_out = run_n_out;
        p.bits = d_bits.p;
        p.words_per_cap = run_words;
        p.fir_out = d_fir.p;            // (allocated with OOKD_RX_KEEP_FIR only)
        p.recompute_count = &d_hdr.p->recompute;
        p.quiet_count = count_quiet ? d_quiet.p : nullptr;
        p.tile_info = d_tile_info.p;
        p.tiles_per_cap = tile_bits() ? (uint32_t)(run_words * 64 / tile_bits()) : 0;
        p.sparse = sparse ? 1u : 0u;
        p.stamp_bits = tile_stamp << kTileStampShift;
        return p;
    }

    EdgeParams edge_params() const {
        EdgeParams e{};
        e.bits = d_bits.p;
        e.words_per_cap = run_words;
        e.n_out = run_n_out;
        e.num_captures = run_caps;
        e.blocks_per_cap = run_blocks;
        e.blk_count = d_blk_count.p;
        e.blk_offset = d_blk_offset.p;
        e.group_total = d_group_total.p;
        e.edges = d_edges.p;
        e.edge_capacity = edge_capacity;
        e.overflow = &d_hdr.p->edge_overflow;
        if (tile_bits() && d_tile_info.p) {
            e.tile_info = d_tile_info.p;
            e.tiles_per_block = (uint32_t)(kBlockWords * 64) / tile_bits();
            e.stamp_bits = tile_stamp << kTileStampShift;
        }
        return e;
    }

    FsmParams fsm_params() const {
        FsmParams f{};
        f.tables = d_tables.p;
        f.big = big_device ? d_big.p : nullptr;
        f.big_words = big_device ? (uint32_t)d_big.n : 0u;
        f.bits = d_bits.p;
        f.words_per_cap = run_words;
        f.edges = d_edges.p;
        f.blk_offset = d_blk_offset.p;
        f.blocks_per_cap = run_blocks;
        f.num_captures = run_caps;
        f.n_out = run_n_out;
        f.spb = cfg.samples_per_buffer;
        f.total_decim = total_decim();
        f.seg_len = seg_len;
        f.segs_per_cap = run_segs_per_cap;
        f.seg_bounds = d_seg_bounds.p;
        f.msg_slots = msg_slots;
        f.err_slots = err_slots;
        f.state_in = d_state_in.p;
        f.state_out = d_state_out.p;
        f.seg_msgs = d_seg_msgs.p;
        f.seg_msg_count = d_seg_msg_count.p;
        f.seg_errs = d_seg_errs.p;
        f.seg_err_count = d_seg_err_count.p;
        f.changed = d_hdr.p->changed;
        f.flags = &d_hdr.p->flags;
        f.msgs = d_msgs.p;
        f.msg_capacity = msg_capacity;
        f.totals = d_hdr.p->totals;
        f.debug = d_debug.p;
        f.edge_overflow = &d_hdr.p->edge_overflow;
        if (tile_bits() && d_tile_info.p) {
            f.tile_info = d_tile_info.p;
            f.tiles_per_cap = (uint32_t)(run_words * 64 / tile_bits());
            f.tile_shift = (uint32_t)__builtin_ctz(tile_bits());
            f.stamp_bits = tile_stamp << kTileStampShift;
        }
        if (debounce()) {
            f.edges = debounce_view.edges;
            f.blk_offset = debounce_view.blk_prefix;
            f.level_from_list = 1u;
        }
        return f;
    }

    uint32_t next_scan_stamp() {
        if (++scan_stamp == 0) scan_stamp = 1;
        return scan_stamp;
    }

    // sync_mode for the next run's scan (scan_args passes it on): called once per run
    void next_sync_mode() {
        sync_mode = 0;
        if (!scan_sync) return;
        // a short edge list goes through the composing kernels faster: the walk ends with its longest region (a few
        // hundred leaves at 0.14 us, whatever the capture's size) -- chain 131 against 153 us for the 46 000 edges of a
        // 1 GiB bench capture, 275 against 400 for the 737 000 of 16 GiB, about even at 20 000.  By the edge count of
        // this context's last run; before there is one, by the capture's length
        const uint64_t expect = stats.num_edges ? stats.num_edges : ((uint64_t)run_n_out * run_caps) >> 12;
        if (expect < sync_min_edges) return;
        if (sync_backoff == 0) sync_mode = 2;
        else sync_mode = (--sync_backoff == 0) ? 1u : 0u;
    }

    int front_and_edges(const void *d_iq, uint64_t stride, const int16_t *d_halo_ptr,
                        uint32_t halo_len);
    bool plan_chunks();
    int run_pipelined(const void *d_iq);
    int prepare_front(FrontParams &fp);
    int widen_for_form(FrontParams &fp);
    int run_state_machine(const FsmStateDev *first, bool fresh);
    FsmScanArgs scan_args() const;
    int fsm_scan(const FsmStateDev *first);
    int dump_scan_debug();
    int fsm_to_fixpoint(const FsmStateDev *first, bool fresh, bool force_first, const FsmParams *view = nullptr);
    int redo_refused_captures();
    int segment_errors_overflow() const;
    int fetch_results();
    int enqueue_publish();
    PublishParams publish_params() const;
    bool scan_published = false;    // the queued scan ends with the publish step
    int rearm_header(const ResultHeader &seen);
    int collect_results();
    bool submitted = false;         // a run is queued (ookd_rx_submit_device) and not yet waited for
};

// A new run of the front end: the next stamp.  Sparse output leaves the quiet tiles' words and infos
// alone -- whatever they hold carries an older stamp and reads as quiet -- so nothing is zeroed between
// runs, except when the geometry changes (rare; keeps "a zero info means zero words" simple to reason
// about) or the 16-bit stamp wraps (every 2^16 - 1 runs): then every tile the buffer may hold is zeroed.
// An 8-bit context about to run a form that only exists for SC16Q11 (anything but the OOKD_FRONT_*_8 numbers):
// the run's captures and halo go through the widening kernel into staging buffers, and the front end is
// pointed at those.  Test and fallback paths: the fused forms never come here and never pay for the buffer.
int ookd_rx::widen_for_form(FrontParams &fp) {
    const uint32_t form = front.plan.form;
    if (fp.sample_fmt == kFmtSc16 || form == OOKD_FRONT_NO_FILTER_8 || form == OOKD_FRONT_FIR1_MFMA_8 ||
        form == OOKD_FRONT_FIR2_MFMA_8) {
        return OOKD_OK;
    }
    // (a carrier context reads one capture whatever its carrier count: one staging copy)
    const bool one = num_carriers() != 0;
    if (!d_widen.p) {
        const int rc = d_widen.alloc(2 * (size_t)max_samples * (one ? 1u : max_captures) + 8);
        if (rc != OOKD_OK) return rc;
    }
    HIPCHK(launch_widen(fp.iq, fp.sample_fmt, d_widen.p, run_n_valid, one ? 1u : run_caps, fp.cap_stride, run_n_valid, stream));
    fp.iq = d_widen.p;
    fp.cap_stride = run_n_valid;
    if (fp.halo && fp.halo_len) {
        if (!d_halo_w.p) {
            const int rc = d_halo_w.alloc(2 * (halo_needed() + 4));
            if (rc != OOKD_OK) return rc;
        }
        HIPCHK(launch_widen(fp.halo, fp.sample_fmt, d_halo_w.p, fp.halo_len, 1, 0, 0, stream));
        fp.halo = d_halo_w.p;
    }
    fp.sample_fmt = kFmtSc16;
    return OOKD_OK;
}

int ookd_rx::prepare_front(FrontParams &fp) {
    if (!tile_bits()) return OOKD_OK;
    if (sparse) {
        const uint64_t tiles = (uint64_t)run_caps * fp.tiles_per_cap;
        const bool same = tiles == dirty_tiles && fp.tiles_per_cap == dirty_tiles_per_cap && run_words == dirty_words_per_cap;
        if (tile_stamp >= kTileStampMax) {
            const uint64_t wpt = tile_bits() / 64u;
            const uint64_t all = std::min<uint64_t>(std::min<uint64_t>(d_tile_info.n, d_bits.n / wpt), 0xfffffff8ull) & ~(uint64_t)7;
            // (the tile -> words mapping is linear: the whole buffer as one capture)
            HIPCHK(launch_clear_tiles(d_tile_info.p, d_bits.p, all, (uint32_t)all, all * wpt, tile_bits(), 0u, stream));
            tile_stamp = 0;
        } else if (!same && dirty_tiles) {
            HIPCHK(launch_clear_tiles(d_tile_info.p, d_bits.p, dirty_tiles, dirty_tiles_per_cap, dirty_words_per_cap,
                                      tile_bits(), 0u, stream));
        }
        dirty_tiles = tiles;
        dirty_tiles_per_cap = fp.tiles_per_cap;
        dirty_words_per_cap = run_words;
    } else if (tile_stamp >= kTileStampMax) {
        tile_stamp = 0;         // dense output rewrites every tile of a run
    }
    ++tile_stamp;
    bits_dense = !sparse;
    fp.stamp_bits = tile_stamp << kTileStampShift;
    return OOKD_OK;
}

// Readers of the raw bit words (ookd_rx_get_bits) want the quiet tiles zero: zero what earlier runs
// left in the current run's extents.
int ookd_rx::densify_bits() const {
    if (bits_dense || !sparse || !dirty_tiles) return OOKD_OK;
    HIPCHK(launch_clear_tiles(d_tile_info.p, d_bits.p, dirty_tiles, dirty_tiles_per_cap, dirty_words_per_cap, tile_bits(),
                              tile_stamp << kTileStampShift, stream));
    HIPCHK(hipStreamSynchronize(stream));
    bits_dense = true;
    return OOKD_OK;
}

// ---------------------------------------------------------------------------
// chunk pipeline
// ---------------------------------------------------------------------------
// A long single capture is cut into chunks at multiples of lcm(4096 outputs,
// samples_per_buffer): chunk boundaries are buffer boundaries (the
// drop-rest-of-buffer rule stays chunk-local) and edge-block boundaries.  The
// front end of chunk c+1 (s_front) runs while the edges + state machine of
// chunk c (s_chain) run; each stream owns one half of the CUs, spread evenly
// over the XCDs -- the front end is HBM bound and as fast on half the chip
// (tools/cu_mask_probe.py), the chain's kernels no longer wait for a wave slot
// beside a grid that refills every one it frees.  Every chunk is a shard of
// the capture for the state machine: positions chunk-local, the level in
// front of it counted as 0, the incoming state = the chunk before's outgoing
// state, in device memory.  Messages / errors are appended behind the chunks
// before's.  A refusal of the scan anywhere sends the whole capture through
// the unchunked path.
bool ookd_rx::plan_chunks() {
    chunks.clear();
    if (!pipe_ok || no_pipeline_once || run_caps != 1 || run_n_out == 0) return false;
    if (debounce()) return false;       // (chunk-local lists and carried levels are not cleaned: as with pipeline = false)
    const uint64_t spb = cfg.samples_per_buffer;
    // boundary (decimated index) o: o % 4096 == 0 and o * D % spb == 0
    const uint64_t per_buf = spb / gcd64(spb, total_decim());
    const uint64_t align = (uint64_t)kFirTile / gcd64(kFirTile, per_buf) * per_buf;
    const uint64_t target = std::max<uint64_t>(align, pipe_chunk_in / total_decim() / align * align);
    if (run_n_out < 2 * target) return false;
    std::vector<uint64_t> sizes;
    uint64_t left = run_n_out;
    while (left > target + target / 2) {
        sizes.push_back(target);
        left -= target;
    }
    // the tail shrinks: the chain of the last chunk is all that is not hidden behind a front end
    const uint64_t tail_min = std::max<uint64_t>(align, kPipeTailChunk / total_decim() / align * align);
    while (left > 2 * tail_min && sizes.size() + 2 < (size_t)kMaxChunks) {
        uint64_t half = left / 2 / align * align;
        if (half < tail_min) break;
        sizes.push_back(half);
        left -= half;
    }
    sizes.push_back(left);
    if (sizes.size() < 2 || sizes.size() > (size_t)kMaxChunks) return false;
    uint64_t at = 0, eoff = 0;
    for (uint64_t sz : sizes) {
        Chunk c{};
        c.out0 = at;
        c.nout = sz;
        c.blk0 = (uint32_t)(at / kFirTile);
        c.nblk = (uint32_t)((sz + kFirTile - 1) / kFirTile);
        c.edge_off = eoff;
        c.edge_cap = edge_capacity / run_blocks * c.nblk;       // its share of the list, by blocks
        eoff += c.edge_cap;
        at += sz;
        chunks.push_back(c);
    }
    return true;
}

int ookd_rx::run_pipelined(const void *d_iq) {
    const size_t nc = chunks.size();
    while (ev_c0.size() < nc) {
        hipEvent_t a = nullptr, b = nullptr;
        HIPCHK(hipEventCreate(&a));
        ev_c0.push_back(a);
        HIPCHK(hipEventCreate(&b));
        ev_c1.push_back(b);
    }
    if (hdr_dirty) HIPCHK(hipMemsetAsync(d_hdr.p, 0, sizeof(ResultHeader), stream));
    hdr_dirty = true;
    FrontParams fp = front_params(d_iq, run_n_valid);
    {
        int rc = widen_for_form(fp);
        if (rc == OOKD_OK) rc = prepare_front(fp);
        if (rc != OOKD_OK) return rc;
    }
    HIPCHK(hipEventRecord(ev_start, stream));
    HIPCHK(hipStreamWaitEvent(s_front, ev_start, 0));
    HIPCHK(hipStreamWaitEvent(s_chain, ev_start, 0));

    const uint32_t tiles_per_block = (uint32_t)kFirTile / tile_bits();
    scan_used = false;
    scan_pending = true;
    stats.fsm_path = 0;
    stats.scan_entry_form = 0;
    stats.fsm_fallback_reason = 0;
    pending_first_valid = false;
    // every front-end launch first: the device starts on the capture at once and is not held up by
    // the host still queueing the (ten times as many) chain kernels behind
    for (size_t c = 0; c < nc; ++c) {
        const Chunk &ch = chunks[c];
        HIPCHK(launch_front(fp, 1, front.plan.exact, s_front, ev_c0[c], ev_c1[c], (uint64_t)ch.blk0 * tiles_per_block,
                            (uint64_t)ch.nblk * tiles_per_block));
    }
    // one scan form for every chunk: a refusal anywhere redoes the capture whole
    next_sync_mode();
    for (size_t c = 0; c < nc; ++c) {
        const Chunk &ch = chunks[c];
        const bool last = c + 1 == nc;
        HIPCHK(hipStreamWaitEvent(s_chain, ev_c1[c], 0));
        // ---- its edges: chunk-local positions (the run is one capture) -------------------------------------
        EdgeParams e = edge_params();
        e.bits = d_bits.p + (size_t)ch.blk0 * kBlockWords;
        e.words_per_cap = (uint64_t)ch.nblk * kBlockWords;
        e.n_out = ch.nout;
        e.blocks_per_cap = ch.nblk;
        e.blk_count = d_blk_count.p + ch.blk0;
        e.blk_offset = d_blk_offset.p + ch.blk0 + c;            // nblk + 1 entries per chunk
        e.edges = d_edges.p + ch.edge_off;
        e.edge_capacity = ch.edge_cap;
        e.tile_info = d_tile_info.p + (size_t)ch.blk0 * tiles_per_block;
        e.total_acc = &d_hdr.p->total_edges;
        e.has_prev = c ? 1u : 0u;
        HIPCHK(launch_edges(e, s_chain));
        // ---- its state machine, from the chunk before's outgoing state --------------------------------------
        FsmScanArgs a = scan_args();
        a.f.bits = e.bits;
        a.f.tile_info = e.tile_info;
        a.f.words_per_cap = e.words_per_cap;
        a.f.edges = e.edges;
        a.f.blk_offset = e.blk_offset;
        a.f.blocks_per_cap = ch.nblk;
        a.f.n_out = ch.nout;
        a.f.totals = last ? d_hdr.p->totals : d_chunk_totals.p + 2 * (c & 1);
        if (last) {
            a.publish.total_edges = nullptr;        // accumulated in the header by the edge stages
        } else {
            // messages go to the host as they are resolved; the header only with the last chunk
            PublishParams pp{};
            pp.d_msgs = reinterpret_cast<const uint4 *>(d_msgs.p);
            pp.h_msgs = reinterpret_cast<uint4 *>(h_msgs_dev);
            pp.first_msgs = std::min<uint64_t>(kHostMsgFirst, msg_capacity);
            a.publish = pp;
        }
        a.first_dev = c ? d_carry.p + ((c - 1) & 1) : nullptr;
        a.pos_origin = ch.out0;
        a.totals_in = c ? d_chunk_totals.p + 2 * ((c - 1) & 1) : nullptr;
        a.final_state = d_carry.p + (c & 1);
        a.fin_ticket = d_fin_tickets.p + c;
        a.run_stamp = next_scan_stamp();
        HIPCHK(launch_fsm_scan(a, s_chain, last ? ev[2] : nullptr));
    }
    scan_published = true;
    HIPCHK(hipEventRecord(ev_end, s_chain));
    HIPCHK(hipStreamWaitEvent(stream, ev_end, 0));
    return OOKD_OK;
}

// The front end of a carrier context: the fused kernel for all carriers (OOKD_FRONT_TUNED_MULTI), or the fused
// two-stage kernel (OOKD_FRONT_TUNED_FIR2) or the generic tuned kernel once per carrier, each launch with that
// carrier's taps, threshold (band, quiet weights) and result planes.
hipError_t ookd_rx::launch_carriers(const FrontParams &fp, hipEvent_t t0, hipEvent_t t1, uint64_t tile_begin,
                                    uint64_t tile_count) {
    const uint32_t K = num_carriers();
    if (fp.n_out != 0 && front.plan.form == OOKD_FRONT_TUNED_MULTI) {
        return launch_front_tuned_multi(fp, front.d_carriers.p, K, stream, t0, t1, tile_begin, tile_count);
    }
    if (fp.n_out != 0 && front.plan.form == OOKD_FRONT_TUNED_FIR2) {
        // carrier k is the tuned context's launch on capture plane k; the time stamps ride on the first and the last
        for (uint32_t k = 0; k < K; ++k) {
            const CarrierPlan &c = front.plan.carriers[k];
            FrontParams pk = fp;
            pk.ctaps = fp.ctaps + c.tap_off;
            pk.p_star = c.p_star;
            pk.p_lo = c.p_lo;
            pk.p_hi = c.p_hi;
            pk.quiet_a = c.quiet_a;
            pk.quiet_b = c.quiet_b;
            pk.bits = fp.bits + (size_t)k * run_words;
            pk.tile_info = fp.tile_info + (size_t)k * fp.tiles_per_cap;
            if (fp.fir_out) pk.fir_out = fp.fir_out + 2 * (size_t)k * run_n_out;
            const hipError_t e = launch_front_tuned_fir2(pk, 1, stream, k == 0 ? t0 : nullptr, k + 1 == K ? t1 : nullptr,
                                                         tile_begin, tile_count);
            if (e != hipSuccess) return e;
        }
        return hipSuccess;
    }
    if (tile_begin != 0 || tile_count != ~0ull) return hipErrorInvalidValue;    // the generic kernel runs whole captures
    if (t0 && hipEventRecord(t0, stream) != hipSuccess) return hipGetLastError();
    for (uint32_t k = 0; k < K && fp.n_out != 0; ++k) {
        FrontParams pk = fp;
        pk.ctaps = fp.ctaps + front.plan.carriers[k].tap_off;
        pk.p_star = front.plan.carriers[k].p_star;
        pk.bits = fp.bits + (size_t)k * run_words;
        if (fp.fir_out) pk.fir_out = fp.fir_out + 2 * (size_t)k * run_n_out;
        const hipError_t e = launch_front_tuned_generic(pk, 1, stream);
        if (e != hipSuccess) return e;
    }
    if (t1 && hipEventRecord(t1, stream) != hipSuccess) return hipGetLastError();
    return hipSuccess;
}

int ookd_rx::front_and_edges(const void *d_iq, uint64_t stride, const int16_t *d_halo_ptr,
                             uint32_t halo_len) {
    if (hdr_dirty) HIPCHK(hipMemsetAsync(d_hdr.p, 0, sizeof(ResultHeader), stream));
    hdr_dirty = true;
    FrontParams fp = front_params(d_iq, stride);
    fp.halo = d_halo_ptr;
    fp.halo_len = halo_len;
    {
        int rc = widen_for_form(fp);
        if (rc == OOKD_OK) rc = prepare_front(fp);
        if (rc != OOKD_OK) return rc;
    }
    // The tuned kernels go out as several grid launches of front_launch_tiles wave tiles: while a
    // grid has workgroups left to dispatch, kernels of OTHER queues (the edges / state machine
    // chain of the capture before, on another context's stream) are hardly dispatched at all --
    // they get their turn when a front-end launch has drained (profiles/r02_pipeline_trace.txt),
    // and once dispatched they run beside the next launch.  ev[0] / ev[1] = start of the first,
    // end of the last launch.
    const uint64_t tiles = tile_bits() ? (uint64_t)fp.tiles_per_cap : 0;
    // (a carrier context's grid covers the one capture it reads, whatever its carrier count)
    const uint32_t read_caps = num_carriers() ? 1u : run_caps;
    const uint64_t per = tile_bits() ? std::max<uint64_t>(1, front_launch_outputs / tile_bits() / std::max(1u, read_caps)) : 0;
    auto launch_range = [&](hipEvent_t e0, hipEvent_t e1, uint64_t t, uint64_t n) -> hipError_t {
        if (num_carriers()) return launch_carriers(fp, e0, e1, t, n);
        return launch_front(fp, run_caps, front.plan.exact, stream, e0, e1, t, n);
    };
    auto launch_all = [&]() -> hipError_t {
        front_launches = 1;
        if (!tile_bits() || tiles <= per + per / 2) return launch_range(ev[0], ev[1], 0, ~0ull);
        front_launches = (uint32_t)((tiles + per - 1) / per);
        for (uint64_t t = 0; t < tiles; t += per) {
            const bool first = t == 0, last = t + per >= tiles;
            const hipError_t e = launch_range(first ? ev[0] : nullptr, last ? ev[1] : nullptr, t, per);
            if (e != hipSuccess) return e;
        }
        return hipSuccess;
    };
    if (gate) {
        // wait + launch + publish under the lock: the event must be on its way before another
        // context may wait for it
        std::lock_guard<std::mutex> lock(gate->m);
        hipEvent_t prev = gate->last;
        if (prev && prev != ev[1]) HIPCHK(hipStreamWaitEvent(stream, prev, 0));
        HIPCHK(launch_all());
        gate->last = ev[1];
    } else {
        HIPCHK(launch_all());
    }
    if (run_n_out > 0) HIPCHK(launch_edges(edge_params(), stream));
    if (debounce()) {
        // the clean pass behind the edge stage, on the same stream: nothing here waits for the device
        EdgeRun run;
        ookd_rx_edge_run(this, &run);
        HIPCHK(clean_chain_queue(this, run, debounce_on, debounce_off));
    }
    return OOKD_OK;
}

// Runs segment-parallel state machine rounds until no segment's incoming
// state changes.  fresh: (re)initialise every segment's assumed state.
// view: the geometry to run on instead of the whole run's (one capture of a batch: redo_refused_captures)
int ookd_rx::fsm_to_fixpoint(const FsmStateDev *first, bool fresh, bool force_first, const FsmParams *view) {
    if (!have_fsm || run_n_out == 0) {
        HIPCHK(hipEventRecord(ev[2], stream));
        return OOKD_OK;
    }
    const FsmParams fp = view ? *view : fsm_params();
    if (fresh) {
        HIPCHK(launch_fsm_prepare(fp, first, stream));
        iter_next = 0;
    } else if (force_first) {
        // refine: new incoming state for segment 0 of the (single) capture
        // (the FsmStateDev is the leading member of SegState; skip_to stays 0:
        // shards start on buffer boundaries)
        HIPCHK(hipMemcpyAsync(d_state_in.p, first, sizeof(FsmStateDev), hipMemcpyHostToDevice, stream));
    }
    uint32_t rounds = 0;
    uint32_t mode = fresh ? 0u : (force_first ? 2u : 1u);
    for (;;) {
        HIPCHK(hipMemsetAsync(d_hdr.p->changed, 0, sizeof(uint32_t) * kIterBatch, stream));
        const uint32_t batch_mode0 = mode;
        for (uint32_t i = 0; i < kIterBatch; ++i) {
            HIPCHK(launch_fsm_round(fp, iter_next & 1u, mode, i, stream));
            iter_next++;
            mode = 1;
        }
        HIPCHK(hipMemcpyAsync(h_hdr->changed, d_hdr.p->changed, sizeof(uint32_t) * kIterBatch,
                              hipMemcpyDeviceToHost, stream));
        HIPCHK(hipStreamSynchronize(stream));
        rounds += kIterBatch;
        if (getenv("OOKD_DEBUG")) {
            fprintf(stderr, "[ookd] fsm batch mode0=%u changed:", batch_mode0);
            for (uint32_t i = 0; i < kIterBatch; ++i) fprintf(stderr, " %u", h_hdr->changed[i]);
            fprintf(stderr, " (segments %u)\n", run_caps * run_segs_per_cap);
        }
        // converged once an incremental round reran nothing (a mode-0 round
        // reruns everything and reports no count; a mode-2 round counts the
        // forced first segments)
        bool conv = false;
        for (uint32_t i = 0; i < kIterBatch && !conv; ++i) {
            const bool incremental = !(i == 0 && batch_mode0 != 1u);
            if (incremental && h_hdr->changed[i] == 0) conv = true;
        }
        if (conv) break;
        // every round settles at least one more segment's incoming state, left to right: a capture of
        // S segments is through after at most S + 1 rounds -- more would be a bug, not a hard input
        // (captures are independent chains of segs_per_cap segments: the bound is per capture, and it IS the
        //  check -- a fix-point that has not closed by then is a bug, not a hard input)
        if (rounds > fp.segs_per_cap + 2 * kIterBatch) {
            set_error("state machine fix-point did not converge in %u rounds", rounds);
            return OOKD_ERR_ARG;
        }
    }
    if (d_debug.p && !view) {
        const size_t nseg = (size_t)run_caps * run_segs_per_cap;
        std::vector<uint64_t> dbg(nseg * 4);
        HIPCHK(hipMemcpy(dbg.data(), d_debug.p, dbg.size() * 8, hipMemcpyDeviceToHost));
        uint64_t turns = 0, cyc = 0, fused = 0, loads = 0, maxcyc = 0, maxturns = 0;
        for (size_t i = 0; i < nseg; ++i) {
            turns += dbg[4 * i];
            cyc += dbg[4 * i + 1];
            fused += dbg[4 * i + 2];
            loads += dbg[4 * i + 3];
            maxcyc = std::max(maxcyc, dbg[4 * i + 1]);
            maxturns = std::max(maxturns, dbg[4 * i]);
        }
        fprintf(stderr, "[ookd] fsm last-run per segment: turns avg %.1f max %llu, fused %.1f, window loads %.1f, "
                        "memtime ticks avg %.0f max %llu\n",
                (double)turns / nseg, (unsigned long long)maxturns, (double)fused / nseg, (double)loads / nseg,
                (double)cyc / nseg, (unsigned long long)maxcyc);
    }
    final_parity = (iter_next - 1) & 1u;
    stats.fsm_iterations = rounds;
    HIPCHK(launch_fsm_gather(fp, stream));
    if (!view) HIPCHK(hipEventRecord(ev[2], stream));
    return OOKD_OK;
}

// A batched run in which the scan refused some captures (their path left its model): the scan's
// results for all the others stand; each refused capture is redone alone in the round form and
// its messages / errors are merged in, in capture order.  (Round 1 sent the whole call -- every
// capture of the batch -- through the rounds.)
// The round form ran out of error slots in a segment (header flag 4): only where setup_run_buffers had to cap them
int ookd_rx::segment_errors_overflow() const {
    set_error("a state machine segment reported more than %u errors (the context's error lists are capped at %llu "
              "positions: raise ookd_rx_config.samples_per_buffer or lower segment_buffers)", err_slots,
              (unsigned long long)kErrListMax);
    return OOKD_ERR_CAPACITY;
}

int ookd_rx::redo_refused_captures() {
    std::vector<uint32_t> flags(run_caps);
    HIPCHK(hipMemcpy(flags.data(), d_cap_fallback.p, run_caps * sizeof(uint32_t), hipMemcpyDeviceToHost));
    const uint64_t first = std::min<uint64_t>(kHostMsgFirst, msg_capacity);
    const uint64_t total = std::min<uint64_t>(h_hdr->totals[0], msg_capacity);
    std::vector<MsgDev> merged(h_msgs, h_msgs + std::min(total, first));
    if (total > first) {
        merged.resize(total);
        HIPCHK(hipMemcpy(merged.data() + first, d_msgs.p + first, (total - first) * sizeof(MsgDev), hipMemcpyDeviceToHost));
    }
    mixed_errs.resize(std::min<uint64_t>(h_hdr->totals[1], d_scan_errs.n));
    if (!mixed_errs.empty()) {
        HIPCHK(hipMemcpy(mixed_errs.data(), d_scan_errs.p, mixed_errs.size() * 8, hipMemcpyDeviceToHost));
    }
    uint64_t nerr = h_hdr->totals[1];
    uint32_t reasons = 0, rounds = 0;
    for (uint32_t cap = 0; cap < run_caps; ++cap) {
        if (!flags[cap]) continue;
        reasons |= flags[cap];
        FsmParams one = fsm_params();
        one.bits += (size_t)cap * run_words;
        if (one.tile_info) one.tile_info += (size_t)cap * one.tiles_per_cap;
        one.blk_offset += (size_t)cap * run_blocks;     // (its entries are offsets into the one edge list)
        one.num_captures = 1;
        HIPCHK(hipMemsetAsync(d_hdr.p, 0, sizeof(ResultHeader), stream));
        int rc = fsm_to_fixpoint(nullptr, true, false, &one);
        if (rc != OOKD_OK) return rc;
        rounds += stats.fsm_iterations;
        // (the gather is queued behind the last round, unwaited for; the copies below run on the null stream, which
        //  this non-blocking stream does not order itself against: without the wait they could read the totals and the
        //  list before the gather wrote them, and the capture came back with no messages)
        HIPCHK(hipStreamSynchronize(stream));
        ResultHeader hdr;
        HIPCHK(hipMemcpy(&hdr, d_hdr.p, sizeof(hdr), hipMemcpyDeviceToHost));
        if (hdr.flags & 1u) {
            set_error("a state machine segment produced more than %u messages "
                      "(raise ookd_rx_config.message_slots)", msg_slots);
            return OOKD_ERR_CAPACITY;
        }
        if (hdr.flags & 4u) return segment_errors_overflow();
        const uint64_t m = std::min<uint64_t>(hdr.totals[0], msg_capacity);
        const size_t at = merged.size();
        merged.resize(at + m);
        if (m) HIPCHK(hipMemcpy(merged.data() + at, d_msgs.p, m * sizeof(MsgDev), hipMemcpyDeviceToHost));
        for (size_t i = at; i < merged.size(); ++i) merged[i].capture = cap;
        // its errors, from the per-segment lists
        const size_t nseg = run_segs_per_cap;
        std::vector<uint32_t> counts(nseg);
        std::vector<uint64_t> errs(nseg * err_slots);
        HIPCHK(hipMemcpy(counts.data(), d_seg_err_count.p, nseg * 4, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(errs.data(), d_seg_errs.p, errs.size() * 8, hipMemcpyDeviceToHost));
        for (size_t sgi = 0; sgi < nseg; ++sgi) {
            for (uint32_t i = 0; i < std::min<uint32_t>(counts[sgi], err_slots); ++i) mixed_errs.push_back(errs[sgi * err_slots + i]);
        }
        nerr += hdr.totals[1];
    }
    HIPCHK(hipMemsetAsync(d_hdr.p, 0, sizeof(ResultHeader), stream));
    HIPCHK(hipStreamSynchronize(stream));
    hdr_dirty = false;
    std::stable_sort(merged.begin(), merged.end(), [](const MsgDev &a, const MsgDev &b) { return a.capture < b.capture; });
    if (merged.size() > msg_capacity) {
        set_error("message list overflow: %zu messages, capacity %llu", merged.size(), (unsigned long long)msg_capacity);
        return OOKD_ERR_CAPACITY;
    }
    if (!merged.empty()) memcpy(h_msgs, merged.data(), merged.size() * sizeof(MsgDev));
    num_msgs = merged.size();
    stats.num_messages = merged.size();
    stats.num_errors = nerr;
    stats.fsm_path = 3;                 // the scan, with the rounds for what it refused
    stats.fsm_fallback_reason = reasons;
    stats.fsm_iterations = rounds;
    mixed_valid = true;
    return OOKD_OK;
}

// The state machine over the current edge list: scan form when possible,
// segment/round form otherwise (or when the scan refuses the capture).
int ookd_rx::run_state_machine(const FsmStateDev *first, bool fresh) {
    (void)fresh;
    scan_used = false;
    scan_pending = false;
    stats.fsm_path = 0;
    stats.scan_entry_form = 0;
    stats.fsm_fallback_reason = 0;
    if (!have_fsm || run_n_out == 0) {
        HIPCHK(hipEventRecord(ev[2], stream));
        return OOKD_OK;
    }
    bool try_scan = scan_ok;
    if (first && (first->cur >= scan_tab.h.S || first->nbits > scan_tab.h.max_bits + 1)) try_scan = false;
    if (try_scan) {
        // queued without a host sync; fetch_results() looks at the scan's verdict
        // and, if it refused the capture, runs the round path instead
        pending_first_valid = first != nullptr;
        if (first) pending_first = *first;
        int rc = fsm_scan(first);
        if (rc != OOKD_OK) return rc;
        scan_pending = true;
        return OOKD_OK;
    }
    int rc = fsm_to_fixpoint(first, true, false);
    if (rc != OOKD_OK) return rc;
    stats.fsm_path = 2;
    return OOKD_OK;
}

// The scan's arguments that follow from the context (and, through fsm_params / publish_params, the run's
// geometry): fsm_scan and run_pipelined add what is their run's or chunk's own.
FsmScanArgs ookd_rx::scan_args() const {
    FsmScanArgs a{};
    a.f = fsm_params();
    scan_tab.fill(a);
    a.grid_blocks = 1024;
    a.block_tab = d_block_tab.p;
    a.publish = publish_params();
    a.cap_group_off = d_cap_group_off.p;
    a.group_tab = d_group_tab.p;
    a.cap_super_off = d_cap_super_off.p;
    a.super_tab = d_super_tab.p;
    a.super_in = d_super_in.p;
    a.cap_end = d_cap_end.p;
    a.cap_first = d_cap_end.p + (max_captures + 8);
    a.cap_block_off = d_cap_block_off.p;
    a.total_blocks_cap = scan_blocks_cap;
    a.events = d_events.p;
    a.ev_hot = d_ev_hot.p;
    a.app_vals = d_app_vals.p;
    a.app_capacity = d_app_vals.n - 64;     // fin_msg reads whole 8-byte groups
    a.errs = d_scan_errs.p;
    a.err_capacity = d_scan_errs.n;
    a.final_state = d_final_state.p;
    a.fallback = &d_hdr.p->scan_fallback;
    a.edge_overflow = &d_hdr.p->edge_overflow;
    a.pre_codes = d_pre.p;
    a.blk_in = d_blk_in.p;
    a.rowz = d_rowz.p;
    a.skipc = d_skipc.p;
    a.sync_rec = d_sync_rec.p;
    a.pre_plane = pre_plane;
    a.sync_fail = &d_hdr.p->sync_fail;
    a.fin_off = d_fin_off.p;
    a.fsum = d_fsum.p;
    a.fin_blocks_cap = scan_fin_cap;
    a.sync_try = sync_mode;
    return a;
}

int ookd_rx::fsm_scan(const FsmStateDev *first) {
    next_sync_mode();
    FsmScanArgs a = scan_args();
    a.first = first;
    if (run_caps > 1) {
        HIPCHK(hipMemsetAsync(d_cap_fallback.p, 0, run_caps * sizeof(uint32_t), stream));
        a.cap_fallback = d_cap_fallback.p;
    }
    a.fin_ticket = d_fin_tickets.p + kMaxChunks;
    a.run_stamp = next_scan_stamp();
    // totals / scan_fallback are still zero from the header memset of front_and_edges
    HIPCHK(launch_fsm_scan(a, stream, ev[2]));      // ev[2]: end of its last kernel
    scan_published = true;          // its last kernel also publishes
    return dump_scan_debug();
}

// OOKD_DEBUG_SCAN: waits for the scan just queued and prints what its kernels left in d_debug
int ookd_rx::dump_scan_debug() {
    static const char *const debug_scan = getenv("OOKD_DEBUG_SCAN");     // read once: this is the hot path
    if (!debug_scan) return OOKD_OK;
    HIPCHK(hipStreamSynchronize(stream));
    if (d_debug.p) {
        uint64_t dbg[64];
        HIPCHK(hipMemcpy(dbg, d_debug.p, sizeof(dbg), hipMemcpyDeviceToHost));
        fprintf(stderr, "[scan] block_sims phases: resume %llu gap+rep %llu uniq %llu sims %llu\n",
                (unsigned long long)(dbg[41] - dbg[40]), (unsigned long long)(dbg[42] - dbg[41]),
                (unsigned long long)(dbg[43] - dbg[42]), (unsigned long long)(dbg[44] - dbg[43]));
        {
            const uint64_t *c = dbg + 48;       // the leaf kernel's stamps (block 2)
            fprintf(stderr, "[scan] leaf (wave form) block 2: rows %llu stuck marks %llu compose %llu stuck starts %llu block table %llu ticks\n",
                    (unsigned long long)(c[1] - c[0]), (unsigned long long)(c[2] - c[1]), (unsigned long long)(c[3] - c[2]),
                    (unsigned long long)(c[4] - c[3]), (unsigned long long)(c[5] - c[4]));
        }
        uint64_t dbg2[8];
        HIPCHK(hipMemcpy(dbg2, d_debug.p + 56, sizeof(dbg2), hipMemcpyDeviceToHost));
        HIPCHK(hipMemset(d_debug.p + 56, 0, sizeof(dbg2)));
        fprintf(stderr, "[scan] sync walk: %llu arrivals outside the image; first: block %u cand %u code %u len %u, image %08x %08x, info %08x next %08x, "
                        "next block %u f0 %u, own cands %08x %08x; nothing to hold on to at block %u (%u)\n",
                (unsigned long long)dbg2[0], (uint32_t)dbg2[1], (uint32_t)(dbg2[1] >> 32), (uint32_t)dbg2[2], (uint32_t)(dbg2[2] >> 32),
                (uint32_t)dbg2[3], (uint32_t)(dbg2[3] >> 32), (uint32_t)dbg2[4], (uint32_t)(dbg2[4] >> 32), (uint32_t)dbg2[5],
                (uint32_t)(dbg2[5] >> 32), (uint32_t)dbg2[6], (uint32_t)(dbg2[6] >> 32), (uint32_t)dbg2[7], (uint32_t)(dbg2[7] >> 32));
        for (int i = 0; i < 4; ++i)
            fprintf(stderr, "[scan] leaf block %d: sims %llu expand %llu compose %llu ticks, %llu unique spans, cap %llx\n", i,
                    (unsigned long long)dbg[4 * i], (unsigned long long)dbg[4 * i + 1],
                    (unsigned long long)dbg[4 * i + 2], (unsigned long long)(dbg[4 * i + 3] & 0xffffffffu),
                    (unsigned long long)(dbg[4 * i + 3] >> 32));
    }
    if (debug_scan[0] == '2') {
        uint32_t off[2];
        HIPCHK(hipMemcpy(off, d_cap_block_off.p, 8, hipMemcpyDeviceToHost));
        uint32_t ne32[2];
        HIPCHK(hipMemcpy(&ne32[0], d_blk_offset.p, 4, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(&ne32[1], d_blk_offset.p + run_blocks, 4, hipMemcpyDeviceToHost));
        const uint32_t ne = ne32[1] - ne32[0];
        fprintf(stderr, "[scan] blocks %u..%u ne %u D %u LB %u\n", off[0], off[1], ne, scan_tab.h.D, scan_tab.h.leaf_block);
        std::vector<LeafEvDev> evs(ne + 1);
        HIPCHK(hipMemcpy(evs.data(), d_events.p, (ne + 1) * sizeof(LeafEvDev), hipMemcpyDeviceToHost));
        for (uint32_t i = 0; i <= ne && i < 14; ++i)
            fprintf(stderr, "[scan] leaf %u napp %u nout %u nerr %u flags %u end cur %u k %u prev %u\n", i,
                    evs[i].napp, evs[i].nout, evs[i].nerr, evs[i].flags, evs[i].end_cur, evs[i].end_k, evs[i].end_prev);
    }
    return OOKD_OK;
}

int ookd_rx::fetch_results() {
    int rc = enqueue_publish();
    if (rc != OOKD_OK) return rc;
    return collect_results();
}

PublishParams ookd_rx::publish_params() const {
    static_assert(sizeof(ResultHeader) % 4 == 0 && sizeof(ResultHeader) / 4 <= 256, "header is published by one workgroup");
    PublishParams pp{};
    pp.d_hdr = reinterpret_cast<uint32_t *>(d_hdr.p);
    pp.h_hdr = reinterpret_cast<uint32_t *>(h_hdr_dev);
    pp.hdr_words = sizeof(ResultHeader) / 4;
    pp.totals_word = offsetof(ResultHeader, totals) / 4;
    pp.edges_word = offsetof(ResultHeader, total_edges) / 4;
    pp.done_word = offsetof(ResultHeader, publish_done) / 4;
    pp.total_edges = run_n_out > 0 ? d_blk_offset.p + (size_t)run_caps * run_blocks : nullptr;
    if (have_fsm && run_n_out > 0) {
        pp.d_msgs = reinterpret_cast<const uint4 *>(d_msgs.p);
        pp.h_msgs = reinterpret_cast<uint4 *>(h_msgs_dev);
    }
    pp.first_msgs = std::min<uint64_t>(kHostMsgFirst, msg_capacity);
    return pp;
}

// Last kernel of a run: header and first messages into pinned host memory (the
// scan form's last kernel has already done it).
int ookd_rx::enqueue_publish() {
    if (scan_published) {
        scan_published = false;
        return OOKD_OK;
    }
    HIPCHK(launch_publish(publish_params(), stream));
    return OOKD_OK;
}

// The publish kernel zeroed the device header: put the front end's counters back, minus the scan's
// verdict and totals, for a second pass of the state machine over the same edges.  (publish_done:
// the scan's last kernel counts its workgroups there to find the one that publishes.)
int ookd_rx::rearm_header(const ResultHeader &seen) {
    ResultHeader keep = seen;
    keep.totals[0] = keep.totals[1] = 0;
    keep.scan_fallback = 0;
    keep.sync_fail = 0;
    keep.publish_done = 0;
    HIPCHK(hipMemcpyAsync(d_hdr.p, &keep, sizeof(keep), hipMemcpyHostToDevice, stream));
    HIPCHK(hipStreamSynchronize(stream));
    hdr_dirty = true;
    return OOKD_OK;
}

// Waits for the run queued on the stream and turns it into host-side results.
int ookd_rx::collect_results() {
    const uint64_t first = std::min<uint64_t>(kHostMsgFirst, msg_capacity);
    uint32_t total_edges = 0;
    bool redo_some = false;             // the scan left some captures of the batch to the rounds
    mixed_valid = false;
    HIPCHK(hipStreamSynchronize(stream));
    hdr_dirty = false;              // the publish kernel left the device header zeroed
    if (scan_pending) {
        scan_pending = false;
        if (h_hdr->scan_fallback == 0) {
            scan_used = true;
            stats.fsm_path = 1;
            stats.scan_entry_form = (h_hdr->sync_fail & 3u) == 2u ? 1u : 2u;
            if (sync_mode == 1 && (h_hdr->sync_fail & 1u)) sync_backoff = kSyncBackoff;     // tried with both queued: not yet
            redo_some = run_caps > 1 && (h_hdr->flags & 2u) != 0;
        } else if (h_hdr->scan_fallback == kScanFbSync && !h_hdr->edge_overflow && chunks.empty()) {
            // the walk from synchronising spans gave up and nothing was queued behind it: the scan again, composing
            // (and so for the next runs of this context)
            sync_backoff = kSyncBackoff;
            int rc = rearm_header(*h_hdr);
            if (rc != OOKD_OK) return rc;
            rc = run_state_machine(pending_first_valid ? &pending_first : nullptr, true);
            if (rc != OOKD_OK) return rc;
            rc = fetch_results();
            // (the second pass zeroed it: say why this run composed, as a pipelined run that was redone whole does)
            if (rc == OOKD_OK && stats.fsm_fallback_reason == 0) stats.fsm_fallback_reason = kScanFbSync;
            return rc;
        } else if (h_hdr->edge_overflow) {
            // refused because the edge list overflowed: there is nothing to run the rounds on (blk_offset counts
            // edges that were never written); reported below
            stats.fsm_fallback_reason = h_hdr->scan_fallback;
        } else if (!chunks.empty()) {
            if (h_hdr->scan_fallback & kScanFbSync) sync_backoff = kSyncBackoff;
            // the scan refused a chunk of a pipelined run: the whole capture again, unchunked (the
            // last chunk's publishing kernel left the device header zeroed)
            stats.fsm_fallback_reason = h_hdr->scan_fallback;
            if (getenv("OOKD_DEBUG")) {
                fprintf(stderr, "[ookd] pipelined run refused (reason %u), running the capture whole\n", h_hdr->scan_fallback);
            }
            chunks.clear();
            no_pipeline_once = true;
            const uint32_t reason = stats.fsm_fallback_reason;
            int rc = front_and_edges(last_iq, last_stride, nullptr, 0);
            if (rc == OOKD_OK) rc = run_state_machine(nullptr, true);
            if (rc == OOKD_OK) rc = enqueue_publish();
            no_pipeline_once = false;
            if (rc != OOKD_OK) return rc;
            rc = collect_results();
            if (stats.fsm_fallback_reason == 0) stats.fsm_fallback_reason = reason;
            return rc;
        } else {
            // the scan refused this capture: run the round path and fetch again
            stats.fsm_fallback_reason = h_hdr->scan_fallback;
            if (getenv("OOKD_DEBUG")) {
                fprintf(stderr, "[ookd] fsm scan refused (reason %u), using rounds\n", h_hdr->scan_fallback);
            }
            int rc = rearm_header(*h_hdr);
            if (rc != OOKD_OK) return rc;
            rc = fsm_to_fixpoint(pending_first_valid ? &pending_first : nullptr, true, false);
            if (rc != OOKD_OK) return rc;
            stats.fsm_path = 3;
            return fetch_results();
        }
    }
    total_edges = run_n_out > 0 ? h_hdr->total_edges : 0;
    run_overflow = h_hdr->edge_overflow != 0;
    run_edges_valid = true;
    num_msgs = 0;
    stats.num_edges = total_edges;
    stats.num_messages = 0;
    stats.num_errors = 0;
    stats.guard_recomputes = h_hdr->recompute;
    stats.front_form = front.plan.form;
    stats.total_waves = front_wave_tiles(front_params(nullptr, 0)) * run_caps;
    if (stats.total_waves) {
        if (count_quiet) {
            // running counters (never zeroed: a memset per run is a 20 us fill kernel on the critical path):
            // this run's share is the difference to what the run before left, modulo 2^32 per counter
            std::vector<uint32_t> q(kQuietCounters);
            HIPCHK(hipMemcpyAsync(q.data(), d_quiet.p, q.size() * 4, hipMemcpyDeviceToHost, stream));
            HIPCHK(hipStreamSynchronize(stream));
            if (quiet_prev.size() != q.size()) quiet_prev.assign(q.size(), 0u);
            for (size_t i = 0; i < q.size(); ++i) {
                stats.quiet_waves += (uint32_t)(q[i] - quiet_prev[i]);
                quiet_prev[i] = q[i];
            }
        }
    }
    stats.input_samples = run_n_in;
    stats.decimated_samples = run_n_out;
    stats.num_segments = run_caps * run_segs_per_cap;
    float ms = 0.0f;
    if (!chunks.empty()) {
        // pipelined: the front-end kernels of all chunks; first kernel start -> last kernel end
        stats.pipeline_chunks = (uint32_t)chunks.size();
        stats.front_launches = (uint32_t)chunks.size();
        float sum = 0.0f;
        for (size_t c = 0; c < chunks.size(); ++c) {
            if (hipEventElapsedTime(&ms, ev_c0[c], ev_c1[c]) == hipSuccess) sum += ms;
        }
        stats.fir_kernel_ms = sum;
        if (hipEventElapsedTime(&ms, ev_c0[0], ev[2]) == hipSuccess) stats.total_device_ms = ms;
    } else {
        stats.front_launches = front_launches;
        if (hipEventElapsedTime(&ms, ev[0], ev[1]) == hipSuccess) stats.fir_kernel_ms = ms;
        if (hipEventElapsedTime(&ms, ev[0], ev[2]) == hipSuccess) stats.total_device_ms = ms;
    }
    if (h_hdr->edge_overflow) {
        set_error("edge list overflow: %u level changes found, capacity %llu "
                  "(raise ookd_rx_config.edge_capacity)",
                  total_edges, (unsigned long long)edge_capacity);
        return OOKD_ERR_CAPACITY;
    }
    if (have_fsm && run_n_out > 0) {
        if (!scan_used && (h_hdr->flags & 1u)) {
            set_error("a state machine segment produced more than %u messages "
                      "(raise ookd_rx_config.message_slots)", msg_slots);
            return OOKD_ERR_CAPACITY;
        }
        const uint64_t total = h_hdr->totals[0];
        if (total > msg_capacity) {
            set_error("message list overflow: %llu messages, capacity %llu",
                      (unsigned long long)total, (unsigned long long)msg_capacity);
            return OOKD_ERR_CAPACITY;
        }
        if (total > first) {
            // (on the context's stream, not the null stream: that one joins every blocking stream of the process)
            HIPCHK(hipMemcpyAsync(h_msgs + first, d_msgs.p + first, (total - first) * sizeof(MsgDev),
                                  hipMemcpyDeviceToHost, stream));
            HIPCHK(hipStreamSynchronize(stream));
        }
        num_msgs = total;
        stats.num_messages = total;
        stats.num_errors = h_hdr->totals[1];
        // every reported error has its position, or the run fails: ookd_rx_get_errors never hands out a list with holes
        if (scan_used && stats.num_errors > d_scan_errs.n) {
            set_error("error list overflow: %llu errors, the list holds %llu (one per buffer of max_samples, at most %llu: "
                      "raise ookd_rx_config.samples_per_buffer)", (unsigned long long)stats.num_errors,
                      (unsigned long long)d_scan_errs.n, (unsigned long long)kErrListMax);
            return OOKD_ERR_CAPACITY;
        }
        if (!scan_used && (h_hdr->flags & 4u)) return segment_errors_overflow();
        if (redo_some) {
            const int rc = redo_refused_captures();
            if (rc != OOKD_OK) return rc;
        }
        // (the scan's finish kernel numbers message slots capture-major, the round
        //  form's gather does too: the list is already in capture order)
    }
    return OOKD_OK;
}

// ---------------------------------------------------------------------------
// context creation: one step per function, each false on failure (error text set)
// ---------------------------------------------------------------------------
namespace {

// The state machine's tables on the device
bool setup_device_tables(ookd_rx &rx, const ookd_device &device) {
    const size_t ns = device.state_duration_us.size();
    const size_t nt = device.trig_cond.size();
    const bool big = ns > (size_t)kMaxStates || nt > (size_t)kMaxTriggers;
    if (ns > (size_t)kMaxStatesBig || nt > (size_t)kMaxTriggersBig || device.num_bits > 254) {
        set_error("device has %zu states / %zu triggers / %u bits, this build supports %d / %d / 254", ns, nt,
                  device.num_bits, kMaxStatesBig, kMaxTriggersBig);
        return false;
    }
    // the kernel counts elapsed samples in 32 bits (saturating)
    auto too_long = [](const std::vector<uint64_t> &v) {
        for (uint64_t x : v) {
            if (x != ~0ull && x >= (1ull << 31)) return true;
        }
        return false;
    };
    if (too_long(device.state_kmin) || too_long(device.state_kmax) || too_long(device.state_kto) ||
        too_long(device.trig_kmin) || too_long(device.trig_kmax)) {
        set_error("a device duration/timeout exceeds 2^31 samples at this rate: unsupported");
        return false;
    }
    std::unique_ptr<FsmTablesDev> t(new FsmTablesDev());
    memset(t.get(), 0, sizeof(FsmTablesDev));
    fill_fsm_tables(device, *t);
    if (rx.d_tables.alloc(1) != OOKD_OK) return false;
    if (hipMemcpy(rx.d_tables.p, t.get(), sizeof(FsmTablesDev), hipMemcpyHostToDevice) != hipSuccess) {
        set_error("table upload failed");
        return false;
    }
    if (big) {
        // more than 64 states / triggers: the round form with the tables in LDS (the scan's tables and the
        // lane-resident ones stop at 64)
        const std::vector<uint32_t> w = big_tables(device, t->quiet_state);
        if (rx.d_big.alloc(w.size()) != OOKD_OK) return false;
        if (hipMemcpy(rx.d_big.p, w.data(), w.size() * sizeof(uint32_t), hipMemcpyHostToDevice) != hipSuccess) {
            set_error("table upload failed");
            return false;
        }
        rx.big_device = true;
    }
    rx.have_fsm = true;
    rx.num_bits = device.num_bits;
    rx.h_tables = std::move(t);
    return true;
}

// Capacities, and the buffers of the front end, the edges and the round form of the state machine
bool setup_run_buffers(ookd_rx &rx, const ookd_rx_config &cfg) {
    const uint64_t spb = cfg.samples_per_buffer;
    // nominal decimated samples per state machine segment (~2^19 by default;
    // segment_buffers expresses it in input buffers)
    if (cfg.segment_buffers) {
        rx.seg_len = std::max<uint64_t>(1, (uint64_t)cfg.segment_buffers * spb / rx.total_decim());
    } else {
        rx.seg_len = 1ull << 19;
    }
    rx.seg_len = std::min<uint64_t>(rx.seg_len, 1ull << 30);   // 32-bit offsets inside a segment
    rx.msg_slots = cfg.message_slots ? cfg.message_slots : 32;
    uint32_t blocks = 0, segs = 0;
    rx.geometry(rx.max_samples, true, rx.max_n_in, rx.max_n_out, rx.max_words, blocks, segs);
    rx.max_blocks = blocks;
    rx.max_segs_per_cap = std::max<uint32_t>(segs, 1);
    {
        // Error positions of a segment of the round form.  The reference reports at most one error per buffer (the
        // rest of it is dropped, device.c:646), and fsm_cuts_kernel moves each end of a segment by up to seg_len / 2:
        // a segment spans at most 2 seg_len decimated samples, or the capture.  Every position fits, unless a tiny
        // samples_per_buffer on a huge context runs into kErrListMax -- then a run with more errors than slots fails
        // with OOKD_ERR_CAPACITY (collect_results), it never hands out a list with holes.
        const uint64_t span_in = std::min<uint64_t>(2 * rx.seg_len * rx.total_decim(), rx.max_n_in);
        const uint64_t need = (span_in + spb - 1) / spb + 2;
        const uint64_t room = std::max<uint64_t>(32, kErrListMax / ((uint64_t)rx.max_captures * rx.max_segs_per_cap));
        rx.err_slots = (uint32_t)std::min<uint64_t>(need, room);
    }
    const uint64_t total_out = rx.max_n_out * rx.max_captures;
    rx.edge_capacity = cfg.edge_capacity ? cfg.edge_capacity : total_out / 32 + (1u << 20);
    if (rx.edge_capacity > 0xfffffff0ull) rx.edge_capacity = 0xfffffff0ull;
    rx.msg_capacity = cfg.message_capacity ? cfg.message_capacity
                                           : std::max<uint64_t>(1u << 16, (uint64_t)rx.max_captures * 64);

    const size_t caps = rx.max_captures;
    const size_t nseg = caps * rx.max_segs_per_cap;
    int rc = OOKD_OK;
    rc |= rx.d_bits.alloc(caps * rx.max_words + 64);
    if (cfg.flags & OOKD_RX_KEEP_FIR) rc |= rx.d_fir.alloc(2 * caps * rx.max_n_out + 2);
    rc |= rx.d_halo.alloc(2 * (rx.halo_needed() + 4));
    rc |= rx.d_blk_count.alloc(caps * blocks + 1);
    rc |= rx.d_tile_info.alloc(caps * blocks * 16 + 16);       // smallest wave tile: 256 bits
    if (const char *w = dev_getenv("OOKD_FRONT_LAUNCH_LOG2")) rx.front_launch_outputs = 1ull << std::min(40, std::max(16, atoi(w)));
    rc |= rx.d_blk_offset.alloc(caps * blocks + 1 + kMaxChunks);     // (a pipelined run keeps one total per chunk)
    rc |= rx.d_group_total.alloc((caps * blocks + kScanGroup - 1) / kScanGroup + 1);
    rc |= rx.d_edges.alloc(rx.edge_capacity + 64);
    rc |= rx.d_hdr.alloc(1);
    rx.count_quiet = (cfg.flags & OOKD_RX_COUNT_QUIET) != 0;
    if (rx.count_quiet) rc |= rx.d_quiet.alloc(kQuietCounters);
    if (rx.count_quiet && rc == OOKD_OK && hipMemset(rx.d_quiet.p, 0, kQuietCounters * sizeof(uint32_t)) != hipSuccess) rc = OOKD_ERR_HIP;
    if (rx.have_fsm) {
        rc |= rx.d_seg_bounds.alloc(caps * (rx.max_segs_per_cap + 1));
        rc |= rx.d_state_in.alloc(nseg);
        rc |= rx.d_state_out.alloc(2 * nseg);
        rc |= rx.d_seg_msgs.alloc(nseg * rx.msg_slots);
        rc |= rx.d_msgs.alloc(rx.msg_capacity);
        rc |= rx.d_seg_msg_count.alloc(nseg);
        rc |= rx.d_seg_err_count.alloc(nseg);
        rc |= rx.d_seg_errs.alloc(nseg * rx.err_slots);
        if (getenv("OOKD_DEBUG")) rc |= rx.d_debug.alloc(nseg * 4 + 128);
    }
    return rc == OOKD_OK;
}

// The scan's run buffers, sized by the domain and the leaf block its tables gave
int setup_scan_workspace(ookd_rx &rx) {
    const size_t caps = rx.max_captures;
    const uint32_t D = rx.scan_tab.h.D, leaf_block = rx.scan_tab.h.leaf_block;
    int rc = OOKD_OK;
    rx.scan_blocks_cap = (uint32_t)(rx.edge_capacity / leaf_block + caps + 8);
    rc |= rx.d_block_tab.alloc((size_t)rx.scan_blocks_cap * ((D + 7u) & ~7u) + 64);
    {
        const size_t ngroups = rx.scan_blocks_cap / 16 + caps + 8;
        rc |= rx.d_cap_group_off.alloc(caps + 1);
        rc |= rx.d_group_tab.alloc(ngroups * ((D + 7u) & ~7u) + 64);
        const size_t nsuper = rx.scan_blocks_cap / 64 + caps + 8;
        rc |= rx.d_cap_super_off.alloc(caps + 1);
        rc |= rx.d_super_tab.alloc(nsuper * ((D + 7u) & ~7u) + 64);
        rc |= rx.d_super_in.alloc(nsuper);
        rc |= rx.d_cap_end.alloc(2 * (caps + 8));         // + cap_first
    }
    rc |= rx.d_cap_block_off.alloc(caps + 1);
    rc |= rx.d_events.alloc(rx.edge_capacity + caps + 8);
    rc |= rx.d_ev_hot.alloc(rx.edge_capacity + caps + 8);
    rc |= rx.d_app_vals.alloc(2 * (rx.edge_capacity + caps) + 512 * caps + 1024);
    {
        // error positions of a run: at most one per buffer and capture (device.c:646), and never more than there are
        // level changes (an error is a pulse_start / pulse_end trigger that fails its state's duration: it takes a
        // change of level, fed or inside a dropped rest-of-buffer) -- every position fits; beyond kErrListMax a run
        // with more errors fails with OOKD_ERR_CAPACITY (collect_results)
        const uint64_t spb = rx.cfg.samples_per_buffer;
        const uint64_t per_cap = (rx.max_n_in + spb - 1) / spb + 1;
        const uint64_t need = std::min<uint64_t>(caps * per_cap, rx.edge_capacity + caps);
        rc |= rx.d_scan_errs.alloc(std::max<uint64_t>(64, std::min<uint64_t>(need, kErrListMax)));
    }
    rc |= rx.d_cap_fallback.alloc(caps);
    // (the walk from synchronising spans keeps a plane of entry codes per candidate)
    rx.pre_plane = rx.scan_sync ? (size_t)rx.scan_blocks_cap * leaf_block + 64 : 0;
    rc |= rx.d_pre.alloc(((size_t)rx.scan_blocks_cap * leaf_block + 64) * (rx.scan_sync ? 4 : 1));
    rc |= rx.d_rowz.alloc((size_t)rx.scan_blocks_cap * leaf_block + 64);
    rc |= rx.d_skipc.alloc((size_t)rx.scan_blocks_cap * leaf_block + 64);
    rc |= rx.d_sync_rec.alloc(((size_t)rx.scan_blocks_cap + 8) * 10);     // records, digests, selections
    rc |= rx.d_blk_in.alloc((size_t)rx.scan_blocks_cap + 16);
    rc |= rx.d_final_state.alloc(caps);
    // (fin_msg_kernel resolves every capture's record: one that no run has written yet must read as "no bits")
    if (rc == OOKD_OK && hipMemset(rx.d_final_state.p, 0, caps * sizeof(SegState)) != hipSuccess) rc = OOKD_ERR_HIP;
    rx.scan_fin_cap = (uint32_t)((rx.edge_capacity + caps) / fsm_scan_fin_block() + caps + 8);
    rc |= rx.d_fin_off.alloc(caps + 1);
    rc |= rx.d_fsum.alloc(4 * (size_t)rx.scan_fin_cap);
    // stamped work counters (fsm_scan.hip: take_stamped_ticket): zeroed ONCE -- stamp 0 is no run's
    rc |= rx.d_fin_tickets.alloc(kMaxChunks + 1);
    if (rc == OOKD_OK && hipMemset(rx.d_fin_tickets.p, 0, (kMaxChunks + 1) * sizeof(unsigned long long)) != hipSuccess) rc = OOKD_ERR_HIP;
    // stamped aggregates: the stamp half of every word must start out as "no run"
    if (rc == OOKD_OK && hipMemset(rx.d_fsum.p, 0, rx.d_fsum.n * sizeof(uint64_t)) != hipSuccess) rc = OOKD_ERR_HIP;
    return rc;
}

// The scan form of the state machine (fsm_scan.hip): its tables and buffers
bool setup_scan(ookd_rx &rx, const ookd_device &device, const ookd_rx_config &cfg) {
    // abstract states = states x bit counts + skip x2 + poison
    const uint32_t d0 = (uint32_t)device.state_duration_us.size() * (device.num_bits + 2) + 3;
    rx.scan_ok = !(cfg.flags & OOKD_RX_FSM_ROUNDS) && d0 <= 384 && device.num_bits <= 254 && !rx.big_device;
    if (!rx.scan_ok) return true;
    const bool with_spans = !(cfg.flags & OOKD_RX_SCAN_SIMS);
    const auto t0 = std::chrono::steady_clock::now();
    ScanTables t = build_scan_tables(*rx.h_tables, cfg.samples_per_buffer, rx.total_decim(), with_spans);
    if (with_spans && getenv("OOKD_DEBUG")) {
        size_t zeros = 0;
        for (uint32_t v : t.pk) zeros += v == 0;
        fprintf(stderr, "[ookd] span tables: %s, %zu intervals (%zu need simulation), %zu codes can get stuck, "
                        "%zu codes reachable, %.1f ms\n",
                t.spans_built ? "built" : "REFUSED", t.n0.size(), zeros, t.stuck_src.size(), t.reach.size(),
                std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
        if (getenv("OOKD_DEBUG")[0] == '2') {
            for (size_t r = 0; r + 1 < t.off.size(); ++r) {
                fprintf(stderr, "[ookd]  row %zu L %zu:", r / 2, r % 2);
                for (uint32_t i = t.off[r]; i < t.off[r + 1]; ++i) fprintf(stderr, " %u:%08x", t.n0[i], t.pk[i]);
                fprintf(stderr, "\n");
            }
        }
    }
    int rc = rx.scan_tab.upload(std::move(t));
    if (rx.scan_tab.d_lt_merged.n) {
        rx.scan_sync = !(cfg.flags & OOKD_RX_SCAN_TABLES) && !dev_getenv("OOKD_SCAN_NO_SYNC");
        if (const char *e = dev_getenv("OOKD_SYNC_MIN_EDGES")) rx.sync_min_edges = strtoull(e, nullptr, 0);
    }
    rc |= setup_scan_workspace(rx);
    return rc == OOKD_OK;
}

// Sparse front-end output and the pinned result buffers
bool setup_results(ookd_rx &rx) {
    // sparse front-end output (1-stage kernels with the quiet shortcut, no float dump): the bit
    // words and tile infos start out zero and every run zeroes what the run before wrote
    rx.sparse = rx.front.plan.sparse_capable && !dev_getenv("OOKD_DENSE_BITS");
    if (rx.sparse &&
        (hipMemset(rx.d_bits.p, 0, rx.d_bits.n * sizeof(uint64_t)) != hipSuccess ||
         hipMemset(rx.d_tile_info.p, 0, rx.d_tile_info.n * sizeof(uint32_t)) != hipSuccess)) {
        set_error("hipMemset of the bit words failed");
        return false;
    }
    if (hipHostMalloc(reinterpret_cast<void **>(&rx.h_hdr), sizeof(ResultHeader)) != hipSuccess ||
        hipHostMalloc(reinterpret_cast<void **>(&rx.h_msgs), rx.msg_capacity * sizeof(MsgDev)) != hipSuccess) {
        set_error("hipHostMalloc failed");
        return false;
    }
    memset(rx.h_hdr, 0, sizeof(ResultHeader));
    if (hipHostGetDevicePointer(reinterpret_cast<void **>(&rx.h_hdr_dev), rx.h_hdr, 0) != hipSuccess ||
        hipHostGetDevicePointer(reinterpret_cast<void **>(&rx.h_msgs_dev), rx.h_msgs, 0) != hipSuccess) {
        set_error("pinned result buffers are not mapped into the device");
        return false;
    }
    return true;
}

// The chunk pipeline: two internal streams, each on its own half of the CUs
bool setup_pipeline(ookd_rx &rx, const ookd_rx_config &cfg) {
    // off unless asked for (pipeline_chunk_samples, or OOKD_PIPELINE=1 for the default chunk): with the
    // hardware-dispatched front end the chain's kernels are hardly dispatched while a front-end grid
    // has workgroups pending, and the chunked run is slower than the whole one
    uint64_t want = cfg.pipeline_chunk_samples;
    if (!want && dev_getenv("OOKD_PIPELINE")) want = kPipeDefaultChunk;
    rx.pipe_chunk_in = want ? want : kPipeDefaultChunk;
    rx.pipe_ok = want != 0 && !rx.num_carriers() && rx.have_fsm && rx.scan_ok && rx.tile_bits() != 0 && !(cfg.flags & OOKD_RX_NO_PIPELINE) &&
                 cfg.pipeline_chunk_samples != ~0ull && !dev_getenv("OOKD_NO_PIPELINE") &&
                 rx.max_n_out >= 2 * (rx.pipe_chunk_in / rx.total_decim());
    if (!rx.pipe_ok) return true;
    // every other CU of every XCD for the front end, the rest for the chain (an UNEVEN mask
    // slows the front end: the dispatcher deals workgroups evenly over the XCDs).
    // OOKD_PIPE_MASKS=front,chain (hex, per 32 CUs; 0 = no mask) overrides.
    uint32_t mf = 0x55555555u, mc = 0xAAAAAAAAu;
    if (const char *m = dev_getenv("OOKD_PIPE_MASKS")) {
        char *end = nullptr;
        mf = (uint32_t)strtoul(m, &end, 16);
        mc = (end && *end == ',') ? (uint32_t)strtoul(end + 1, nullptr, 16) : 0u;
    }
    auto make = [&](hipStream_t &s, uint32_t pattern) {
        if (pattern == 0) return hipStreamCreateWithFlags(&s, hipStreamNonBlocking);
        uint32_t mask[8];
        for (auto &w : mask) w = pattern;
        hipError_t e = hipExtStreamCreateWithCUMask(&s, 8, mask);
        if (e != hipSuccess) {          // (no CU masking on this system: plain streams still pipeline)
            (void)hipGetLastError();
            e = hipStreamCreateWithFlags(&s, hipStreamNonBlocking);
        }
        return e;
    };
    if (make(rx.s_front, mf) != hipSuccess || make(rx.s_chain, mc) != hipSuccess ||
        hipEventCreateWithFlags(&rx.ev_start, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&rx.ev_end, hipEventDisableTiming) != hipSuccess) {
        set_error("creating the pipeline streams failed");
        return false;
    }
    return rx.d_carry.alloc(2) == OOKD_OK && rx.d_chunk_totals.alloc(4) == OOKD_OK;
}

}  // namespace

// ---------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------
extern "C" {

ookd_rx *ookd_rx_create(const ookd_rx_config *cfg, const ookd_filter *filter,
                        const ookd_device *device) {
    return ookd_rx_create_tuned(cfg, filter, device, nullptr);
}

double ookd_rx_tune(const ookd_rx *rx) {
    // (a tuned context is one carrier record and no table)
    return rx && !rx->num_carriers() && !rx->front.plan.carriers.empty() ? rx->front.plan.carriers[0].nu : 0.0;
}

// the body of every create call: a context tuned to nu, or (num_carriers != 0) a carrier context
static ookd_rx *create_context(const ookd_rx_config *cfg, const ookd_filter *filter, const ookd_device *device,
                               double nu, const ookd_rx_carrier *carriers, uint32_t num_carriers) {
    if (!cfg || cfg->samples_per_buffer == 0 || cfg->max_samples == 0) {
        set_error("ookd_rx_create: samples_per_buffer and max_samples must be non-zero");
        return nullptr;
    }
    FrontPlan plan;
    if (!plan_front(cfg->flags, cfg->threshold, filter, nu, carriers, num_carriers, plan)) return nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
        set_error("no HIP device available: libookiedokie_amd has no CPU fallback");
        return nullptr;
    }
    if (cfg->hip_device < 0 || cfg->hip_device >= ndev) {
        set_error("hip_device %d out of range (%d devices)", cfg->hip_device, ndev);
        return nullptr;
    }
    std::unique_ptr<ookd_rx> rx(new ookd_rx());
    rx->cfg = *cfg;
    rx->dev = cfg->hip_device;
    if (hipSetDevice(rx->dev) != hipSuccess) {
        set_error("hipSetDevice(%d) failed", rx->dev);
        return nullptr;
    }
    if (cfg->stream) {
        rx->stream = static_cast<hipStream_t>(cfg->stream);
    } else {
        if (hipStreamCreateWithFlags(&rx->stream, hipStreamNonBlocking) != hipSuccess) {
            set_error("hipStreamCreate failed");
            return nullptr;
        }
        rx->own_stream = true;
    }
    for (auto &e : rx->ev) {
        if (hipEventCreate(&e) != hipSuccess) {
            set_error("hipEventCreate failed");
            return nullptr;
        }
    }
    // (a carrier context's results are those of a batch of num_carriers captures)
    rx->max_captures = num_carriers ? num_carriers : cfg->max_captures ? cfg->max_captures : 1;
    rx->max_samples = cfg->max_samples;

    if (rx->front.upload(std::move(plan)) != OOKD_OK) return nullptr;
    if (device && !setup_device_tables(*rx, *device)) return nullptr;
    if (!setup_run_buffers(*rx, *cfg)) return nullptr;
    if (rx->have_fsm && !setup_scan(*rx, *device, *cfg)) return nullptr;
    if (!setup_results(*rx) || !setup_pipeline(*rx, *cfg)) return nullptr;
    rx->gate = static_cast<ookd_rx_gate *>(cfg->front_gate);
    // (tests: start the tile stamp near its wrap-around)
    if (const char *e = dev_getenv("OOKD_TILE_STAMP_START")) rx->tile_stamp = std::min<uint32_t>((uint32_t)strtoul(e, nullptr, 0), kTileStampMax);
    return rx.release();
}

ookd_rx *ookd_rx_create_tuned(const ookd_rx_config *cfg, const ookd_filter *filter,
                              const ookd_device *device, const ookd_tune *tune) {
    clear_error();
    return create_context(cfg, filter, device, tune ? tune->nu : 0.0, nullptr, 0);
}

ookd_rx *ookd_rx_create_carriers(const ookd_rx_config *cfg, const ookd_filter *filter, const ookd_device *device,
                                 const ookd_rx_carrier *carriers, uint32_t num_carriers) {
    clear_error();
    if (!carriers || num_carriers == 0 || num_carriers > OOKD_RX_MAX_CARRIERS) {
        set_error("ookd_rx_create_carriers: 1 to %d carriers, got %u%s", OOKD_RX_MAX_CARRIERS, num_carriers,
                  carriers ? "" : " (carriers == NULL)");
        return nullptr;
    }
    static_assert(OOKD_RX_MAX_CARRIERS == kMaxCarriers, "the fused kernel's carrier mask");
    for (uint32_t k = 0; k < num_carriers; ++k) {
        if (!(std::fabs(carriers[k].nu) <= 0.5)) {
            set_error("ookd_rx_create_carriers: carrier %u: nu must be within [-0.5, 0.5] cycles per sample", k);
            return nullptr;
        }
        for (uint32_t r : carriers[k].reserved) {
            if (r) {
                set_error("ookd_rx_create_carriers: carrier %u: reserved words must be zero", k);
                return nullptr;
            }
        }
    }
    if (cfg && cfg->max_captures > 1) {
        set_error("ookd_rx_create_carriers: a carrier context runs one capture per run (max_captures = %u)", cfg->max_captures);
        return nullptr;
    }
    return create_context(cfg, filter, device, 0.0, carriers, num_carriers);
}

uint32_t ookd_rx_num_carriers(const ookd_rx *rx) { return rx ? rx->num_carriers() : 0u; }

int ookd_rx_get_carrier(const ookd_rx *rx, uint32_t k, ookd_rx_carrier *out) {
    clear_error();
    if (!rx || !out || k >= rx->num_carriers()) {
        set_error("ookd_rx_get_carrier: bad argument");
        return OOKD_ERR_ARG;
    }
    *out = ookd_rx_carrier{};
    out->nu = rx->front.plan.carriers[k].nu;
    out->threshold = rx->front.plan.carriers[k].threshold;
    return OOKD_OK;
}

void ookd_rx_destroy(ookd_rx *rx) { delete rx; }

uint32_t ookd_rx_sample_bytes(const ookd_rx *rx) { return rx ? sample_bytes(rx->front.base.sample_fmt) : 0u; }

ookd_rx_gate *ookd_rx_gate_create(void) { return new (std::nothrow) ookd_rx_gate(); }

void ookd_rx_gate_destroy(ookd_rx_gate *gate) { delete gate; }

int ookd_rx_submit_device(ookd_rx *rx, const void *d_iq, uint32_t num_captures,
                          uint64_t samples_per_capture, uint64_t capture_stride_samples) {
    clear_error();
    if (!rx || (!d_iq && samples_per_capture)) {
        set_error("ookd_rx_submit_device: null argument");
        return OOKD_ERR_ARG;
    }
    if (rx->submitted) {
        set_error("ookd_rx_submit_device: the previous run has not been waited for");
        return OOKD_ERR_ARG;
    }
    if (rx->num_carriers() && num_captures != 1) {
        set_error("a carrier context runs one capture per run (num_captures = %u)", num_captures);
        return OOKD_ERR_ARG;
    }
    if (num_captures == 0 || num_captures > rx->max_captures || samples_per_capture > rx->max_samples) {
        set_error("run of %u captures x %llu samples exceeds the context capacity (%u x %llu)",
                  num_captures, (unsigned long long)samples_per_capture, rx->max_captures,
                  (unsigned long long)rx->max_samples);
        return OOKD_ERR_ARG;
    }
    if (num_captures > 1 && capture_stride_samples < samples_per_capture) {
        set_error("capture stride smaller than the capture");
        return OOKD_ERR_ARG;
    }
    HIPCHK(hipSetDevice(rx->dev));
    // (behind the front end a carrier context's carriers are the captures of a batch)
    rx->run_caps = rx->num_carriers() ? rx->num_carriers() : num_captures;
    rx->run_n_valid = samples_per_capture;
    rx->geometry(samples_per_capture, true, rx->run_n_in, rx->run_n_out, rx->run_words,
                 rx->run_blocks, rx->run_segs_per_cap);
    rx->stats = ookd_rx_stats{};
    ++rx->run_serial;
    rx->run_shard = false;
    rx->run_overflow = rx->run_edges_valid = false;
    rx->last_iq = d_iq;
    rx->last_stride = capture_stride_samples;
    if (rx->plan_chunks()) {
        const int rcp = rx->run_pipelined(d_iq);
        if (rcp != OOKD_OK) return rcp;
        rx->submitted = true;
        return OOKD_OK;
    }
    int rc = rx->front_and_edges(d_iq, capture_stride_samples, nullptr, 0);
    if (rc != OOKD_OK) return rc;
    rc = rx->run_state_machine(nullptr, true);
    if (rc != OOKD_OK) return rc;
    rc = rx->enqueue_publish();
    if (rc != OOKD_OK) return rc;
    rx->submitted = true;
    return OOKD_OK;
}

int ookd_rx_wait(ookd_rx *rx) {
    clear_error();
    if (!rx || !rx->submitted) {
        set_error("ookd_rx_wait: nothing was submitted");
        return OOKD_ERR_ARG;
    }
    rx->submitted = false;
    HIPCHK(hipSetDevice(rx->dev));
    return rx->collect_results();
}

int ookd_rx_process_device(ookd_rx *rx, const void *d_iq, uint32_t num_captures,
                           uint64_t samples_per_capture, uint64_t capture_stride_samples) {
    static const bool timing = getenv("OOKD_DEBUG_TIME") != nullptr;
    using clk = std::chrono::steady_clock;
    const auto t0 = clk::now();
    int rc = ookd_rx_submit_device(rx, d_iq, num_captures, samples_per_capture, capture_stride_samples);
    if (rc != OOKD_OK) return rc;
    const auto t1 = clk::now();
    rc = ookd_rx_wait(rx);
    if (timing) {
        const auto t2 = clk::now();
        auto us = [](clk::time_point a, clk::time_point b) {
            return std::chrono::duration<double, std::micro>(b - a).count();
        };
        fprintf(stderr, "[ookd] host us: enqueue %.1f, wait + collect %.1f\n", us(t0, t1), us(t1, t2));
    }
    return rc;
}

int ookd_rx_process_host(ookd_rx *rx, const int16_t *iq, uint64_t num_samples) {
    clear_error();
    if (!rx || (!iq && num_samples)) {
        set_error("ookd_rx_process_host: null argument");
        return OOKD_ERR_ARG;
    }
    if (num_samples > rx->max_samples) {
        set_error("capture of %llu samples exceeds max_samples %llu", (unsigned long long)num_samples,
                  (unsigned long long)rx->max_samples);
        return OOKD_ERR_ARG;
    }
    HIPCHK(hipSetDevice(rx->dev));
    if (!rx->d_stage_in.p) {
        int rc = rx->d_stage_in.alloc(rx->max_samples * (sample_bytes(rx->front.base.sample_fmt) / 2) + 8);
        if (rc != OOKD_OK) return rc;
    }
    if (num_samples && rx->ingest.from_host(iq, rx->d_stage_in.p, num_samples * sample_bytes(rx->front.base.sample_fmt)) < 0) return OOKD_ERR_HIP;
    return ookd_rx_process_device(rx, rx->d_stage_in.p, 1, num_samples, num_samples);
}

uint64_t ookd_rx_halo_samples(const ookd_rx *rx) { return rx ? rx->halo_needed() : 0; }

int ookd_scan_domain_info(const ookd_device *device, uint32_t samples_per_buffer, uint32_t total_decimation,
                          uint32_t out[8]) {
    clear_error();
    if (!device || !out || !samples_per_buffer || !total_decimation) {
        set_error("ookd_scan_domain_info: bad argument");
        return OOKD_ERR_ARG;
    }
    std::unique_ptr<FsmTablesDev> g(new FsmTablesDev());
    memset(g.get(), 0, sizeof(FsmTablesDev));
    fill_fsm_tables(*device, *g);
    const ScanTables t = build_scan_tables(*g, samples_per_buffer, total_decimation, true);
    size_t zeros = 0;
    for (uint32_t v : t.pk) zeros += v == 0;
    out[0] = scan_tables_selfcheck(t) ? 1u : 0u;
    out[1] = (uint32_t)t.n0.size();
    out[2] = (uint32_t)zeros;
    out[3] = (uint32_t)t.reach.size();
    out[4] = (uint32_t)t.stuck_src.size();
    out[5] = (uint32_t)t.stuck_rows.size();
    out[6] = t.D;
    out[7] = t.S;
    return OOKD_OK;
}

// Test aid, not in the public header: 64-bit FNV-1a digests of  off | n0 | pk,  reach | reach_by_level,  merged
// (sync tables appended)  and the LTab image, to hold the host builders against recorded values without a GPU.
int ookd_scan_tables_digest(const ookd_device *device, uint32_t samples_per_buffer, uint32_t total_decimation,
                            uint64_t out[4]) {
    if (!device || !out || !samples_per_buffer || !total_decimation) return OOKD_ERR_ARG;
    std::unique_ptr<FsmTablesDev> g(new FsmTablesDev());
    memset(g.get(), 0, sizeof(FsmTablesDev));
    fill_fsm_tables(*device, *g);
    const ScanTables t = build_scan_tables(*g, samples_per_buffer, total_decimation, true);
    auto fnv = [](uint64_t h, const auto &v) { return fnv1a(h, v.data(), v.size() * sizeof(v[0])); };
    const uint64_t h0 = kFnvBasis;
    out[0] = fnv(fnv(fnv(h0, t.off), t.n0), t.pk);
    out[1] = fnv(fnv(h0, t.reach), t.reach_by_level);
    out[2] = fnv(h0, t.merged);
    out[3] = fnv(h0, t.ltab);
    return OOKD_OK;
}

int ookd_rx_shard_begin(ookd_rx *rx, const void *d_iq, uint64_t num_samples, const int16_t *halo,
                        uint64_t halo_samples, int last_shard, const ookd_fsm_state *state_in,
                        ookd_fsm_state *state_out) {
    clear_error();
    if (!rx || (!d_iq && num_samples) || num_samples > rx->max_samples) {
        set_error("ookd_rx_shard_begin: bad argument");
        return OOKD_ERR_ARG;
    }
    if (rx->num_carriers()) {
        set_error("ookd_rx_shard_begin: a carrier context runs whole captures, not shards");
        return OOKD_ERR_ARG;
    }
    if (rx->debounce()) {
        set_error("ookd_rx_shard_begin: the context has a debounce set (ookd_rx_set_debounce): the level in front of a "
                  "shard is not known to the clean pass");
        return OOKD_ERR_ARG;
    }
    const uint64_t spb = rx->cfg.samples_per_buffer;
    const uint64_t align = spb / gcd64(spb, rx->total_decim()) * rx->total_decim();
    if (!last_shard && (num_samples % align) != 0) {
        set_error("shard of %llu samples is not a multiple of lcm(samples_per_buffer, decimation) = %llu",
                  (unsigned long long)num_samples, (unsigned long long)align);
        return OOKD_ERR_ARG;
    }
    if (halo && halo_samples < rx->halo_needed()) {
        set_error("halo of %llu samples is shorter than the %llu the filter needs",
                  (unsigned long long)halo_samples, (unsigned long long)rx->halo_needed());
        return OOKD_ERR_ARG;
    }
    HIPCHK(hipSetDevice(rx->dev));
    uint32_t hl = 0;
    if (halo && rx->halo_needed()) {
        hl = (uint32_t)rx->halo_needed();
        // hipMemcpyDefault: the halo may be a host array or a device buffer an
        // RCCL recv landed in
        const size_t sb = sample_bytes(rx->front.base.sample_fmt);
        HIPCHK(hipMemcpyAsync(rx->d_halo.p, reinterpret_cast<const char *>(halo) + sb * (halo_samples - hl), (size_t)hl * sb,
                              hipMemcpyDefault, rx->stream));
    }
    rx->run_caps = 1;
    rx->run_n_valid = num_samples;
    rx->geometry(num_samples, last_shard != 0, rx->run_n_in, rx->run_n_out, rx->run_words,
                 rx->run_blocks, rx->run_segs_per_cap);
    rx->chunks.clear();
    rx->stats = ookd_rx_stats{};
    ++rx->run_serial;
    rx->run_shard = true;
    rx->run_overflow = rx->run_edges_valid = false;
    int rc = rx->front_and_edges(d_iq, num_samples, hl ? rx->d_halo.p : nullptr, hl);
    if (rc != OOKD_OK) return rc;
    static_assert(sizeof(ookd_fsm_state) == sizeof(FsmStateDev), "fsm state layout");
    rc = rx->run_state_machine(reinterpret_cast<const FsmStateDev *>(state_in), true);
    if (rc != OOKD_OK) return rc;
    rc = rx->fetch_results();
    if (rc != OOKD_OK) return rc;
    if (state_out && rx->have_fsm && rx->run_n_out > 0) {
        const size_t nseg = rx->run_segs_per_cap;
        const SegState *src = rx->scan_used ? rx->d_final_state.p
                                            : &rx->d_state_out.p[(size_t)rx->final_parity * nseg + (nseg - 1)];
        HIPCHK(hipMemcpy(state_out, &src->st, sizeof(FsmStateDev), hipMemcpyDeviceToHost));
    } else if (state_out) {
        if (state_in) *state_out = *state_in;
        else memset(state_out, 0, sizeof(*state_out));
    }
    return OOKD_OK;
}

int ookd_rx_shard_refine(ookd_rx *rx, const ookd_fsm_state *state_in, ookd_fsm_state *state_out) {
    clear_error();
    if (!rx || !state_in) {
        set_error("ookd_rx_shard_refine: null argument");
        return OOKD_ERR_ARG;
    }
    if (rx->num_carriers()) {
        set_error("ookd_rx_shard_refine: a carrier context runs whole captures, not shards");
        return OOKD_ERR_ARG;
    }
    if (rx->debounce()) {
        set_error("ookd_rx_shard_refine: the context has a debounce set (ookd_rx_set_debounce): it runs no shards");
        return OOKD_ERR_ARG;
    }
    HIPCHK(hipSetDevice(rx->dev));
    if (!rx->have_fsm || rx->run_n_out == 0) {
        if (state_out) *state_out = *state_in;
        return OOKD_OK;
    }
    int rc;
    if (rx->scan_used) {
        // the scan is cheap enough to simply run again from the new incoming state
        HIPCHK(hipMemsetAsync(rx->d_hdr.p->totals, 0, sizeof(uint64_t) * 2, rx->stream));
        HIPCHK(hipMemsetAsync(&rx->d_hdr.p->scan_fallback, 0, 2 * sizeof(uint32_t), rx->stream));   // + sync_fail
        rc = rx->run_state_machine(reinterpret_cast<const FsmStateDev *>(state_in), true);
    } else {
        rc = rx->fsm_to_fixpoint(reinterpret_cast<const FsmStateDev *>(state_in), false, true);
    }
    if (rc != OOKD_OK) return rc;
    rc = rx->fetch_results();
    if (rc != OOKD_OK) return rc;
    if (state_out) {
        const size_t nseg = rx->run_segs_per_cap;
        const SegState *src = rx->scan_used ? rx->d_final_state.p
                                            : &rx->d_state_out.p[(size_t)rx->final_parity * nseg + (nseg - 1)];
        HIPCHK(hipMemcpy(state_out, &src->st, sizeof(FsmStateDev), hipMemcpyDeviceToHost));
    }
    return OOKD_OK;
}

int ookd_rx_set_debounce(ookd_rx *rx, uint64_t min_on, uint64_t min_off) {
    clear_error();
    if (!rx) {
        set_error("ookd_rx_set_debounce: NULL argument");
        return OOKD_ERR_ARG;
    }
    if (rx->submitted) {
        set_error("ookd_rx_set_debounce: a run is in flight (ookd_rx_wait first)");
        return OOKD_ERR_ARG;
    }
    if (min_on > 1 || min_off > 1) {
        // by what the context can hold, not by any run's edge count: nothing is allocated on a run's path
        // (+ 64: as d_edges is allocated)
        const int rc = clean_chain_reserve(rx, rx->dev, rx->edge_capacity + 64, rx->max_captures, rx->max_blocks, rx->debounce_view);
        if (rc != OOKD_OK) {
            // (a buffer of the chain may be gone: the context runs on without a debounce rather than on half of them)
            rx->debounce_on = rx->debounce_off = 0;
            return rc;
        }
    }
    rx->debounce_on = min_on;
    rx->debounce_off = min_off;
    return OOKD_OK;
}

int ookd_rx_get_debounce(const ookd_rx *rx, uint64_t *min_on, uint64_t *min_off) {
    clear_error();
    if (!rx) {
        set_error("ookd_rx_get_debounce: NULL argument");
        return OOKD_ERR_ARG;
    }
    if (min_on) *min_on = rx->debounce_on;
    if (min_off) *min_off = rx->debounce_off;
    return OOKD_OK;
}

uint64_t ookd_rx_num_messages(const ookd_rx *rx) { return rx ? rx->num_msgs : 0; }

const ookd_message *ookd_rx_messages(const ookd_rx *rx) {
    static_assert(sizeof(ookd_message) == sizeof(MsgDev), "message layout");
    return rx ? reinterpret_cast<const ookd_message *>(rx->h_msgs) : nullptr;
}

int ookd_rx_get_stats(const ookd_rx *rx, ookd_rx_stats *out) {
    if (!rx || !out) return OOKD_ERR_ARG;
    *out = rx->stats;
    return OOKD_OK;
}

int ookd_rx_get_front_info(const ookd_rx *rx, ookd_front_info *out) {
    if (!rx || !out) return OOKD_ERR_ARG;
    *out = front_info(rx->front.plan, 0);
    return OOKD_OK;
}

int ookd_rx_get_carrier_front_info(const ookd_rx *rx, uint32_t k, ookd_front_info *out) {
    clear_error();
    if (!rx || !out || k >= rx->num_carriers()) {
        set_error("ookd_rx_get_carrier_front_info: bad argument");
        return OOKD_ERR_ARG;
    }
    *out = front_info(rx->front.plan, k);
    return OOKD_OK;
}

uint64_t ookd_rx_bit_words(const ookd_rx *rx) { return rx ? rx->run_words : 0; }

}  // extern "C"

// edge_pass.hpp: the last run for the edge-list readers, and where the context keeps their passes
void ookd_rx_edge_run(const ookd_rx *rx, EdgeRun *out) {
    EdgeRun r;
    r.dev = rx->dev;
    r.stream = rx->stream;
    r.serial = rx->run_serial;
    r.in_flight = rx->submitted;
    r.valid = rx->run_edges_valid;
    r.shard = rx->run_shard;
    r.pipelined = !rx->chunks.empty();
    r.overflow = rx->run_overflow;
    r.captures = rx->run_caps;
    r.blocks_per_cap = rx->run_blocks;
    r.n_out = rx->run_n_out;
    r.num_edges = rx->stats.num_edges;
    r.edge_capacity = rx->edge_capacity;
    r.d_edges = rx->d_edges.p;
    r.d_blk_offset = rx->d_blk_offset.p;
    *out = r;
}

std::unique_ptr<EdgePass> &ookd_rx_edge_pass(ookd_rx *rx, EdgePassId id) { return rx->edge_pass[id]; }

// run_levels.hpp: what the pulse-level pass reads again of the last run
void ookd_rx_level_source(const ookd_rx *rx, RunLevelSource *out) {
    out->plan = &rx->front.plan;
    out->iq = rx->last_iq;
    out->stride = rx->last_stride;
    out->n_valid = rx->run_n_valid;
}

extern "C" {

int ookd_rx_get_bits(const ookd_rx *rx, uint32_t capture, uint64_t *words, uint64_t capacity_words) {
    clear_error();
    if (!rx || !words || capture >= rx->run_caps) return OOKD_ERR_ARG;
    const uint64_t n = std::min<uint64_t>(capacity_words, rx->run_words);
    HIPCHK(hipSetDevice(rx->dev));
    {
        const int rc = rx->densify_bits();      // sparse front-end output: quiet tiles hold older runs' words
        if (rc != OOKD_OK) return rc;
    }
    HIPCHK(hipMemcpy(words, rx->d_bits.p + (size_t)capture * rx->run_words, n * 8, hipMemcpyDeviceToHost));
    return OOKD_OK;
}

int ookd_rx_get_edges(const ookd_rx *rx, uint32_t capture, uint64_t *edges, uint64_t capacity,
                      uint64_t *num_edges) {
    clear_error();
    if (!rx || capture >= rx->run_caps) return OOKD_ERR_ARG;
    HIPCHK(hipSetDevice(rx->dev));
    if (rx->run_n_out == 0) {
        if (num_edges) *num_edges = 0;
        return OOKD_OK;
    }
    if (!rx->chunks.empty()) {
        // pipelined run: one list per chunk, positions chunk-local
        std::vector<uint64_t> all;
        for (size_t c = 0; c < rx->chunks.size(); ++c) {
            const Chunk &ch = rx->chunks[c];
            uint32_t ne = 0;
            HIPCHK(hipMemcpy(&ne, rx->d_blk_offset.p + ch.blk0 + c + ch.nblk, 4, hipMemcpyDeviceToHost));
            std::vector<uint64_t> loc(std::min<uint64_t>(ne, ch.edge_cap));
            if (!loc.empty()) {
                HIPCHK(hipMemcpy(loc.data(), rx->d_edges.p + ch.edge_off, loc.size() * 8, hipMemcpyDeviceToHost));
            }
            for (uint64_t e : loc) all.push_back(e + ch.out0);
        }
        if (num_edges) *num_edges = all.size();
        if (edges && !all.empty()) memcpy(edges, all.data(), std::min<uint64_t>(all.size(), capacity) * 8);
        return OOKD_OK;
    }
    uint32_t off[2];
    HIPCHK(hipMemcpy(&off[0], rx->d_blk_offset.p + (size_t)capture * rx->run_blocks, 4, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(&off[1], rx->d_blk_offset.p + (size_t)(capture + 1) * rx->run_blocks, 4,
                     hipMemcpyDeviceToHost));
    const uint64_t n = off[1] - off[0];
    if (num_edges) *num_edges = n;
    if (edges && n) {
        HIPCHK(hipMemcpy(edges, rx->d_edges.p + off[0], std::min<uint64_t>(n, capacity) * 8,
                         hipMemcpyDeviceToHost));
    }
    return OOKD_OK;
}

int ookd_rx_get_fir(const ookd_rx *rx, uint32_t capture, ookd_complexf *out, uint64_t capacity) {
    clear_error();
    if (!rx || !out || capture >= rx->run_caps) return OOKD_ERR_ARG;
    if (!rx->d_fir.p) {
        set_error("ookd_rx_get_fir needs OOKD_RX_KEEP_FIR");
        return OOKD_ERR_ARG;
    }
    HIPCHK(hipSetDevice(rx->dev));
    const uint64_t n = std::min<uint64_t>(capacity, rx->run_n_out);
    HIPCHK(hipMemcpy(out, rx->d_fir.p + 2 * (size_t)capture * rx->run_n_out, n * 8, hipMemcpyDeviceToHost));
    return OOKD_OK;
}

int ookd_rx_get_errors(const ookd_rx *rx, uint64_t *samples, uint64_t capacity, uint64_t *num) {
    clear_error();
    if (!rx) return OOKD_ERR_ARG;
    if (num) *num = rx->stats.num_errors;
    if (!rx->have_fsm || rx->run_n_out == 0 || !samples || capacity == 0) return OOKD_OK;
    HIPCHK(hipSetDevice(rx->dev));
    if (rx->mixed_valid) {              // scan + rounds for the captures it refused: the list lives on the host
        const uint64_t n = std::min<uint64_t>(rx->mixed_errs.size(), capacity);
        if (n) memcpy(samples, rx->mixed_errs.data(), n * 8);
        return OOKD_OK;
    }
    if (rx->scan_used) {
        const uint64_t n = std::min<uint64_t>(std::min<uint64_t>(rx->stats.num_errors, capacity), rx->d_scan_errs.n);
        if (n) HIPCHK(hipMemcpy(samples, rx->d_scan_errs.p, n * 8, hipMemcpyDeviceToHost));
        return OOKD_OK;
    }
    const size_t nseg = (size_t)rx->run_caps * rx->run_segs_per_cap;
    std::vector<uint32_t> counts(nseg);
    std::vector<uint64_t> errs(nseg * rx->err_slots);
    HIPCHK(hipMemcpy(counts.data(), rx->d_seg_err_count.p, nseg * 4, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(errs.data(), rx->d_seg_errs.p, errs.size() * 8, hipMemcpyDeviceToHost));
    uint64_t at = 0;
    for (size_t s = 0; s < nseg && at < capacity; ++s) {
        const uint32_t c = std::min<uint32_t>(counts[s], rx->err_slots);
        for (uint32_t i = 0; i < c && at < capacity; ++i) samples[at++] = errs[s * rx->err_slots + i];
    }
    return OOKD_OK;
}

}  // extern "C"

// ---------------------------------------------------------------------------
// recorders
// ---------------------------------------------------------------------------

namespace {

// record_dig (ookiedokie.c:146-169) restated over the edge list: the first
// line is sample 0's level, every later level change at i writes the pair
// "i-1, old" / "i, new".  The edge list counts a capture that starts high as
// a change at 0 (level before the capture = 0); record_dig does not.
template <typename Sink>
void dig_lines(const uint64_t *edges, uint64_t n, Sink &&sink) {
    char line[96];
    bool level = n > 0 && edges[0] == 0;
    int m = snprintf(line, sizeof(line), "0, %c\n", level ? '1' : '0');
    sink(line, (size_t)m);
    for (uint64_t e = level ? 1 : 0; e < n; ++e) {
        const uint64_t i = edges[e];
        m = snprintf(line, sizeof(line), "%" PRIu64 ", %c\n%" PRIu64 ", %c\n", i - 1, level ? '1' : '0', i,
                     level ? '0' : '1');
        sink(line, (size_t)m);
        level = !level;
    }
}

int fetch_edges(const ookd_rx *rx, uint32_t capture, std::vector<uint64_t> &edges) {
    uint64_t n = 0;
    int rc = ookd_rx_get_edges(rx, capture, nullptr, 0, &n);
    if (rc != OOKD_OK) return rc;
    if (n > rx->edge_capacity) {
        set_error("edge list overflowed its capacity: raise ookd_rx_config.edge_capacity");
        return OOKD_ERR_CAPACITY;
    }
    edges.resize(n);
    if (n) rc = ookd_rx_get_edges(rx, capture, edges.data(), n, &n);
    return rc;
}

}  // namespace

extern "C" {

size_t ookd_rx_dig_text(const ookd_rx *rx, uint32_t capture, char *out, size_t capacity) {
    clear_error();
    if (out && capacity) out[0] = '\0';
    if (!rx || capture >= rx->run_caps) {
        set_error("ookd_rx_dig_text: bad argument");
        return 0;
    }
    if (rx->run_n_out == 0) return 0;           // no buffer was ever processed: record_dig never ran
    std::vector<uint64_t> edges;
    if (fetch_edges(rx, capture, edges) != OOKD_OK) return 0;
    size_t len = 0;
    dig_lines(edges.data(), edges.size(), [&](const char *s, size_t m) {
        if (out && len < capacity) memcpy(out + len, s, std::min(m, capacity - len));
        len += m;
    });
    if (out && capacity) out[std::min(len, capacity - 1)] = '\0';
    return len;
}

int ookd_rx_record_dig(const ookd_rx *rx, uint32_t capture, const char *path) {
    clear_error();
    if (!rx || !path || capture >= rx->run_caps) {
        set_error("ookd_rx_record_dig: bad argument");
        return OOKD_ERR_ARG;
    }
    std::vector<uint64_t> edges;
    if (rx->run_n_out) {
        int rc = fetch_edges(rx, capture, edges);
        if (rc != OOKD_OK) return rc;
    }
    FILE *f = fopen(path, "w");                 // ookiedokie.c:112
    if (!f) {
        set_error("Failed to open %s: %s", path, strerror(errno));
        return OOKD_ERR_IO;
    }
    bool ok = true;
    if (rx->run_n_out) {
        dig_lines(edges.data(), edges.size(), [&](const char *s, size_t m) { ok = ok && fwrite(s, 1, m, f) == m; });
    }
    ok = (fclose(f) == 0) && ok;
    if (!ok) {
        set_error("Failed to write %s", path);
        return OOKD_ERR_IO;
    }
    return OOKD_OK;
}

int ookd_rx_get_fir_sc16q11(const ookd_rx *rx, uint32_t capture, int16_t *out, uint64_t capacity) {
    clear_error();
    if (!rx || !out || capture >= rx->run_caps) return OOKD_ERR_ARG;
    if (!rx->d_fir.p) {
        set_error("ookd_rx_get_fir_sc16q11 needs OOKD_RX_KEEP_FIR");
        return OOKD_ERR_ARG;
    }
    HIPCHK(hipSetDevice(rx->dev));
    const uint64_t n = std::min<uint64_t>(capacity, rx->run_n_out);
    if (n == 0) return OOKD_OK;
    int16_t *d_tmp = nullptr;
    HIPCHK(hipMalloc(reinterpret_cast<void **>(&d_tmp), n * 4));
    hipError_t e = launch_pack(rx->d_fir.p + 2 * (size_t)capture * rx->run_n_out, d_tmp, n, rx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(out, d_tmp, n * 4, hipMemcpyDeviceToHost, rx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(rx->stream);
    (void)hipFree(d_tmp);
    if (e != hipSuccess) {
        set_error("ookd_rx_get_fir_sc16q11: %s", hipGetErrorString(e));
        return OOKD_ERR_HIP;
    }
    return OOKD_OK;
}

int ookd_rx_record_fir(const ookd_rx *rx, uint32_t capture, const char *path) {
    clear_error();
    if (!rx || !path || capture >= rx->run_caps) {
        set_error("ookd_rx_record_fir: bad argument");
        return OOKD_ERR_ARG;
    }
    if (!rx->d_fir.p) {
        set_error("ookd_rx_record_fir needs OOKD_RX_KEEP_FIR");
        return OOKD_ERR_ARG;
    }
    std::vector<int16_t> buf(2 * rx->run_n_out);
    if (rx->run_n_out) {
        int rc = ookd_rx_get_fir_sc16q11(rx, capture, buf.data(), rx->run_n_out);
        if (rc != OOKD_OK) return rc;
    }
    FILE *f = fopen(path, "wb");                // bladeRF_file.c:82 (tx direction)
    if (!f) {
        set_error("Failed to open %s: %s", path, strerror(errno));
        return OOKD_ERR_IO;
    }
    bool ok = fwrite(buf.data(), 4, rx->run_n_out, f) == rx->run_n_out;
    ok = (fclose(f) == 0) && ok;
    if (!ok) {
        set_error("Failed to write %s", path);
        return OOKD_ERR_IO;
    }
    return OOKD_OK;
}

}  // extern "C"
