/*
 * ookiedokie_amd.h -- C ABI of the MI355X-native OOK receive / demodulation
 * path (libookiedokie_amd.so).
 *
 * This is the drop-in boundary for OOKiedokie's rx hot loop
 *     SC16Q11 -> complexf -> FIR -> |.| >= thr -> symbol state machine
 * (reference: src/ookiedokie.c:238-290).  Plain C types only: pointers,
 * sizes, opaque handles.  Every entry point names the reference interface
 * it replaces (file:line under the OOKiedokie source tree).  How a
 * maintainer binds it from the existing C host is shown in INTEGRATION.md.
 *
 * Conventions kept from the reference:
 *   - constructors return a heap handle or NULL; `*_free(NULL)` is a no-op;
 *   - functions returning int use 0 = success, non-zero = failure;
 *     OOKD_FILE_EOF (= INT_MIN, src/sdr/sdr.h:36) means clean end of input;
 *   - nothing here calls exit(); the text of the last failure on the
 *     calling thread is available from ookd_last_error() (the reference
 *     prints the same kind of text through log_error, src/log.h);
 *   - handles are not thread safe; one rx context per host thread / GPU.
 *
 * There is NO CPU fallback: every compute entry point needs a HIP device
 * and fails with OOKD_ERR_HIP otherwise.
 */
#ifndef OOKIEDOKIE_AMD_H
#define OOKIEDOKIE_AMD_H

#include <limits.h>
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OOKD_API_VERSION 1

/* src/sdr/sdr.h:36 */
#define OOKD_FILE_EOF INT_MIN

enum {
    OOKD_OK = 0,
    OOKD_ERR_ARG = -1,          /* bad argument / unsupported configuration  */
    OOKD_ERR_IO = -2,           /* file could not be opened / read            */
    OOKD_ERR_PARSE = -3,        /* JSON syntax or schema error                */
    OOKD_ERR_HIP = -4,          /* HIP runtime failure (message has details)  */
    OOKD_ERR_CAPACITY = -5,     /* a device-side list overflowed; see message */
    OOKD_ERR_NOMEM = -6
};

/* Payload bytes carried per decoded message: supports num_bits <= 256. */
#define OOKD_MAX_PAYLOAD_BYTES 32

/* src/complexf.h:31-34 */
typedef struct ookd_complexf {
    float real;
    float imag;
} ookd_complexf;

/* Text of the last error raised on this thread ("" if none). */
const char *ookd_last_error(void);
int ookd_api_version(void);

/* ------------------------------------------------------------------------
 * Filter: replaces fir_init / fir_deinit / fir_get_total_decimation
 * (src/fir.h:43-66, loader src/fir.c:68-249).  The JSON schema is the
 * reference's, unchanged (filters/README.md:31-63): decimation optional,
 * default 1, must be > 0; taps are numbers cast double -> float.
 * `path` is an explicit file name (the reference's search path, src/find.c,
 * stays with the host).
 * ---------------------------------------------------------------------- */
typedef struct ookd_filter ookd_filter;

ookd_filter *ookd_filter_load(const char *path);
ookd_filter *ookd_filter_create(uint32_t num_stages,
                                const uint32_t *decimation,
                                const uint32_t *num_taps,
                                const float *taps /* all stages, in order */);
void ookd_filter_free(ookd_filter *f);
uint32_t ookd_filter_total_decimation(const ookd_filter *f);  /* fir.h:66 */
uint32_t ookd_filter_num_stages(const ookd_filter *f);
/* Stage geometry and a pointer to its float taps (owned by the filter). */
int ookd_filter_stage(const ookd_filter *f, uint32_t stage,
                      uint32_t *decimation, uint32_t *num_taps,
                      const float **taps);

/* ------------------------------------------------------------------------
 * Frequency-tuned taps: decode a carrier that is NOT at 0 Hz (a zero-IF
 * receiver tuned beside the transmitter to keep its DC spike out of the way;
 * one of several transmitters in a wide capture) with the low-pass filters as
 * they are.  The slicer only looks at |y|, and
 *   | sum_k h[k] x[n-k] e^{-j 2 pi nu (n-k)} | = | sum_k (h[k] e^{+j 2 pi nu k}) x[n-k] |,
 * so "mix down by nu, then low-pass with h" has the envelope of ONE FIR with
 * complex taps c[k] = h[k] e^{j 2 pi nu k} on the raw samples: no oscillator,
 * no phase state -- a capture, a chunk or a shard may start anywhere.
 *
 * nu = carrier offset in cycles per INPUT sample (offset_hz / sample_rate),
 * |nu| <= 0.5.  The contract, taps (pure host code, no GPU): for stage s with
 * P_s = the product of the decimations before it, tap k:
 *     t = nu * (P_s k) (double; P_s k is an integer),  r = t - rint(t),
 *     re[k] = (float)(h[k] * cos(2 pi r)),   im[k] = (float)(h[k] * sin(2 pi r)),
 * evaluated for |nu| with the sign of nu put on im afterwards, and a sine that
 * is exactly 0 giving im = 0 of that sign.  So nu = 0 gives re == h bitwise and
 * im == +0; -nu gives the same re and the bitwise negated im, also on the taps
 * whose phase is a whole turn.  re / im receive num_taps of that stage each.
 * OOKD_ERR_ARG for NaN, |nu| > 0.5, NULL, a stage the filter does not have.
 *
 * The contract, one stage output: all float32, UNFUSED, taps newest sample
 * first (k = 0 multiplies the newest sample, as fir.c does), accumulators
 * from +0, four statements per tap in this order:
 *     ar = ar + re[k]*xr;   ar = ar - im[k]*xi;
 *     ai = ai + re[k]*xi;   ai = ai + im[k]*xr;
 * Stages chain, decimate and start from zero history exactly as the untuned
 * path; the power is ar*ar + ai*ai against the same threshold.  With im == 0
 * every extra term is +-0, so nu = 0 is the reference's result bit for bit.
 * ---------------------------------------------------------------------- */
int ookd_filter_tuned_taps(const ookd_filter *f, double nu, uint32_t stage,
                           float *re, float *im);

/* ------------------------------------------------------------------------
 * Device: replaces device_init / device_deinit (src/device.h:47-91, loader
 * src/device.c:76-632) for the rx direction.  `sample_rate` is the rate the
 * state machine sees, i.e. samplerate / total decimation (src/main.c:683).
 * The device JSON is consumed unchanged (devices/README.md).
 * ---------------------------------------------------------------------- */
typedef struct ookd_device ookd_device;

/* Flat view of the state machine tables (what sm_add_state /
 * sm_add_state_trigger were fed, src/state_machine.c:250-335); state 0 is
 * the reset state.  Pointers are owned by the device handle. */
typedef struct ookd_fsm_tables {
    uint32_t num_states;
    uint32_t max_bits;
    uint32_t sample_rate;
    uint32_t num_triggers;
    const uint64_t *state_duration_us;
    const uint64_t *state_timeout_us;
    const uint32_t *trig_begin;         /* num_states + 1 */
    const uint8_t *trig_cond;           /* enum sm_trigger_cond values   */
    const uint8_t *trig_action;         /* enum sm_trigger_action values */
    const uint32_t *trig_next;
    const uint64_t *trig_duration_us;
    /* Integer sample-count form of the above, obtained by replaying the
     * reference's double accumulation of elapsed_us (state_machine.c:78-82,
     * :514) against its float windows (:100-133) -- what the GPU uses.
     * A window is empty when kmin > kmax; "none" is encoded as kmin = 0,
     * kmax = UINT64_MAX; no timeout as UINT64_MAX. */
    const uint64_t *state_kmin, *state_kmax, *state_kto;
    const uint64_t *trig_kmin, *trig_kmax;
} ookd_fsm_tables;

ookd_device *ookd_device_load(const char *path, uint32_t sample_rate);
ookd_device *ookd_device_create(const ookd_fsm_tables *t /* *_us fields + counts */);
void ookd_device_free(ookd_device *d);
uint32_t ookd_device_num_bits(const ookd_device *d);
const char *ookd_device_name(const ookd_device *d);
const char *ookd_device_state_name(const ookd_device *d, uint32_t state);
int ookd_device_tables(const ookd_device *d, ookd_fsm_tables *out);

/* ------------------------------------------------------------------------
 * Rx context: the fused replacement for one or more iterations of the
 * reference loop body, src/ookiedokie.c:243-288
 *     sdr_rx -> fir_filter_and_decimate -> threshold -> device_process
 * over a whole SC16Q11 capture resident in HBM.  Semantics kept:
 *   - the capture is consumed in buffers of `samples_per_buffer` input
 *     samples; a short final buffer is zero padded and fully processed
 *     (src/sdr/bladeRF_file.c:107-119), so ceil(n/spb)*spb samples are
 *     filtered and floor(that / total_decimation) are decoded;
 *   - FIR history starts at zero (fir_reset, src/fir.c:272-295), outputs
 *     at input indices D-1, 2D-1, ...;
 *   - after a state machine ERROR the rest of THAT buffer is not fed to the
 *     state machine (src/device.c:646) -- results depend on
 *     samples_per_buffer exactly as the reference's do.
 * filter may be NULL ("-F none", ookiedokie.c:260-263); device may be NULL
 * (threshold / bit stream only).
 * ---------------------------------------------------------------------- */
typedef struct ookd_rx ookd_rx;

enum {
    /* FIR arithmetic. Default (0): fused multiply-add accumulation plus a
     * guard band around the threshold inside which the sample is recomputed
     * in the reference's exact order -- bits are identical to the
     * reference, floats within 1e-5.  EXACT: unfused mul/add in reference
     * order everywhere -- floats bit-identical too, ~half the speed. */
    OOKD_RX_EXACT_FIR = 1u << 0,
    /* Keep the post-filter complexf stream in HBM (parity / --rx-rec). */
    OOKD_RX_KEEP_FIR = 1u << 1,
    /* State machine: always use the segment/round path.  By default the
     * state machine runs as a scan of per-edge transition functions and
     * falls back to this path only when a capture leaves the scan's model
     * (results are identical either way). */
    OOKD_RX_FSM_ROUNDS = 1u << 2,
    /* Front end: never take the "quiet" shortcut.  By default a wavefront whose
     * whole input window is provably too small to reach the threshold
     * (sqrt(2) * sum|taps| * max|sample| < threshold) emits its 1024 zero bits
     * without running the filter -- the bits are identical, captures that are
     * mostly silence run at memory speed.  Set this to time the worst case. */
    OOKD_RX_NO_QUIET_SKIP = 1u << 3,
    /* Diagnostics: count the windows that took the shortcut (one atomic per
     * quiet window -- slows the front end, keep out of timed runs). */
    OOKD_RX_COUNT_QUIET = 1u << 4,
    /* State machine scan: simulate every span instead of looking its result
     * up in the per-device span tables built at create time (identical
     * results; exists so the tests can run both). */
    OOKD_RX_SCAN_SIMS = 1u << 5,
    /* Accepted and ignored: the grid is the only form of the front end. */
    OOKD_RX_FRONT_GRID = 1u << 6,
    /* Never pipeline a long capture in chunks (see pipeline_chunk_samples). */
    OOKD_RX_NO_PIPELINE = 1u << 7,
    /* Front end, single-stage filters of up to 256 taps without decimation: by
     * default the filter runs on the matrix cores (taps and samples split into
     * fp16 pieces whose products are exact, fp32 accumulation, guard band +
     * exact recompute as in the fused form: identical bits, floats within 1e-5).
     * Set this for the packed-VALU loop instead (exists so the tests run both). */
    OOKD_RX_FIR_VALU = 1u << 8,
    /* State machine scan: always compose the per-block transition tables.  By
     * default an edge list of 20 000 edges and more is first searched for
     * SYNCHRONISING spans -- stretches of constant level long enough that the
     * machine can only end them in one of a few states whatever state it
     * entered them in (the silence between two messages) --, every stretch
     * between two of them is walked once per such state, and a scan over the
     * resulting few-entry maps picks the true one; the composing kernels run
     * for short edge lists and for captures without such spans (no one within
     * 512 edges).  Identical results; the flag exists so the tests can run
     * both (stats.scan_entry_form). */
    OOKD_RX_SCAN_TABLES = 1u << 9,
    /* Sample format of every capture (and shard halo) the context is given.  Neither bit: SC16Q11,
     * int16 I,Q, 4 bytes per sample (bladeRF).  One of them: 8-bit I,Q pairs, 2 bytes per sample --
     *   CS8: signed bytes, the `.cs8` files HackRF tools write (hackrf_transfer);
     *   CU8: unsigned bytes around 128, the `.cu8` files rtl_sdr writes.
     * An 8-bit sample IS the SC16Q11 sample of 16 times its value:
     *   CS8 v (int8)  = SC16Q11 16 * v,    CU8 u (uint8) = SC16Q11 16 * (u - 128),
     * so the unpacked float is v / 128 = (16 v) / 2048 exactly, and a run computes, bit for bit,
     * what the same context without the flag computes on the capture widened to int16 that way.
     * The fused front ends (OOKD_FRONT_*_8) read the 2-byte samples themselves; nothing widens the
     * capture in HBM first.  Zero padding is value 0 of the format (the byte 128 for CU8).  Both
     * bits set: ookd_rx_create fails. */
    OOKD_RX_SAMPLES_CS8 = 1u << 10,
    OOKD_RX_SAMPLES_CU8 = 1u << 11,
    /* Tuned and carrier contexts (ookd_rx_create_tuned with nu != 0, ookd_rx_create_carriers) on a
     * filter of two decimate-by-2 stages with <= 16 and <= 32 taps (the backend default
     * fs128_fs16_dec4): run the fused kernel OOKD_FRONT_TUNED_FIR2 -- packed FMAs, guard band with
     * recompute in the contract's order, quiet shortcut, sparse output -- in place of
     * OOKD_FRONT_TUNED_GENERIC.  The contract is unchanged: bits, edges, messages and error
     * positions are those of ookd_filter_tuned_taps's contract, exactly; OOKD_RX_KEEP_FIR floats are
     * within err_valu per component.  Accepted and without effect on every other context: untuned
     * ones, nu = 0, other filter shapes, OOKD_RX_EXACT_FIR. */
    OOKD_RX_TUNED_FIR2 = 1u << 12
};

/* Contexts created with the same gate (and on the same device) queue their front-end kernels one
 * after the other instead of side by side: the front end is HBM bound, two at once only slow each
 * other down, while the latency-bound edges / state machine of one capture do overlap the next
 * context's front end.  For hosts that keep several captures in flight (bench.py does).  The gate
 * must outlive the contexts that use it; contexts without one never wait for anybody. */
typedef struct ookd_rx_gate ookd_rx_gate;
ookd_rx_gate *ookd_rx_gate_create(void);
void ookd_rx_gate_destroy(ookd_rx_gate *gate);

typedef struct ookd_rx_config {
    int32_t hip_device;             /* ordinal, e.g. LOCAL_RANK               */
    uint32_t flags;                 /* OOKD_RX_*                              */
    float threshold;                /* cfg->rx_threshold, default 0.1f        */
    uint32_t samples_per_buffer;    /* cfg->samples_per_buffer, default 8192  */
    uint64_t max_samples;           /* largest capture (input samples) / run  */
    uint32_t max_captures;          /* captures per batched run (>= 1)        */
    uint64_t edge_capacity;         /* 0 = default (max_samples/32 + 1M)      */
    uint32_t segment_buffers;       /* buffers per FSM segment, 0 = default   */
    uint32_t message_slots;         /* per segment, 0 = default               */
    uint64_t message_capacity;      /* messages per run, 0 = default (65536)  */
    void *stream;                   /* hipStream_t to launch on, NULL = own.  A run reads its capture in
                                       the stream's order: work queued on the caller's stream before
                                       ookd_rx_submit_device (the copy or kernel that produces the
                                       capture) is finished when the run reads it, and the buffer may be
                                       overwritten once ookd_rx_wait has returned.  A context's own stream
                                       is non-blocking and waits for nobody: synchronise the producer
                                       before submitting to it.                                        */
    uint64_t pipeline_chunk_samples;/* non-zero: single-capture runs at least twice this long are
                                       pipelined in chunks of about this many input samples: the front
                                       end of chunk c+1 is queued beside the edges / state machine of
                                       chunk c, the state machine's state carried from chunk to chunk in
                                       device memory (results identical).  0 = never (the default: on
                                       this runtime the chunked run is slower)          */
    ookd_rx_gate *front_gate;       /* shared front-end gate (see above), NULL = none */
} ookd_rx_config;

typedef struct ookd_message {
    uint32_t capture;               /* index within a batched run             */
    uint32_t reserved;
    uint64_t sample;                /* decimated sample index on which the
                                       state machine returned OUTPUT_READY
                                       (sm_process, state_machine.c:541-556)  */
    uint8_t payload[OOKD_MAX_PAYLOAD_BYTES]; /* first received bit = bit 0 of
                                       byte 0 (state_machine.c:365-385)       */
} ookd_message;

/* Carried state of the symbol state machine between shards of one capture
 * (what struct state_machine holds across sm_process calls,
 * src/state_machine.c:57-75): current state, increments of elapsed_us since
 * it was last zeroed, previous bit, bits collected so far and the payload.
 *
 * A state_out is what the sequential machine holds in front of the shard's
 * next sample, and it is canonical: two shards that leave the machine in the
 * same condition hand on the same 64 bytes, whichever form of the state
 * machine ran (callers compare states as bytes to see whether a refinement
 * changed anything).  All zero is the reset state a capture starts in.
 *   state, prev_bit : the machine's.  Behind an error the rest of that buffer
 *       is dropped: state is the reset state and prev_bit the level of the
 *       ERROR sample, not that of the shard's last sample.
 *   num_bits, payload : as the machine holds them, first bit = bit 0 of byte 0.
 *       In the reset state they are still those of the message (or the error)
 *       before: the machine zeroes them on its next sample and nothing reads
 *       them before that.  Payload bits at and above num_bits, and every byte
 *       behind them, are 0.
 *   k : increments of elapsed_us (one per evaluation without a firing) since
 *       it was last zeroed, in every state that looks at it -- a state or
 *       trigger duration, a time-out that a trigger waits for.  In a state in
 *       which nothing reads it (the reset state, an idle state without a
 *       time-out) k is 0, however long the machine has been there.  k
 *       saturates: a state_out never holds more than 0xfffffffe, and a
 *       state_in above that is read as that (no device window reaches it:
 *       devices with a finite bound above 2^31 increments are refused).
 *   reserved : 0. */
typedef struct ookd_fsm_state {
    uint32_t state;
    uint32_t num_bits;
    uint64_t k;
    uint32_t prev_bit;
    uint32_t reserved;
    uint8_t payload[OOKD_MAX_PAYLOAD_BYTES + 8];
} ookd_fsm_state;

typedef struct ookd_rx_stats {
    uint64_t input_samples;         /* per capture, after zero padding        */
    uint64_t decimated_samples;     /* per capture                            */
    uint64_t num_edges;             /* whole batch                            */
    uint64_t num_messages;
    uint64_t num_errors;            /* state machine ERROR events             */
    uint64_t guard_recomputes;      /* samples redone in exact order          */
    uint32_t fsm_iterations;        /* segment-parallel fix-point rounds      */
    uint32_t num_segments;
    uint32_t fsm_path;              /* 1 scan, 2 rounds, 3 scan fell back to rounds */
    uint32_t fsm_fallback_reason;   /* scan's refusal bits (0 = none)         */
    float fir_kernel_ms;            /* HIP-event time of the dominant kernel  */
    float total_device_ms;          /* first kernel start -> last kernel end  */
    uint64_t quiet_waves;           /* 1024-output windows that took the quiet
                                       shortcut (only with OOKD_RX_COUNT_QUIET) */
    uint64_t total_waves;           /* 1024-output windows of the run (1-stage
                                       decimation-1 front end; else 0)        */
    uint32_t pipeline_chunks;       /* chunks the run was pipelined in (0 = not pipelined) */
    uint32_t front_launches;        /* grid launches the front end went out as; fir_kernel_ms spans
                                       first start -> last end                */
    uint32_t scan_entry_form;       /* how the scan found the leaves' entry states: 1 walk from
                                       synchronising spans, 2 composed block tables, 0 no scan */
    uint32_t front_form;            /* the front-end kernel the run launched: OOKD_FRONT_* */
} ookd_rx_stats;

/* Front-end forms (ookd_rx_stats.front_form, ookd_front_info.form): which
 * kernel computed the filter, power and threshold.  0 = no run yet. */
enum {
    OOKD_FRONT_NO_FILTER = 1,       /* no filter: threshold on the samples      */
    OOKD_FRONT_GENERIC = 2,         /* any shape, reference order throughout    */
    OOKD_FRONT_FIR1_VALU = 3,       /* 1 stage, decimation 1, <= 256 taps:
                                       packed-VALU FMA + guard band             */
    OOKD_FRONT_FIR1_VALU_EXACT = 4, /* ... reference order (OOKD_RX_EXACT_FIR)  */
    OOKD_FRONT_FIR1_MFMA = 5,       /* ... matrix cores + guard band            */
    OOKD_FRONT_FIR2_VALU = 6,       /* 2 x decimate-by-2 (<= 16, <= 32 taps):
                                       packed-VALU FMA + guard band             */
    OOKD_FRONT_FIR2_VALU_EXACT = 7, /* ... reference order (OOKD_RX_EXACT_FIR)  */
    OOKD_FRONT_FIR2_MFMA = 8,       /* ... folded decimate-by-4 on the matrix
                                       cores + guard band                       */
    /* 8-bit contexts (OOKD_RX_SAMPLES_CS8 / _CU8): the fused forms that read the
     * 2-byte samples themselves.  An 8-bit run that reports one of the numbers
     * above ran that 16-bit kernel on a widened staging copy of the capture
     * (OOKD_RX_FIR_VALU, OOKD_RX_EXACT_FIR, filters the matrix cores refuse,
     * generic shapes); the staging buffer is allocated on the first such run. */
    OOKD_FRONT_NO_FILTER_8 = 9,
    OOKD_FRONT_FIR1_MFMA_8 = 10,
    OOKD_FRONT_FIR2_MFMA_8 = 11,
    /* Tuned contexts (ookd_rx_create_tuned, nu != 0): complex taps on the raw
     * samples.  All of them read SC16Q11; an 8-bit tuned context runs them on a
     * widened staging copy of the capture, like the non-fused forms above. */
    OOKD_FRONT_TUNED_GENERIC = 12,  /* any shape, the contract's order throughout
                                       (also what OOKD_RX_EXACT_FIR selects):
                                       KEEP_FIR floats are the contract's       */
    OOKD_FRONT_TUNED_FIR1 = 13,     /* 1 stage, decimation 1, <= 256 taps:
                                       packed-VALU FMA (four per sample-tap) +
                                       guard band, recompute in contract order  */
    /* Carrier contexts (ookd_rx_create_carriers): OOKD_FRONT_TUNED_FIR1's shape for
     * all carriers in one pass over the capture.  Every other shape, and
     * OOKD_RX_EXACT_FIR, runs OOKD_FRONT_TUNED_GENERIC once per carrier and reports 12. */
    OOKD_FRONT_TUNED_MULTI = 14,
    /* Tuned and carrier contexts created with OOKD_RX_TUNED_FIR2: 2 x decimate-by-2
     * (<= 16, <= 32 taps), packed-VALU FMA (four per sample-tap) in both stages +
     * guard band, recompute in contract order from the raw window.  A carrier
     * context runs it once per carrier and reports 15 too. */
    OOKD_FRONT_TUNED_FIR2 = 15
};

/* The front end a context settled on at create time, and the forward error
 * bounds its guard bands were built from.  Bounds are per component of a
 * filter output, in output units (2048 LSB = 1): a sample whose power lies
 * in the band around p_star is recomputed in the reference's order, so bits
 * are the reference's as long as |y_kernel - y_ref| stays within them. */
typedef struct ookd_front_info {
    uint32_t form;                  /* OOKD_FRONT_* of a run started now       */
    uint32_t mfma_ksteps;           /* K-steps of the matrix-core product (0 = none prepared) */
    float p_star;                   /* smallest power whose sqrtf >= threshold */
    float p_lo, p_hi;               /* the packed-VALU kernels' band (tuned
                                       context: OOKD_FRONT_TUNED_FIR1's or
                                       OOKD_FRONT_TUNED_FIR2's)                */
    float mfma_c;                   /* matrix-core accumulator -> output scale */
    double err_nominal;             /* matrix-core form, samples in [-2048, 2047] */
    double err_wide;                /* matrix-core form, any int16 samples     */
    double err_valu;                /* packed-VALU form, any int16 samples
                                       (tuned context: OOKD_FRONT_TUNED_FIR1 or
                                       OOKD_FRONT_TUNED_FIR2 against the
                                       contract's order)                       */
    double mfma_delta;              /* sum |h - (h1 + h2)|: what the two fp16
                                       tap pieces do not carry                 */
} ookd_front_info;

/* Filters: any ookd_filter of up to 8 stages whose shape one of the fused kernels takes (1 stage of
 * decimation 1 with <= 256 taps; 2 decimate-by-2 stages of <= 16 and <= 32 taps).  Every other shape runs
 * on the generic kernels, which build each level of a tile of L final outputs in LDS: level s holds
 * len_s = D_s * (len_{s+1} - 1) + T_s samples (len_S = L; D_s, T_s: decimation and tap count of stage s),
 * and a tile needs (max len of the even levels + max len of the odd levels + 2) * 8 bytes.  L is the
 * largest power of two in [64, 1024] for which that is <= 163840 bytes (160 KiB).  A filter that does not
 * fit L = 64 -- one stage: 63 * D + T > 20478, e.g. any decimation beyond 325 -- is refused here, by
 * ookd_rx_create_tuned, ookd_rx_create_carriers and ookd_fir_create (NULL; ookd_last_error names the
 * total decimation, the tap counts and the limit), never by a run. */
ookd_rx *ookd_rx_create(const ookd_rx_config *cfg, const ookd_filter *filter,
                        const ookd_device *device);
/* A context tuned to a carrier at nu cycles per input sample (see
 * ookd_filter_tuned_taps for the contract).  tune == NULL or nu == 0 IS
 * ookd_rx_create: same kernels, same front_form.  Otherwise the front end is
 * one of the OOKD_FRONT_TUNED_* forms; bit words, edges, state machine,
 * recorders, batches, shards and ookd_rx_halo_samples are what they were, and
 * every run entry point below works.  OOKD_RX_FIR_VALU is accepted and changes
 * nothing.  Fails for NaN or |nu| > 0.5, and for nu != 0 without a filter:
 * |x| of the unfiltered samples does not depend on nu, there is nothing to tune.
 * Not tuned (yet): the matrix-core forms, ookd_fir_*.  (The envelope survey has
 * its own tuned entry point: ookd_survey_create_tuned.)
 * Two decimate-by-2 stages (<= 16 and <= 32 taps, e.g. fs128_fs16_dec4) run
 * OOKD_FRONT_TUNED_GENERIC unless cfg->flags holds OOKD_RX_TUNED_FIR2: then the
 * fused kernel OOKD_FRONT_TUNED_FIR2 runs, unless OOKD_RX_EXACT_FIR is set too.
 * The contract does not change with the flag: bits, edges, messages and error
 * positions are those of ookd_filter_tuned_taps's contract, exactly, and
 * OOKD_RX_KEEP_FIR floats are within err_valu per component (bitwise the
 * contract's without the flag).  On every other shape the flag changes nothing. */
typedef struct ookd_tune {
    double nu;                      /* cycles per input sample, |nu| <= 0.5     */
    uint64_t reserved[3];           /* zero                                     */
} ookd_tune;
ookd_rx *ookd_rx_create_tuned(const ookd_rx_config *cfg, const ookd_filter *filter,
                              const ookd_device *device, const ookd_tune *tune);
double ookd_rx_tune(const ookd_rx *rx);    /* nu of the context, 0 for an untuned one */

/* Several carriers of ONE capture in one context: the capture is read from HBM,
 * tested for silence and unpacked once, the complex-tap accumulation and the
 * threshold run per carrier (OOKD_FRONT_TUNED_MULTI, for the shape
 * OOKD_FRONT_TUNED_FIR1 takes: 1 stage, decimation 1, <= 256 taps).
 *
 * CONTRACT.  Carrier k of a run is, bit for bit, the run of
 * ookd_rx_create_tuned(cfg with threshold = carriers[k].threshold, filter,
 * device, {carriers[k].nu}) on the same capture: bit words, edges, OUTPUT_READY
 * sample indices, payloads and error positions.  With OOKD_RX_KEEP_FIR the
 * floats are within that carrier's err_valu (ookd_rx_get_carrier_front_info) of
 * the contract at ookd_filter_tuned_taps, and bitwise equal to it under
 * OOKD_RX_EXACT_FIR.  nu = 0 is a legal carrier (im == +0: the untuned context's
 * result); the same nu may appear twice with different thresholds.
 * cfg->threshold is not used.
 *
 * Runs.  A carrier context runs ONE capture per run: ookd_rx_process_device,
 * ookd_rx_submit_device / ookd_rx_wait with num_captures == 1, and
 * ookd_rx_process_host.  cfg->max_captures must be 0 or 1; num_captures > 1,
 * ookd_rx_shard_begin and ookd_rx_shard_refine fail with a message;
 * pipeline_chunk_samples is ignored (the run is never pipelined).  One device
 * per context.
 *
 * Results.  Inside, the carriers are the "captures" of a batched run: carrier
 * k's bit words, edges, floats and messages live where capture k's would, with
 * buffers sized for num_carriers captures at create time (a non-zero
 * cfg->edge_capacity or message_capacity is the whole run's, all carriers
 * together, as for a batch).  ookd_message.capture
 * is the carrier index, and ookd_rx_get_bits, _get_edges, _get_fir,
 * _get_fir_sc16q11, _dig_text, _record_dig and _record_fir take the carrier
 * index as `capture`.  stats.total_waves and stats.quiet_waves count
 * (window, carrier) pairs.
 *
 * Forms.  front_form / ookd_front_info.form report OOKD_FRONT_TUNED_MULTI when
 * the fused kernel ran, OOKD_FRONT_TUNED_GENERIC when the shape is not the fused
 * one (decimating or multi-stage filters, more than 256 taps) or with
 * OOKD_RX_EXACT_FIR: then the generic kernel runs once per carrier.  8-bit
 * contexts (OOKD_RX_SAMPLES_CS8 / _CU8) widen the capture ONCE into a staging
 * copy and run either form on it.  With OOKD_RX_TUNED_FIR2 and a filter of two
 * decimate-by-2 stages (<= 16, <= 32 taps), without OOKD_RX_EXACT_FIR, the
 * fused kernel OOKD_FRONT_TUNED_FIR2 runs once per carrier in place of the
 * generic one and 15 is reported; the contract above is unchanged (carrier k is
 * the tuned context created with the flag, bits exactly the contract's, floats
 * within err_valu per component).
 *
 * Fails, with a message: num_carriers == 0 or > OOKD_RX_MAX_CARRIERS,
 * carriers == NULL, a NaN nu, |nu| > 0.5, no filter, non-zero reserved words,
 * cfg->max_captures > 1. */
#define OOKD_RX_MAX_CARRIERS 16
typedef struct ookd_rx_carrier {
    double nu;                      /* cycles per input sample, |nu| <= 0.5; 0 is allowed */
    float threshold;                /* this carrier's rx threshold (cfg->threshold is not used) */
    uint32_t reserved[5];           /* zero                                     */
} ookd_rx_carrier;
ookd_rx *ookd_rx_create_carriers(const ookd_rx_config *cfg, const ookd_filter *filter,
                                 const ookd_device *device,
                                 const ookd_rx_carrier *carriers, uint32_t num_carriers);
uint32_t ookd_rx_num_carriers(const ookd_rx *rx);   /* 0 for every other context */
int ookd_rx_get_carrier(const ookd_rx *rx, uint32_t k, ookd_rx_carrier *out);
/* ookd_rx_get_front_info with carrier k's p_star, band and err_valu */
int ookd_rx_get_carrier_front_info(const ookd_rx *rx, uint32_t k, ookd_front_info *out);
void ookd_rx_destroy(ookd_rx *rx);
/* Bytes per input sample of this context: 4 (SC16Q11) or 2 (CS8 / CU8).  Everywhere below a sample
 * count, stride or halo length counts samples of that size, and a pointer to samples is a pointer
 * to that format: int16 pairs or byte pairs, aligned to 2 bytes at least (16-byte aligned captures
 * take the fast path). */
uint32_t ookd_rx_sample_bytes(const ookd_rx *rx);

/* Demodulate `num_captures` independent captures of `samples_per_capture`
 * SC16Q11 samples each, already resident in HBM at d_iq (int16 I,Q
 * interleaved, capture c at d_iq + 2*c*capture_stride_samples).  Each
 * capture starts from zero FIR history and a reset state machine.  Blocks
 * until results are in host memory. */
int ookd_rx_process_device(ookd_rx *rx, const void *d_iq,
                           uint32_t num_captures,
                           uint64_t samples_per_capture,
                           uint64_t capture_stride_samples);

/* The same split in two, for hosts that overlap captures: submit queues the
 * whole run on the context's stream and returns; wait blocks until its
 * results are in host memory.  One run in flight per context -- use two
 * contexts (each has its own stream) to let the memory-bound front end of
 * one capture overlap the latency-bound state machine of the previous one.
 * ookd_rx_process_device == submit + wait.
 *
 * After a wait that fails (OOKD_ERR_CAPACITY: an edge, message or error list
 * too small for the run) the context is usable: nothing is in flight any more
 * -- a second wait fails with "nothing was submitted" --, the failed run has
 * no results, and the next submit is accepted and decodes as on a context
 * that never failed.  Contexts that share the failed one's gate are not
 * affected.  One context belongs to one host thread at a time; contexts that
 * share a gate may be driven from different host threads. */
int ookd_rx_submit_device(ookd_rx *rx, const void *d_iq,
                          uint32_t num_captures,
                          uint64_t samples_per_capture,
                          uint64_t capture_stride_samples);
int ookd_rx_wait(ookd_rx *rx);

/* Same over a host buffer: stages it to HBM first (PCIe-bound; never the
 * figure bench.py reports).  `iq` holds num_samples samples in the context's
 * format (ookd_rx_sample_bytes each; cast the byte pairs of an 8-bit capture). */
int ookd_rx_process_host(ookd_rx *rx, const int16_t *iq,
                         uint64_t num_samples);

/* One shard of a larger capture (multi-GPU split).
 *   halo / halo_samples : the last input samples of the previous shard
 *       (host pointer, at least ookd_rx_halo_samples(rx) of them), or NULL
 *       for the first shard (zero history); like the capture it is in the
 *       context's sample format, halo_samples counting samples;
 *   last_shard : non-zero => zero pad to a whole buffer; otherwise
 *       num_samples must be a multiple of lcm(spb, total decimation);
 *   runs the front end (FIR, threshold, edges) and ONE speculative state
 *   machine pass from `state_in` (NULL = reset state), leaving the shard's
 *   outgoing state in *state_out.  Call ookd_rx_shard_refine with the true
 *   incoming state (the previous shard's state_out) until no rank's
 *   state_out changes; messages are valid after the last refine. */
int ookd_rx_shard_begin(ookd_rx *rx, const void *d_iq, uint64_t num_samples,
                        const int16_t *halo, uint64_t halo_samples,
                        int last_shard, const ookd_fsm_state *state_in,
                        ookd_fsm_state *state_out);
int ookd_rx_shard_refine(ookd_rx *rx, const ookd_fsm_state *state_in,
                         ookd_fsm_state *state_out);
uint64_t ookd_rx_halo_samples(const ookd_rx *rx);

/* Diagnostic, host only (no GPU): the abstract domain the scan form of the
 * state machine would use for this device at this rate / buffer size.
 * out = { span tables built (0/1), table intervals, intervals that need a
 * simulation, reachable codes (0 = unknown), normal codes that can get
 * "stuck" (an edge on which no trigger fires), table rows holding such a
 * result, domain size, machine states }. */
int ookd_scan_domain_info(const ookd_device *device,
                          uint32_t samples_per_buffer,
                          uint32_t total_decimation, uint32_t out[8]);

/* Results of the last run (host copies, valid until the next run). */
uint64_t ookd_rx_num_messages(const ookd_rx *rx);
const ookd_message *ookd_rx_messages(const ookd_rx *rx);
int ookd_rx_get_stats(const ookd_rx *rx, ookd_rx_stats *out);
int ookd_rx_get_front_info(const ookd_rx *rx, ookd_front_info *out);

/* Parity / recorder taps (device -> host copies of intermediate data):
 *   bits  : 1 bit per decimated sample, LSB-first in 64-bit words, per
 *           capture `ookd_rx_bit_words()` words (ookiedokie.c:171-179);
 *   edges : decimated indices whose bit differs from the previous sample's
 *           (sample -1 counts as 0) -- the content of --rx-rec-dig
 *           (ookiedokie.c:146-169);
 *   fir   : post-filter complexf (needs OOKD_RX_KEEP_FIR). */
uint64_t ookd_rx_bit_words(const ookd_rx *rx);
int ookd_rx_get_bits(const ookd_rx *rx, uint32_t capture, uint64_t *words,
                     uint64_t capacity_words);
int ookd_rx_get_edges(const ookd_rx *rx, uint32_t capture, uint64_t *edges,
                      uint64_t capacity, uint64_t *num_edges);
int ookd_rx_get_fir(const ookd_rx *rx, uint32_t capture, ookd_complexf *out,
                    uint64_t capacity);
/* errors: capture-local decimated indices of the samples on which the state
 *         machine reported an error (device.c:646), in increasing order per
 *         capture.  In a batched run the list is capture-major, EXCEPT when the
 *         scan form refused some captures and those were redone by the round
 *         form (stats.fsm_path 3): then the refused captures' errors follow
 *         those of all the others.  *num is always the total, and every one of
 *         them has its position: the first min(*num, capacity) entries of
 *         `samples` are written, none is ever missing in between.  The lists
 *         are sized at context creation by what the reference can report --
 *         one error per buffer of samples_per_buffer, since the rest of that
 *         buffer is dropped -- for max_samples and max_captures.  Only a
 *         context whose bound exceeds 2^25 positions (a tiny
 *         samples_per_buffer with a huge max_samples) holds fewer; a run of it
 *         with more errors than it holds fails with OOKD_ERR_CAPACITY. */
int ookd_rx_get_errors(const ookd_rx *rx, uint64_t *samples, uint64_t capacity,
                       uint64_t *num);

/* Recorders, by-products of a finished run:
 *   dig : the text of `--rx-rec-dig` (record_dig, ookiedokie.c:146-169) --
 *         "0, <level of sample 0>", then per level change at i the pair
 *         "i-1, <old>" / "i, <new>"; snprintf convention for the in-memory
 *         form (returns the full length);
 *   fir : the post-filter stream as SC16Q11, what `--rx-rec` writes when
 *         rx_rec_input is false (ookiedokie.c:265-270 through
 *         complexf_to_sc16q11, complexf.h:87-96); needs OOKD_RX_KEEP_FIR.
 *         (With rx_rec_input the recording is the input capture itself.) */
size_t ookd_rx_dig_text(const ookd_rx *rx, uint32_t capture, char *out, size_t capacity);
int ookd_rx_record_dig(const ookd_rx *rx, uint32_t capture, const char *path);
int ookd_rx_get_fir_sc16q11(const ookd_rx *rx, uint32_t capture, int16_t *out,
                            uint64_t capacity_samples);
int ookd_rx_record_fir(const ookd_rx *rx, uint32_t capture, const char *path);

/* ------------------------------------------------------------------------
 * Envelope survey: which threshold does this capture want?  One pass over
 * captures resident in HBM counts the post-filter power -- the quantity the
 * slicer compares, complexf_power (src/complexf.h:43-46) of the output of
 * fir_filter_and_decimate (src/fir.c:355-395) -- into a histogram per
 * capture; ookd_suggest_threshold (host only) turns a histogram into a value
 * for ookd_rx_config.threshold.  A separate object beside the rx context:
 * nothing an ookd_rx does changes.
 *
 * Arithmetic: unpack and filter are the reference's, bit for bit (taps newest
 * first, separate multiply and add, stages chained as fir.c chains them: what
 * OOKD_RX_EXACT_FIR computes), so a histogram is an exact integer function of
 * the capture.
 * Bins: four per octave of power (0.75 dB of amplitude on average), cut from
 * the float's own bits -- exponent and the two leading mantissa bits --,
 *     b = clamp((bits(p) >> 21) - ((127 - 40) << 2) + 1, 0, 255):
 * bin 0 holds everything below 2^-40 (zeros and denormals included), bin
 * b >= 1 starts at power 2^(-40 + (b - 1) div 4) * (1 + ((b - 1) mod 4) / 4),
 * i.e. at 1, 1.25, 1.5 and 1.75 times each power of two, bin 255 holds
 * everything from 1.5 * 2^23 up (inf, NaN and anything with the sign bit set
 * included; a power is never negative).
 * Counted: per capture the first floor(n / D) filter outputs from zero
 * history, n = samples in the capture, D = total decimation; with no filter
 * the samples themselves.  No zero padding is counted (an rx context pads a
 * capture to whole buffers; that is buffering, not signal).
 * ---------------------------------------------------------------------- */
#define OOKD_LEVEL_BINS 256
typedef struct ookd_level_hist {
    uint64_t samples;               /* floor(n / D) = the sum of bins[]       */
    uint64_t bins[OOKD_LEVEL_BINS];
} ookd_level_hist;

typedef struct ookd_survey ookd_survey;

/* filter may be NULL (no filter).  sample_flags: 0 (SC16Q11), OOKD_RX_SAMPLES_CS8
 * or OOKD_RX_SAMPLES_CU8 (read in place, 2 bytes per sample); both, or any
 * other bit, fails.  stream: hipStream_t to launch on, NULL = own. */
ookd_survey *ookd_survey_create(int32_t hip_device, const ookd_filter *filter,
                                uint32_t sample_flags, uint32_t max_captures,
                                void *stream);
void ookd_survey_destroy(ookd_survey *s);
/* Survey `num_captures` (<= max_captures) captures of `samples_per_capture`
 * samples each, resident in HBM, capture c at sample c * capture_stride_samples
 * of d_iq (samples of the survey's format, as ookd_rx_process_device takes
 * them).  Blocks until the histograms are in host memory; they replace those
 * of the run before.  0 samples is a valid (empty) survey. */
int ookd_survey_device(ookd_survey *s, const void *d_iq, uint32_t num_captures,
                       uint64_t samples_per_capture, uint64_t capture_stride_samples);
/* Same over one host capture: staged to HBM first (PCIe-bound). */
int ookd_survey_host(ookd_survey *s, const void *iq, uint64_t num_samples);
int ookd_survey_get_hist(const ookd_survey *s, uint32_t capture, ookd_level_hist *out);
/* HIP-event time of the last run's histogram kernel (0 before any run). */
float ookd_survey_kernel_ms(const ookd_survey *s);

/* Tuned survey: the threshold for a carrier that is NOT at 0 Hz.  The survey
 * above filters with the real taps around 0 Hz; on a capture whose carrier sits
 * beside the centre it measures the receiver's DC term.  A tuned survey counts
 * what a context made by ookd_rx_create_tuned with the same nu slices.
 *
 * The contract: the histogram is the one defined above with the filter output
 * replaced by the tuned contract's (at ookd_filter_tuned_taps):
 *   - the taps of stage s are ookd_filter_tuned_taps(f, nu, s, re, im);
 *   - each stage output is the four unfused float32 statements per tap, in the
 *     order stated there, tap 0 on the newest sample, accumulators from +0;
 *     stages chain and decimate from zero history;
 *   - p = ar*ar + ai*ai: two products and a sum, each rounded;
 *   - the bin rule is unchanged;
 *   - per capture the first floor(n / D) outputs are counted; nothing is padded
 *     and no input at or beyond n is read.
 * It stays an exact integer function of the capture: no guard band, no fused
 * multiply-add, no matrix cores (an output one ulp off falls into the
 * neighbouring bin).  x - y is x + (-y) bit for bit, so an implementation may
 * hold -im; what matters is the order of the roundings per component: ar gets
 * re*xr first and im*xi second, ai gets re*xi first and im*xr second.
 *
 * flags: the sample-format bits as ookd_survey_create takes them, plus
 * OOKD_RX_EXACT_FIR; any other bit fails.  tune == NULL or nu == 0 IS
 * ookd_survey_create: same kernel, form OOKD_SURVEY_GENERIC, OOKD_RX_EXACT_FIR
 * accepted and ignored.  Otherwise a run takes one of two forms with the same
 * histogram: OOKD_SURVEY_TUNED_FIR1 for 1 stage, decimation 1 and <= 256 taps,
 * OOKD_SURVEY_TUNED_GENERIC for every other shape -- and for every shape with
 * OOKD_RX_EXACT_FIR, which exists so that the two can be run against each other
 * (as the flag does on a tuned rx context).  Fails for NaN, |nu| > 0.5,
 * non-zero ookd_tune.reserved, and nu != 0 without a filter; the argument
 * checks come before any HIP call.
 * 8-bit captures are read in place by all forms (nothing is widened first).
 * Alignment: OOKD_SURVEY_TUNED_FIR1 reads a capture whose first sample lies on
 * a 16-byte boundary with 16-byte loads; any other capture of a batch (an odd
 * stride, an 8-bit capture at an odd sample) is read sample by sample BY THE
 * SAME KERNEL: the form stays OOKD_SURVEY_TUNED_FIR1 and the histogram is the
 * same.
 * ookd_survey_destroy / _device / _host / _get_hist / _kernel_ms and
 * ookd_suggest_threshold serve both kinds of survey. */
enum {
    OOKD_SURVEY_GENERIC = 1,        /* survey_kernel: what ookd_survey_create runs       */
    OOKD_SURVEY_TUNED_GENERIC = 2,  /* any shape, the tuned contract's order throughout  */
    OOKD_SURVEY_TUNED_FIR1 = 3      /* 1 stage, decimation 1, <= 256 taps: register-blocked */
};
ookd_survey *ookd_survey_create_tuned(int32_t hip_device, const ookd_filter *filter,
                                      uint32_t flags, uint32_t max_captures,
                                      void *stream, const ookd_tune *tune);
double ookd_survey_tune(const ookd_survey *s);     /* 0 for an untuned one, 0 for NULL */
uint32_t ookd_survey_form(const ookd_survey *s);   /* the form a run takes / took; 0 for NULL */

/* Carriers survey: the tuned survey of several carriers in ONE pass over the
 * captures, counting every stride-th output.  The threshold rule does not need
 * every power: the envelope behind a channel filter moves over hundreds of
 * samples, so a histogram of every 8th or 64th output shows the same two levels
 * at an 8th or a 64th of the arithmetic.
 *
 * The contract: carrier k's histogram of capture c is the histogram of
 * ookd_survey_create_tuned(..., {tunes[k].nu}) on that capture, RESTRICTED TO
 * THE OUTPUTS WITH INDEX i = 0 (mod stride), i < floor(n / D).
 *   - the tap rule, the four unfused statements per tap, p = ar*ar + ai*ai with
 *     its three roundings, the bin rule, zero history, nothing padded and no
 *     input at or beyond n read: all unchanged;
 *   - ookd_level_hist.samples = ceil(floor(n / D) / stride) = the sum of bins[];
 *   - at stride 1 it is that survey's histogram, bin for bin;
 *   - nu = 0 is a legal carrier (im = +0: the untuned survey's counts, as for
 *     ookd_rx_create_carriers), and the same nu may appear twice.
 * It stays an exact integer function of the capture: the same contract over a
 * subset of the outputs.  ookd_suggest_threshold applies OOKD_LEVEL_MIN_SIDE to
 * COUNTS: see there for what that means at a stride.
 *
 * Forms.  OOKD_SURVEY_TUNED_MULTI for 1 stage, decimation 1 and <= 256 taps,
 * without OOKD_RX_EXACT_FIR: one launch for all carriers and captures; 8-bit
 * captures are read in place; a capture whose first sample is not on a 16-byte
 * boundary is read sample by sample by the same kernel and the form stays
 * OOKD_SURVEY_TUNED_MULTI (the rule of OOKD_SURVEY_TUNED_FIR1).  Any other
 * shape, or OOKD_RX_EXACT_FIR, at stride 1: the OOKD_SURVEY_TUNED_GENERIC path
 * once per carrier, and that form is reported -- the cross-check partner at
 * stride 1.  stride > 1 on those shapes or with the flag fails at create time.
 *
 * OOKD_SURVEY_TUNED_MULTI_FIR2, on request: with OOKD_RX_TUNED_FIR2 in `flags`
 * (the flag of the rx contexts) a filter of two decimate-by-2 stages of <= 16
 * and <= 32 taps -- the backend default fs128_fs16_dec4 -- without
 * OOKD_RX_EXACT_FIR is surveyed in one launch for all carriers and captures,
 * at every stride.  Nothing new is defined: it is the contract above with
 * D = 4, written out for this shape:
 *   - the taps are ookd_filter_tuned_taps(f, nu_k, s, ...) for s = 0, 1; each
 *     tap is the four unfused float32 statements, tap 0 on the newest sample,
 *     the accumulators from +0;
 *   - stage 0 output j sits on input 2 j + 1, stage 1 output i on stage-0
 *     output 2 i + 1; the history is zero: inputs and stage-0 outputs with a
 *     negative index are +0;
 *   - only outputs i = 0 (mod stride), i < floor(n / 4), are counted, and
 *     samples = ceil(floor(n / 4) / stride);
 *   - no fused multiply-add, no guard band, no matrix core, no shortcut for
 *     im == 0: a stage-0 output of inf times a stage-1 tap of +-0 is NaN here
 *     as in the contract.
 * All three sample formats are read in place; a capture whose first sample is
 * not on a 16-byte boundary is read sample by sample by the same kernel and the
 * form stays OOKD_SURVEY_TUNED_MULTI_FIR2.  The stride saves less here than on
 * a single stage: counted outputs are 2 S stage-0 outputs apart and stage 1
 * spans up to 32 of them, so up to stride 16 every stage-0 output is still
 * needed and only stage 1 thins; from 32 on stage 0 thins too.  On every other shape and together with OOKD_RX_EXACT_FIR the
 * flag is accepted and has no effect: the forms and refusals of the paragraph
 * above.  Without the flag nothing changes.
 *
 * Fails, before any HIP call, for: num_carriers 0 or > OOKD_SURVEY_MAX_CARRIERS,
 * tunes == NULL, a NaN nu or |nu| > 0.5, non-zero ookd_tune.reserved, no
 * filter, a stride that is not a power of two in 1 .. OOKD_SURVEY_MAX_STRIDE,
 * flag bits other than the sample-format bits, OOKD_RX_EXACT_FIR and
 * OOKD_RX_TUNED_FIR2, both format bits, max_captures == 0.
 *
 * ookd_survey_device / _host / _kernel_ms / _form / _destroy and
 * ookd_suggest_threshold serve this kind too.  ookd_survey_get_hist returns
 * carrier 0, ookd_survey_tune carrier 0's nu. */
#define OOKD_SURVEY_MAX_CARRIERS 16
#define OOKD_SURVEY_MAX_STRIDE   64
enum { OOKD_SURVEY_TUNED_MULTI = 4 };   /* several carriers, every stride-th output, one launch */
enum { OOKD_SURVEY_TUNED_MULTI_FIR2 = 5 };  /* ... through 2 x decimate-by-2, with OOKD_RX_TUNED_FIR2 */
ookd_survey *ookd_survey_create_carriers(int32_t hip_device, const ookd_filter *filter,
                                         uint32_t flags, uint32_t max_captures, void *stream,
                                         const ookd_tune *tunes, uint32_t num_carriers,
                                         uint32_t stride);
uint32_t ookd_survey_num_carriers(const ookd_survey *s);   /* 0 for the other two kinds, 0 for NULL */
uint32_t ookd_survey_stride(const ookd_survey *s);         /* 1 for the other two kinds, 0 for NULL */
int ookd_survey_get_carrier_hist(const ookd_survey *s, uint32_t capture, uint32_t carrier,
                                 ookd_level_hist *out);

/* The bin rule above and its inverse, pure host code (no GPU needed).
 * ookd_level_bin_lower: the power at which bin `bin` starts (0 for bin 0;
 * bins beyond 255 continue the series: 256 gives the upper edge of the
 * geometric cell that stands for bin 255). */
uint32_t ookd_level_bin(float power);
float ookd_level_bin_lower(uint32_t bin);

/* Suggested threshold.  The rule, a contract:
 *   1. Split.  Over the BIN INDEX (the log domain) find the k in 0..254 with both
 *      sides non-empty -- "off" = bins 0..k, "on" = bins k+1..255 -- that
 *      maximises Otsu's between-class variance
 *          (n * sum_{i<=k} i h[i]  -  a * sum_i i h[i])^2 / (a * (n - a)),
 *      a = sum_{i<=k} h[i], n = sum_i h[i], compared in exact integer
 *      arithmetic.  Several k with the same maximum: the split is
 *      (first + last) / 2 of them, rounded down.
 *   2. Levels.  off_bin / on_bin are the median bins of the two sides: the
 *      first bin at which the side's running count reaches (count + 1) / 2.
 *      The amplitude of bin b is the fourth root of the product of its two
 *      power edges, (lower(b) * lower(b + 1))^(1/4); off_level is 0 when
 *      off_bin is 0.
 *   3. threshold = (off_level + on_level) / 2, the amplitude midpoint: the
 *      slicer level that moves the two flanks of a pulse by the same amount
 *      on a symmetric filter ramp, so pulse widths are distorted least.  (The
 *      split of step 1 itself is NOT a usable threshold: in the log domain it
 *      sits some 15 dB under the on level, inside the noise's skirt.)
 *   4. found = 1 only if on_bin - off_bin >= OOKD_LEVEL_MIN_SEPARATION and
 *      both sides hold at least OOKD_LEVEL_MIN_SIDE samples; otherwise 0
 *      (noise only, empty, silence, or always on) and threshold is 0 -- the
 *      other members still say what was seen.  No split at all (fewer than
 *      two occupied bins): everything 0 but the bin of the one level in
 *      off_bin = on_bin.
 * OOKD_LEVEL_MIN_SEPARATION, 18 bins = 13.5 dB: measured on the golden
 * captures through fs32_fs4 with +-40 LSB of uniform noise, noise alone
 * splits into halves whose medians lie 11..12 bins apart whatever its level
 * (+-5 .. +-1000 LSB: 10..11), while the quietest capture that still decodes
 * (1/16 of nominal level) shows 26; 18 leaves 6 bins to the one and 8 to the
 * other.
 * OOKD_LEVEL_MIN_SIDE, 512 samples: a level held for less is a transient --
 * the start-up ramp of a carrier that is always on (11 outputs through
 * fs32_fs4, at most the tap count) --, while one message holds thousands.
 * The rule is applied to COUNTS: on a histogram of a carriers survey with
 * stride S (ookd_survey_create_carriers) a level must be held for 512 * S
 * outputs in total to count as a level.
 * Limits: two levels only (the strongest of several transmitters sets the on
 * level); a capture of tiny integer noise without a filter has a share of
 * samples exactly zero (bin 0) far from the rest and reads as two levels. */
#define OOKD_LEVEL_MIN_SEPARATION 18
#define OOKD_LEVEL_MIN_SIDE 512
typedef struct ookd_threshold_suggestion {
    int found;                      /* 0: no two levels                        */
    float threshold;                /* amplitude: ookd_rx_config.threshold     */
    float off_level, on_level;      /* amplitudes of the two levels            */
    uint32_t split_bin, off_bin, on_bin;    /* split_bin: the k of step 1      */
    double on_fraction;             /* share of samples above the split        */
} ookd_threshold_suggestion;
/* 0, or OOKD_ERR_ARG for a NULL argument.  n is the sum of h->bins; h->samples is not read. */
int ookd_suggest_threshold(const ookd_level_hist *h, ookd_threshold_suggestion *out);

/* ------------------------------------------------------------------------
 * Carrier survey: which ookd_tune.nu does this capture want?  One pass over
 * captures resident in HBM sums a Welch power spectrum per capture;
 * ookd_suggest_carriers (host only) turns a spectrum into a list of carriers.
 * A separate object beside the rx context and the envelope survey: nothing an
 * ookd_rx or an ookd_survey does changes.
 *
 * The spectrum, a contract:
 *   - frame f of a capture is samples [1024 f, 1024 f + 1024); only whole
 *     frames count, nothing is padded (as in the envelope survey);
 *   - samples are unpacked as the reference unpacks them, v / 2048
 *     (complexf.h:68-77; an 8-bit sample is 16 v first);
 *   - the window is the periodic Hann w[n] = 0.5 - 0.5 cos(2 pi n / 1024);
 *   - X_f[k] = sum_n w[n] x[1024 f + n] e^{-j 2 pi k n / 1024};
 *   - power[k] = sum_f |X_f[k]|^2, k = 0 .. 1023 in FFT order;
 *   - bin k is the carrier at ookd_spectrum_bin_nu(k) cycles per input sample,
 *     the sign convention of ookd_tune.nu: a capture moved to +600 kHz at
 *     3 MHz peaks at bin 205.
 * Arithmetic is fp32 inside a frame and double across frames, so the contract
 * is an error bound, not bit equality.  With S[k] the value in exact (float64)
 * arithmetic and E = sum_k S[k]:
 *     |power[k] - S[k]| <= 2 EPS sqrt(S[k] E) + EPS^2 E + EPS S[k],
 *     EPS = OOKD_SPECTRUM_EPS = 12 log2(1024) 2^-24.
 * Derivation.  Higham's normwise bound for an FFT is
 * ||X^ - X||_2 <= log2(N) eta ||X||_2; with twiddles rounded from double
 * eta ~ 8 u (u = 2^-24), and another 4 u per level, taken as log2(N) 4 u,
 * covers the rounding of the window product: the factor 12.  A single bin's
 * error is bounded by the norm, |X^_f[k] - X_f[k]| <= EPS ||X_f||_2, so
 * | |X^_f[k]|^2 - |X_f[k]|^2 | <= 2 EPS |X_f[k]| ||X_f|| + EPS^2 ||X_f||^2, and
 * Cauchy-Schwarz over the frames gives the first two terms.  The third is the
 * budget for re^2 + im^2 and for adding per-frame powers in fp32 before they
 * are folded into a double: 120 u allows a lane to sum at most 32 frames in
 * fp32 between folds.
 * Results are reproducible: two runs of one context over the same capture give
 * bitwise identical power[] (no floating-point atomics: every workgroup writes
 * its partial sums and a second kernel adds them in a fixed order).
 * ---------------------------------------------------------------------- */
#define OOKD_SPECTRUM_BINS 1024
#define OOKD_SPECTRUM_EPS (12.0 * 10.0 / 16777216.0)   /* 12 * log2(1024) * 2^-24 */
typedef struct ookd_spectrum_result {
    uint64_t frames;                       /* floor(n / 1024) whole frames summed */
    double power[OOKD_SPECTRUM_BINS];      /* sum over frames of |X_f[k]|^2, FFT order */
} ookd_spectrum_result;

typedef struct ookd_spectrum ookd_spectrum;

/* sample_flags: 0 (SC16Q11), OOKD_RX_SAMPLES_CS8 or OOKD_RX_SAMPLES_CU8 (read in
 * place, 2 bytes per sample); both, or any other bit, fails.  stream:
 * hipStream_t to launch on, NULL = own. */
ookd_spectrum *ookd_spectrum_create(int32_t hip_device, uint32_t sample_flags,
                                    uint32_t max_captures, void *stream);
void ookd_spectrum_destroy(ookd_spectrum *s);
/* Captures are addressed as ookd_rx_process_device addresses them: capture c at
 * sample c * capture_stride_samples of d_iq.  Blocks until the spectra are in
 * host memory; they replace those of the run before.  Fewer than 1024 samples
 * (0 included) is a valid run with frames = 0 and all-zero power.  Captures
 * that start on 16-byte boundaries are read with vector loads, others sample
 * by sample. */
int ookd_spectrum_device(ookd_spectrum *s, const void *d_iq, uint32_t num_captures,
                         uint64_t samples_per_capture, uint64_t capture_stride_samples);
/* Same over one host capture: staged to HBM first (PCIe-bound), in a buffer
 * the context keeps and grows to the largest capture it has seen. */
int ookd_spectrum_host(ookd_spectrum *s, const void *iq, uint64_t num_samples);
int ookd_spectrum_get(const ookd_spectrum *s, uint32_t capture, ookd_spectrum_result *out);
/* HIP-event time of the last run's two kernels (0 before any run). */
float ookd_spectrum_kernel_ms(const ookd_spectrum *s);
/* k / 1024 for k < 512, (k - 1024) / 1024 otherwise (k taken mod 1024); host only. */
double ookd_spectrum_bin_nu(uint32_t bin);

/* Suggested carriers, pure host code (no GPU needed).  The rule, a contract:
 *   1. floor = the median of the 1024 powers: the mean of the 512th and 513th
 *      smallest.
 *   2. frames == 0: no carriers.
 *   3. All bins start live.
 *   4. Repeat: take the live bin of largest power, ties going to the lowest k.
 *      Stop when that power is not > 0, is < min_ratio * floor, or `capacity`
 *      carriers have been emitted.  Otherwise emit it and kill every bin within
 *      circular distance <= min_spacing_bins of it (1023 and 0 are neighbours).
 *   5. Output is in decreasing power.  nu is the bin centre, not interpolated:
 *      decoding the golden captures at one bin either side of the true offset
 *      gives the same messages, 1/1024 is far inside the filters' pass band.
 *   6. at_dc (|bin| <= 1) is only a flag: the receiver's own DC term, or a
 *      carrier at 0 Hz.  The caller decides what to do with that peak.
 * OOKD_CARRIER_MIN_RATIO, 64: a bin of one frame of white noise is
 * exponentially distributed, P(S > r median) = 2^-r, so 64 leaves 1024 * 2^-64
 * false peaks per frame; more frames only thin the tail (worst max / median of
 * noise alone over 50 trials: 15.6 with one frame, 5.0 with four, 1.5 with 100).
 * OOKD_CARRIER_MIN_SPACING, 32 bins = 1/32 cycle per sample: the pass band of
 * fs32_fs4 and of the backend's default filter.  Two carriers closer than that
 * cannot be separated by those filters anyway, and the sidebands of the on-off
 * keying fall inside it and are not reported as carriers.
 * Limits: with floor == 0 (a noiseless synthetic capture) rounding residue can
 * qualify as a peak (its ratio is infinite), and a carrier within 32 bins of a
 * stronger DC term is hidden by it. */
typedef struct ookd_carrier {
    double nu;          /* bin centre, cycles per input sample: pass to ookd_tune.nu */
    int32_t bin;        /* -512 .. 511 */
    uint32_t at_dc;     /* |bin| <= 1: the receiver's own DC term, or a carrier at 0 Hz */
    double power;       /* power[k] */
    double ratio;       /* power / floor */
} ookd_carrier;
#define OOKD_CARRIER_MIN_RATIO 64.0
#define OOKD_CARRIER_MIN_SPACING 32
/* 0, or OOKD_ERR_ARG for NULL sp or count, NULL out with capacity > 0, or a
 * negative or NaN min_ratio.  min_ratio 0 / min_spacing_bins 0 = the defaults
 * above.  *count receives the number of carriers written to out[]; floor may
 * be NULL. */
int ookd_suggest_carriers(const ookd_spectrum_result *sp, double min_ratio /* 0 = default */,
                          uint32_t min_spacing_bins /* 0 = default */,
                          ookd_carrier *out, uint32_t capacity, uint32_t *count, double *floor);

/* ------------------------------------------------------------------------
 * Pulse survey: which timings does this capture want?  The slicer's output,
 * the sorted edge list of every capture (or carrier) of a run, stays in HBM
 * after the run; one pass over it counts how long the "on" runs and the "off"
 * runs are into a histogram per capture and level; ookd_suggest_pulses (host
 * only) groups a histogram into the few timing classes a device file names
 * (devices/README.md: the pulse and gap durations of its states).  A by-product
 * of a finished run like the recorders: nothing a run does changes, and a run
 * nobody asks about launches and allocates nothing for it.
 *
 * Runs, a contract.  For capture (or carrier) c of the last run take its edge
 * list e[0..E) as ookd_rx_get_edges returns it and n_out =
 * stats.decimated_samples.  Closed run i, 0 <= i < E - 1, has length
 * e[i+1] - e[i] and level 1 ("on") when i is even, 0 ("off") otherwise: sample
 * -1 counts as 0, so the first edge rises.  The two open runs are not counted
 * in the bins:
 *     open_head  = e[0], or n_out when E = 0; its level is 0;
 *     open_tail  = n_out - e[E-1], or 0 when E = 0;
 *     tail_level = E & 1.
 * The zero padding to whole buffers is part of the edge list (a capture that
 * ends high falls at the first padded sample); the histogram is a function of
 * that list and n_out and of nothing else, whatever filter, tuning, sample
 * format or device the context has.
 *
 * Bins, all integer.  OOKD_PULSE_BINS = 512.  A length d of 1 .. 31 goes to bin
 * d (bin 0 stays empty); for d >= 32, with o = floor(log2 d), to
 *     32 + 16 (o - 5) + ((d >> (o - 4)) & 15),  clamped to 511:
 * sixteen bins per octave, none wider than 6.25 % of its lower edge, d < 2^35
 * covered before the clamp.  ookd_pulse_bin_lower(b) = b for b < 32, otherwise
 * (16 + (b - 32) % 16) << (1 + (b - 32) / 16); 512 and beyond continue the
 * series (512 gives 2^35, the upper edge of what bin 511 holds before the
 * clamp), saturating at UINT64_MAX.  Example: 1503 goes to bin 119 = [1472, 1536).
 *
 * The histogram is an exact integer function of the edge list, the same
 * whatever order the kernel's atomic adds land in.  It is computed for ALL
 * captures (carriers) of the run by one kernel launch at the first
 * ookd_rx_pulse_hist after the run, on the context's stream, and answered from
 * host memory until the next run; its buffers are allocated by the first call
 * in the life of the context.  Contexts without a device, batched runs and
 * carrier contexts (capture = carrier index) all work.
 * Returns OOKD_ERR_ARG for a NULL argument, capture >= the run's captures, no
 * finished run (none yet, one submitted and not waited for, or one that failed
 * before its edges were counted), and -- with a
 * message naming the case -- for a pipelined run (stats.pipeline_chunks != 0:
 * its lists are chunk-local) and for a shard run (ookd_rx_shard_begin: the level
 * in front of the shard is unknown); OOKD_ERR_CAPACITY when the run's edge list
 * overflowed.
 * ---------------------------------------------------------------------- */
#define OOKD_PULSE_BINS 512
typedef struct ookd_pulse_hist {
    uint64_t num_edges, samples;            /* E, n_out                              */
    uint64_t runs[2];                       /* closed runs per level = sum of count  */
    uint64_t count[2][OOKD_PULSE_BINS];     /* [level][bin]                          */
    uint64_t sum[2][OOKD_PULSE_BINS];       /* sum of the lengths counted there      */
    uint64_t open_head, open_tail;
    uint32_t tail_level, reserved;
} ookd_pulse_hist;
int ookd_rx_pulse_hist(ookd_rx *rx, uint32_t capture, ookd_pulse_hist *out);
/* HIP-event time of the pass that computed the last run's histograms: the
 * zeroing of the result and the kernel.  0 while nobody has asked about the
 * last run (also when the call was refused, or the run had no samples). */
float ookd_rx_pulse_kernel_ms(const ookd_rx *rx);

/* The bin rule above and its inverse, pure host code (no GPU needed).
 * ookd_pulse_bin(0) is 0. */
uint32_t ookd_pulse_bin(uint64_t length);
uint64_t ookd_pulse_bin_lower(uint32_t bin);

/* Timing classes, pure host code.  The rule, a contract, per level:
 *   1. Walk the bins upwards.  A class is a maximal group of occupied bins in
 *      which two successive occupied bins lie fewer than OOKD_PULSE_CLASS_GAP
 *      bins apart (their indices differ by less than it: with 2, occupied bins
 *      join a class only when they are adjacent).
 *   2. A class reports first_bin and last_bin (its lowest and highest occupied
 *      bin), runs = the sum of its counts, mean = (sum of its sums) / runs as a
 *      double, lower = ookd_pulse_bin_lower(first_bin), upper =
 *      ookd_pulse_bin_lower(last_bin + 1) - 1 (NOT a bound for a class that ends
 *      in bin 511: that bin also holds every clamped longer run, and upper
 *      then reads 2^35 - 1 while mean may lie above it), and mean_us / lower_us / upper_us
 *      = x / sample_rate * 1e6, or 0 when sample_rate <= 0 (or NaN).
 *      sample_rate is the rate of the DECIMATED samples (what ookd_device_load
 *      takes).
 *   3. At most OOKD_PULSE_MAX_CLASSES classes are reported per level, in
 *      ascending order of length.  If there are more, those with the most runs
 *      are kept -- on a tie the shorter class wins -- and dropped_runs[level]
 *      counts the runs of the rest.
 *   4. found = 1 when each level has a class of at least 2 runs.
 * Only count[][] and sum[][] of the histogram are read.
 * OOKD_PULSE_CLASS_GAP, 2 bins: measured on the golden captures (threshold 0.1,
 * clean and with +-40 LSB of noise, through fs32_fs4 and fs128_fs16_dec4), the
 * narrowest separation between two real timings is 11997 against 13197 samples
 * (unknown-remote1's off-runs): bins 167 and 169, two bins apart with one empty
 * bin between them, which a gap of 2 keeps apart; while one timing that
 * straddles a bin edge -- the same capture's on-runs through fs128_fs16_dec4,
 * 415 and 416 samples -- lands in two ADJACENT bins, which a gap of 2 merges (a
 * gap of 1 would not, a gap of 3 would merge the two real timings).
 * Limits: the rule knows nothing about coding (which class is a sync, a one or
 * a zero is for the author of the device file); one-sample glitches show up as
 * classes of their own (bin 1); timings closer together than two bins (6 to
 * 12 % apart, depending on where the bin edges fall) merge into one class; only
 * two levels exist. */
#define OOKD_PULSE_CLASS_GAP 2
#define OOKD_PULSE_MAX_CLASSES 16
typedef struct ookd_pulse_class {
    uint32_t first_bin, last_bin;
    uint64_t runs;
    double mean;                    /* samples                                 */
    uint64_t lower, upper;          /* samples: the range its bins cover       */
    double mean_us, lower_us, upper_us;
} ookd_pulse_class;
typedef struct ookd_pulse_suggestion {
    int found;                      /* 1: each level has a class of >= 2 runs  */
    uint32_t reserved;
    uint32_t num_classes[2];        /* [level]: 0 = off-runs, 1 = on-runs      */
    uint64_t dropped_runs[2];
    ookd_pulse_class classes[2][OOKD_PULSE_MAX_CLASSES];
} ookd_pulse_suggestion;
/* 0, or OOKD_ERR_ARG for a NULL argument. */
int ookd_suggest_pulses(const ookd_pulse_hist *h, double sample_rate, ookd_pulse_suggestion *out);

/* ------------------------------------------------------------------------
 * Symbol survey: which device does this capture want?  The timing classes above
 * name the pulse and gap lengths; what is still missing for a device file is the
 * coding: which (pulse, gap) pair is a sync, which a zero, which a one, and how
 * many bits lie between two syncs.  One more pass over the edge list that a run
 * leaves in HBM counts pulse/gap SYMBOLS and measures the distance between sync
 * symbols; two host-only rules (ookd_suggest_coding, ookd_suggest_device) turn
 * the counts into a device of the family both device files of the reference
 * belong to: a sync pulse and a sync gap, then num_bits bits, each a fixed pulse
 * followed by a short or a long gap, then a closing pulse.  The decoder runs the
 * suggested device like any other.  A by-product of a finished run: nothing a
 * run does changes, and a run nobody asks about launches and allocates nothing.
 *
 * Symbols, a contract.  Take capture (or carrier) c of the last run, its edge
 * list e[0..E) and the closed runs of the pulse survey's contract (run i is "on"
 * when i is even).  Symbol j, 0 <= j < S = (E - 1) / 2 (integer division; 0
 * when E < 3), is the pair (on-run 2j, off-run 2j + 1); both runs are closed.
 * Indices are relative to the capture's own list.
 *
 * Classes.  ookd_symbol_table holds per level (0 = off-runs, 1 = on-runs, as in
 * ookd_pulse_suggestion) num_classes[level] <= 16 inclusive ranges
 * lower[level][k] <= d <= upper[level][k], ascending and disjoint
 * (lower[k] <= upper[k] < lower[k+1]).  A run length inside no range has class
 * 16 ("none", OOKD_SYMBOL_NONE).  ookd_symbol_table_from_pulses copies the
 * classes' lower / upper: a class that ends in bin 511 keeps upper = 2^35 - 1,
 * so longer runs get class 16.  A table that is not ascending and disjoint, or
 * has more than 16 classes on a level, is OOKD_ERR_ARG.
 *
 * Kinds.  kind(j) = (on class, off class) lies in [0,16]^2; kinds[on][off]
 * counts the symbols of every kind.
 *
 * Roles and frames.  ookd_symbol_roles gives every kind a role, role[on][off],
 * one byte: OOKD_ROLE_OTHER 0, _SYNC 1, _ZERO 2, _ONE 3 (a larger value is
 * OOKD_ERR_ARG).  Let p_0 < ... < p_{m-1} be the symbols whose kind has role
 * SYNC.  Then
 *     num_syncs    = m;
 *     head_symbols = p_0, or S when m = 0;
 *     tail_symbols = S - p_{m-1}, or 0 when m = 0;
 *     frame i, 0 <= i < m - 1, has distance D_i = p_{i+1} - p_i and is CLEAN
 *     when every symbol p_i + 1 ... p_{i+1} - 2 has role ZERO or ONE: the symbol
 *     just before the next sync is free, because its off-run is the pause between
 *     two messages; an empty interior (D <= 2) is clean;
 *     frames[clean][min(D_i, 511)] is incremented (OOKD_FRAME_BINS = 512).
 * With roles == NULL only num_symbols and kinds are computed; the frame members
 * are zero.  Everything is an exact integer function of the edge list, the table
 * and the roles, the same whatever order the kernels' atomic adds land in.
 *
 * ookd_rx_symbol_survey computes this on the GPU for the ONE capture asked
 * about, at every call (table and roles differ from call to call: nothing is
 * cached), on the context's stream; its buffers are allocated by the first call
 * in the life of the context.  It refuses what ookd_rx_pulse_hist refuses, with
 * the same codes: OOKD_ERR_ARG for a NULL rx, table or out, capture >= the run's
 * captures, no finished run, a pipelined run, a shard run; OOKD_ERR_CAPACITY for
 * an overflowed edge list; and OOKD_ERR_ARG for a bad table or role.
 * ---------------------------------------------------------------------- */
#define OOKD_SYMBOL_MAX_CLASSES 16
#define OOKD_SYMBOL_NONE 16             /* the class of a length inside no range  */
#define OOKD_SYMBOL_KINDS 17            /* classes 0 .. 15 and "none", per level  */
#define OOKD_FRAME_BINS 512
enum { OOKD_ROLE_OTHER = 0, OOKD_ROLE_SYNC = 1, OOKD_ROLE_ZERO = 2, OOKD_ROLE_ONE = 3 };
typedef struct ookd_symbol_table {
    uint32_t num_classes[2];                            /* [level]: 0 = off, 1 = on */
    uint64_t lower[2][OOKD_SYMBOL_MAX_CLASSES];
    uint64_t upper[2][OOKD_SYMBOL_MAX_CLASSES];
} ookd_symbol_table;
typedef struct ookd_symbol_roles {
    uint8_t role[OOKD_SYMBOL_KINDS][OOKD_SYMBOL_KINDS]; /* [on class][off class]   */
    uint8_t reserved[7];
} ookd_symbol_roles;
typedef struct ookd_symbol_survey {
    uint64_t num_symbols;                               /* S                        */
    uint64_t kinds[OOKD_SYMBOL_KINDS][OOKD_SYMBOL_KINDS];   /* [on class][off class] */
    uint64_t num_syncs, head_symbols, tail_symbols;
    uint64_t frames[2][OOKD_FRAME_BINS];                /* [clean][min(D, 511)]     */
} ookd_symbol_survey;
/* 0, or OOKD_ERR_ARG for a NULL argument.  Pure host code. */
int ookd_symbol_table_from_pulses(const ookd_pulse_suggestion *pulses, ookd_symbol_table *out);
int ookd_rx_symbol_survey(ookd_rx *rx, uint32_t capture, const ookd_symbol_table *table,
                          const ookd_symbol_roles *roles /* may be NULL */, ookd_symbol_survey *out);
/* HIP-event time of the last ookd_rx_symbol_survey call: the zeroing of the
 * result and its kernels.  0 when that call was refused or had nothing to
 * launch, and after a new run until somebody asks about it. */
float ookd_rx_symbol_kernel_ms(const ookd_rx *rx);

/* The coding rule, pure host code.  From the timing classes and the kind counts:
 *   1. Kinds with a class 16 never take a role.
 *   2. The others with a count > 0 are ordered by count descending, ties to the
 *      smaller (on class, off class).  Fewer than 3: found = 0, reason
 *      OOKD_CODING_KINDS.
 *   3. The first two are the data kinds.  They must share their on class,
 *      otherwise OOKD_CODING_NOT_DISTANCE (pulse-width coding is outside this
 *      family).  ZERO is the one with the shorter off class.  With t0 < t1 the
 *      mean_us of the two off classes (give ookd_suggest_pulses the sample
 *      rate), 1.15 t0 < 0.85 t1 must hold -- the state machine's +-15 % windows
 *      must not meet --, otherwise OOKD_CODING_AMBIGUOUS.
 *   4. SYNC is the first kind after those two in the same order whose count is
 *      >= 2; if there is none: OOKD_CODING_NO_SYNC.
 * roles receives the three roles (all OTHER when found = 0).  Which of the two
 * gaps means 0 cannot be known from a capture: shorter = 0 is the convention of
 * both reference devices. */
enum {
    OOKD_CODING_OK = 0,
    OOKD_CODING_KINDS = 1,          /* fewer than three kinds of symbols         */
    OOKD_CODING_NOT_DISTANCE = 2,   /* the two data kinds differ in their pulse  */
    OOKD_CODING_AMBIGUOUS = 3,      /* the two gaps lie too close together       */
    OOKD_CODING_NO_SYNC = 4,        /* no third kind that occurs at least twice  */
    OOKD_CODING_NO_FRAMES = 5,      /* no frame length that half the frames have */
    OOKD_CODING_TOO_LONG = 6        /* more bits than OOKD_MAX_PAYLOAD_BYTES hold */
};
typedef struct ookd_coding {
    int found;
    uint32_t reason;                /* OOKD_CODING_*                             */
    uint32_t data_on_class, zero_off_class, one_off_class;
    uint32_t sync_on_class, sync_off_class, reserved;
    uint64_t zero_count, one_count, sync_count;
    double t0_us, t1_us;            /* mean gap of a zero and of a one           */
} ookd_coding;
/* 0, or OOKD_ERR_ARG for a NULL argument.  Only survey->kinds is read. */
int ookd_suggest_coding(const ookd_pulse_suggestion *pulses, const ookd_symbol_survey *survey,
                        ookd_symbol_roles *roles, ookd_coding *out);

/* The device rule, pure host code.  survey is one computed WITH the roles of
 * ookd_suggest_coding; sample_rate is that of the decimated samples.
 *   5. Among the distances 3 <= D < 511 -- a frame of 1 or 2 symbols holds no
 *      bit, and bin 511 holds every longer distance: neither can be a message --
 *      L = the distance with the most clean frames, ties to the smaller D.
 *      frames[1][L] >= 1 and 2 frames[1][L] >= the number of all frames of those
 *      distances, clean or not, must hold, otherwise OOKD_CODING_NO_FRAMES.
 *      num_bits = L - 2 (the sync symbol and the closing pulse's symbol); more
 *      than 8 OOKD_MAX_PAYLOAD_BYTES: OOKD_CODING_TOO_LONG.
 *   6. Durations in microseconds are llround(class mean / sample_rate * 1e6).
 *   7. The device has six states, in this order:
 *      reset:      always -> idle.
 *      idle:       pulse_start -> sync_pulse.
 *      sync_pulse: duration = sync on, timeout = twice that; pulse_end ->
 *                  sync_gap; timeout -> reset.
 *      sync_gap:   duration = sync off, timeout = twice that; pulse_start ->
 *                  bit_pulse; timeout -> reset.
 *      bit_pulse:  duration = data on, timeout = twice that; msg_complete ->
 *                  reset with output_data; pulse_end -> bit_gap; timeout -> reset.
 *      bit_gap:    timeout = 2 t1; pulse_start with duration t0 -> bit_pulse,
 *                  append_0; pulse_start with duration t1 -> bit_pulse, append_1;
 *                  timeout -> reset.
 * A coding with found = 0 is passed through: found = 0 with its reason.
 * Limits: this family only; one device per capture; two levels; fields are not
 * inferred; the zero / one polarity is a convention; a capture whose pauses fall
 * into the sync gap's class (its closing symbols then count as syncs, and frames
 * of 1 and of L - 1 symbols appear beside the true ones) is answered only while
 * the modal-frame test of step 5 holds. */
typedef struct ookd_device_suggestion {
    int found;
    uint32_t reason;                /* OOKD_CODING_*                             */
    uint32_t num_bits, frame_symbols;       /* L - 2, L                          */
    uint64_t sync_on_us, sync_off_us, bit_on_us, zero_off_us, one_off_us;
    uint64_t frames_seen;           /* all frames, every distance, clean or not  */
    uint64_t frames_counted;        /* those with 3 <= D < 511, clean or not     */
    uint64_t frames_clean;          /* clean frames at distance L                */
    uint64_t num_syncs;
} ookd_device_suggestion;
/* 0, or OOKD_ERR_ARG for a NULL argument or a sample_rate that is not > 0. */
int ookd_suggest_device(const ookd_pulse_suggestion *pulses, const ookd_symbol_survey *survey,
                        const ookd_coding *coding, double sample_rate, ookd_device_suggestion *out);
/* The suggested device through ookd_device_create (state names reset, s1 .. s5);
 * NULL for a suggestion with found = 0. */
ookd_device *ookd_device_from_suggestion(const ookd_device_suggestion *s, uint32_t sample_rate);
/* A device JSON that ookd_device_load accepts, with the states above, no ts_mode
 * and hex fields over all bits: one field "Payload" up to 64 bits, otherwise
 * "Payload0", "Payload1", ... of 64 bits each (a field holds 64 bits at most).
 * snprintf convention: returns the number of characters the full text has and
 * stores at most size - 1 of them plus a NUL; 0 for a NULL suggestion or name or
 * a suggestion with found = 0. */
size_t ookd_device_suggestion_json(const ookd_device_suggestion *s, const char *name, char *buf, size_t size);

/* ------------------------------------------------------------------------
 * Edge cleaning: drop glitch runs before the surveys.  Both surveys above take
 * the edge list as it is: a one-sample glitch is a class of its own, splits the
 * run it sits in and puts a symbol of its own between two frames.  One more
 * by-product pass over the finished run's edge list deletes the runs shorter
 * than a caller-given length and leaves a second, cleaned list in HBM; the
 * survey kernels read that list unchanged (ookd_rx_pulse_hist_clean,
 * ookd_rx_symbol_survey_clean).  A run nobody asks about stays what it was:
 * the run's own list, ookd_rx_get_edges, ookd_rx_pulse_hist,
 * ookd_rx_symbol_survey, the decoder and every result of the run are untouched.
 *
 * The rule, a contract.  Take capture (or carrier) c of the last run.  Take its
 * edge list e[0..E) and the closed runs of the pulse survey's contract.  Run i,
 * 0 <= i < E - 1, has length L_i = e[i+1] - e[i].  It is "on" when i is even.
 *
 * Two lengths are given in decimated samples: min_on and min_off (uint64).  0
 * and 1 mean "keep every run of that level".
 *
 *   - short(i) = L_i < min[level(i)].  The comparison is strict.
 *   - d(-1) = 0, and d(i) = short(i) && !d(i-1).  A deleted run takes its two
 *     edges with it.  Its neighbours and the run itself merge into one run.  The
 *     run after it no longer exists on its own and cannot be deleted again.
 *   - Edge i is dropped iff d(i) (for i < E - 1) or d(i-1) (for i >= 1).
 *   - The cleaned list is the kept edges in order.
 *   - The two open runs (before e[0], after e[E-1]) are never short.  n_out is
 *     unchanged.
 *
 * An equivalent parallel form: inside a maximal chain of consecutive short runs
 * starting at run a, d(i) = ((i - a) even).  A chatter burst of m short runs
 * vanishes entirely when m is odd.  It leaves exactly its last edge when m is
 * even.
 *
 * Consequences: the number of dropped edges is even, so E & 1 (the tail level)
 * and "the first edge rises" survive; no closed run of the cleaned list is
 * shorter than the minimum of its level; cleaning a cleaned list with the same
 * minimums changes nothing; min_on, min_off <= 1 returns the list itself.
 *
 * ookd_clean_edges is the rule in pure host code (no GPU needed), for hosts that
 * already hold an edge list.  It follows the ookd_rx_get_edges convention:
 * *num_out receives the cleaned list's length whatever the capacity, and at most
 * `capacity` edges are stored when out != NULL.  OOKD_ERR_ARG for edges == NULL
 * with E != 0.
 *
 * ookd_rx_clean_edges cleans ALL captures (carriers) of the last run in one
 * timed pass of three dependent kernel launches on the context's stream.  A
 * repeated call with the same minimums on the same run launches nothing; other
 * minimums recompute, and what the two clean readers kept is forgotten.  The
 * cleaned list, its prefix and the pass's work space are allocated by the first
 * call in the life of the context, sized by the run's num_edges, grown and never
 * shrunk, and freed with the context.  It refuses what ookd_rx_pulse_hist
 * refuses, with the same codes and messages: no finished run, a shard run, a
 * pipelined run, an overflowed list.  A run of no samples is valid and launches
 * nothing.
 *
 * ookd_rx_get_clean_info, ookd_rx_get_clean_edges (the ookd_rx_get_edges
 * convention), ookd_rx_pulse_hist_clean and ookd_rx_symbol_survey_clean answer
 * from the cleaned list of the LAST run: OOKD_ERR_ARG "no cleaned list of the
 * last run" when ookd_rx_clean_edges has not answered it.  The two clean readers
 * take the arguments of the originals, run the originals' kernels over the
 * cleaned list and keep the originals' contracts, with "its edge list" read as
 * "its cleaned edge list"; their times are not reported separately.
 * ---------------------------------------------------------------------- */
typedef struct ookd_clean_info {
    uint64_t edges_in, edges_out;   /* E before and after                        */
    uint64_t deleted[2];            /* [level]: runs deleted, 1 = "on"           */
    uint64_t min_on, min_off;       /* as given                                  */
} ookd_clean_info;
int ookd_clean_edges(const uint64_t *edges, uint64_t E, uint64_t min_on, uint64_t min_off,
                     uint64_t *out, uint64_t capacity, uint64_t *num_out);
int ookd_rx_clean_edges(ookd_rx *rx, uint64_t min_on, uint64_t min_off);
int ookd_rx_get_clean_info(const ookd_rx *rx, uint32_t capture, ookd_clean_info *out);
int ookd_rx_get_clean_edges(const ookd_rx *rx, uint32_t capture, uint64_t *edges, uint64_t capacity,
                            uint64_t *num_edges);
int ookd_rx_pulse_hist_clean(ookd_rx *rx, uint32_t capture, ookd_pulse_hist *out);
int ookd_rx_symbol_survey_clean(ookd_rx *rx, uint32_t capture, const ookd_symbol_table *table,
                                const ookd_symbol_roles *roles /* may be NULL */, ookd_symbol_survey *out);
/* HIP-event time of the pass that cleaned the last run's lists: the zeroing of
 * the counts and the three kernels.  0 while ookd_rx_clean_edges has not answered
 * the last run (also when the call was refused, or the run had no samples). */
float ookd_rx_clean_kernel_ms(const ookd_rx *rx);

/* ------------------------------------------------------------------------
 * Debounced decode: the state machine on the cleaned edge list.  Opt-in, per
 * context.  With a minimum above 1 set, EVERY run of the context cleans its edge
 * list on the GPU as part of the run's chain -- the three kernels of the pass
 * above and a fourth that makes the cleaned list's prefix over blocks of 4096
 * outputs -- and the state machine decodes the cleaned list: the scan in all its
 * forms, the round form, and the redo of the captures the scan refused.
 *
 * min_on, min_off are in decimated samples and follow the clean rule: a run is
 * short when its length is < the minimum of its level (strict), 0 and 1 keep
 * every run of that level.  Both <= 1 turns the debounce off: the context then
 * queues exactly the launches it queued before this call existed, and gives the
 * same results.
 *
 * What the decoder sees, a contract.  Take capture (or carrier) c of the run, its
 * edge list e, and the bit stream painted over n_out decimated samples from
 * ookd_clean_edges(e, min_on, min_off): level 0 before the first edge, toggling
 * at every edge.  Messages, payloads, every error position and num_errors of c
 * are those of the reference state machine fed that stream buffer by buffer
 * (samples_per_buffer / total decimation samples each).  ookd_message.sample
 * keeps its meaning.
 *
 * What stays the run's own: ookd_rx_get_bits, the dig recorders, ookd_rx_get_fir,
 * ookd_rx_get_edges, ookd_rx_pulse_hist, ookd_rx_symbol_survey and
 * ookd_rx_stats.num_edges are the raw stream's.  edge_capacity bounds the raw
 * list, and an edge overflow fails the run as before.
 *
 * The list made in the chain IS the context's cleaned list of that run:
 * ookd_rx_get_clean_edges, ookd_rx_get_clean_info, ookd_rx_pulse_hist_clean and
 * ookd_rx_symbol_survey_clean answer from it without any ookd_rx_clean_edges
 * call, ookd_rx_clean_edges with the same minimums launches nothing, and with
 * other minimums it recomputes the list for the readers only (the run's results
 * are final).  ookd_rx_clean_kernel_ms stays 0: the pass is part of the chain and
 * inside ookd_rx_stats.total_device_ms.  The per-capture counts are fetched by
 * the first call that asks for them, not by the run.
 *
 * Nothing between the front end and the state machine waits for the host: the
 * pass is queued on the context's stream with its grids sized by edge_capacity,
 * so ookd_rx_submit_device / ookd_rx_wait and several contexts in flight work as
 * they did.  Batched runs and carrier contexts work (carriers are captures).  A
 * context without a device makes the cleaned list and runs no state machine.
 *
 * Refused or changed: a debounced context never pipelines a capture in chunks
 * (it behaves as with OOKD_RX_NO_PIPELINE; stats.pipeline_chunks is 0), and
 * ookd_rx_shard_begin / ookd_rx_shard_refine return OOKD_ERR_ARG naming the
 * debounce: chunk-local lists and the level carried into a shard are outside the
 * clean rule, as they are for ookd_rx_clean_edges.
 *
 * ookd_rx_set_debounce may be called between runs (it takes effect with the
 * next); OOKD_ERR_ARG while a run is in flight (submitted, not waited for) and
 * for rx == NULL.  The first call with a minimum above 1 allocates what the
 * chain needs -- the cleaned list, the per-block prefix and the pass's work
 * space -- sized by the context's edge_capacity and max_captures.  When that
 * fails the call returns OOKD_ERR_NOMEM and leaves the debounce OFF (0, 0),
 * whatever it was.  Where the call has to replace the buffers of an earlier
 * ookd_rx_clean_edges (a context that was cleaned by hand first), the last
 * run's cleaned list goes with them: the clean readers answer "no cleaned list
 * of the last run" until the next run or the next ookd_rx_clean_edges.
 * ookd_rx_get_debounce returns the minimums as set (either pointer may be NULL).
 *
 * The per-capture counts of a debounced run are fetched by the first of
 * ookd_rx_get_clean_info, ookd_rx_get_clean_edges, ookd_rx_pulse_hist_clean and
 * ookd_rx_symbol_survey_clean after it: that call does one blocking copy from
 * the device and, although two of them take a const context, updates the
 * context.  Like every call on a context they must not run concurrently with
 * one another on the same context.
 * ---------------------------------------------------------------------- */
int ookd_rx_set_debounce(ookd_rx *rx, uint64_t min_on, uint64_t min_off);
int ookd_rx_get_debounce(const ookd_rx *rx, uint64_t *min_on, uint64_t *min_off);

/* ------------------------------------------------------------------------
 * Pulse levels: the peak power of every on-run of the last run, and a level per
 * message.  A decoded message says where and what, not how strong; two
 * transmitters at different distances on one frequency differ in exactly that.
 *
 * The contract.  Take capture (or carrier) c of the context's last run, its edge
 * list e[0..E) as ookd_rx_get_edges returns it and n_out =
 * ookd_rx_stats.decimated_samples.
 *   - On-run r, 0 <= r < R = ceil(E / 2), covers outputs [e[2r], f_r), f_r =
 *     e[2r + 1], or n_out for an open last run.
 *   - p_j is the power the slicer compares, restated by the context's kind:
 *       untuned context   the survey contract at ookd_survey_create: unpack, FIR
 *                         stages in the reference's order with a separately
 *                         rounded multiply and add per tap, then re*re + im*im
 *                         with three roundings;
 *       tuned or carrier  the tuned survey contract at ookd_survey_create_tuned
 *                         with that carrier's nu (nu = 0 included: the same
 *                         powers as the untuned contract);
 *       no filter         |x_j|^2.
 *     The history in front of the capture is zero.  Inputs at or beyond the
 *     run's n samples are zero and are never read from memory: the capture's
 *     allocation may end at n.  p_j is therefore defined for every j < n_out,
 *     the padding to whole buffers included -- where a capture that ends high
 *     falls.  (An 8-bit capture is the SC16Q11 capture of 16 times its values.)
 *   - peak[r] = max over the run's j of p_j, as a float.  Powers are not
 *     negative, so the maximum of the bit patterns as uint32 is the maximum of
 *     the values: the result is exact and independent of any order.
 *   - hist is an ookd_level_hist of the R peaks under ookd_level_bin, samples = R.
 *   - tile_outputs is the pass's tile; tiles_total = ceil(n_out / tile_outputs);
 *     tiles_filtered counts the tiles [t tile, (t + 1) tile) that hold at least
 *     one output of an on-run -- a function of the edge list, and the number of
 *     tiles the kernel ran the filter on (it counts them itself).
 *
 * Like ookd_rx_pulse_hist the pass is a by-product of a finished run: a run
 * nobody asks about launches and allocates nothing.  The first of these calls
 * after a run makes one timed pass on the context's stream for all captures or
 * carriers of the run (ookd_rx_levels_kernel_ms: its HIP-event time, 0 while
 * nobody has asked or there was nothing to launch); later calls about the same
 * run answer from what it left.  The calls refuse what ookd_rx_pulse_hist
 * refuses, with the same codes: no finished run, a run in flight, a shard run, a
 * pipelined run (OOKD_ERR_ARG), an overflowed edge list (OOKD_ERR_CAPACITY), a
 * capture out of range.  A run of no samples is valid and launches nothing.  A
 * filter whose history the pass's LDS window cannot hold (the one
 * ookd_survey_create refuses) is refused at the first call with that message.
 *
 * The capture is read again, through the pointer and stride the context recorded
 * at submit: the caller of ookd_rx_process_device / ookd_rx_submit_device keeps
 * the capture resident and unchanged until the first of these calls about the
 * run has returned.  After ookd_rx_process_host it is the context's own copy.
 *
 * The _clean forms read the cleaned list of the last run (ookd_rx_clean_edges,
 * or a debounced context's own) in the place of the run's list: an on-run that
 * swallowed a short off-run reports the maximum over its whole extent.  Each
 * form keeps its own pass and time; ookd_rx_levels_kernel_ms is the raw list's.
 * When ookd_rx_clean_edges makes another list for the same run (other
 * minimums), the next _clean call makes a new pass over that list, as
 * ookd_rx_pulse_hist_clean does.
 *
 * ookd_rx_get_run_peaks follows the ookd_rx_get_edges convention: *num_runs
 * receives R, at most `capacity` peaks are stored, peaks may be NULL.
 *
 * Limits: the peak only, no mean; the levels of off-runs are the survey's
 * business (ookd_survey_*); shard and pipelined runs are refused.
 * ---------------------------------------------------------------------- */
typedef struct ookd_run_levels {
    uint64_t num_runs;              /* R                                      */
    uint64_t tiles_total;
    uint64_t tiles_filtered;
    uint32_t tile_outputs;
    uint32_t reserved;
    ookd_level_hist hist;           /* of the R peaks                         */
} ookd_run_levels;

int ookd_rx_run_levels(ookd_rx *rx, uint32_t capture, ookd_run_levels *out);
int ookd_rx_run_levels_clean(ookd_rx *rx, uint32_t capture, ookd_run_levels *out);
int ookd_rx_get_run_peaks(ookd_rx *rx, uint32_t capture, float *peaks, uint64_t capacity,
                          uint64_t *num_runs);
int ookd_rx_get_run_peaks_clean(ookd_rx *rx, uint32_t capture, float *peaks, uint64_t capacity,
                                uint64_t *num_runs);
float ookd_rx_levels_kernel_ms(const ookd_rx *rx);

/* A level per message, pure host code (no GPU).  edges[0..E) and peaks[0..R),
 * R = ceil(E / 2), are one capture's; msg_samples[0..M) that capture's
 * ookd_message.sample values, ascending.  Message m takes the on-runs whose
 * rising edge is <= msg_samples[m] and > msg_samples[m - 1] (every run up to
 * msg_samples[0] for the first message), of these the last `pulses`, and
 * levels[m] is their lower median: element (count - 1) / 2 of the sorted peaks;
 * 0 when there are none.  OOKD_ERR_ARG for a NULL array that is not empty,
 * R != ceil(E / 2), msg_samples that descend, or pulses = 0. */
int ookd_message_levels(const uint64_t *edges, uint64_t E, const float *peaks, uint64_t R,
                        const uint64_t *msg_samples, uint64_t M, uint32_t pulses, float *levels);

/* ------------------------------------------------------------------------
 * Pulse moments: the mean power and the carrier of every on-run of the last run,
 * and per message.  Two remotes of one model on one channel decode to the same
 * kind of message and, at like distances, to like levels; they almost always
 * differ in their carrier.  The phase step between neighbouring filter outputs
 * of a pulse is the transmitter's frequency, and the filter's complex output is
 * formed anyway where the pulse levels take its power.
 *
 * The contract.  Take capture (or carrier) c of the context's last run, its edge
 * list e[0..E) and n_out.  On-run r covers outputs [a_r, f_r) exactly as "Pulse
 * levels" defines them: a_r = e[2r], f_r = e[2r + 1], or n_out for an open last
 * run, the padding to whole buffers included, inputs at or beyond n zero and
 * never loaded.
 *   - y_j = (re_j, im_j) is the float32 complex filter output whose power the
 *     levels' contract calls p_j, by the context's kind: the untuned survey
 *     contract, the tuned survey contract with that carrier's nu, or the
 *     unpacked sample without a filter.  p_j = re*re + im*im with three
 *     roundings, as there.
 *   - For j > a_r inside the run the lag product against the output before is
 *     formed without fused multiply-adds, each product rounded, then the sum or
 *     the difference rounded:
 *         zr_j = (re_j * re_{j-1}) + (im_j * im_{j-1})
 *         zi_j = (im_j * re_{j-1}) - (re_j * im_{j-1})
 *   - q(v) = llrint((double)v * 2^30), ties to even, after v has been clamped to
 *     [-2^32, 2^32]; a NaN gives 0.  The product in double is exact, and for
 *     |v| >= 2^-7 the rounding does nothing (a float32 of that size has no bits
 *     below 2^-30).
 *   - power[r]  = sum over j = a_r     .. f_r - 1 of q(p_j)
 *     lag_re[r] = sum over j = a_r + 1 .. f_r - 1 of q(zr_j)
 *     lag_im[r] = sum over j = a_r + 1 .. f_r - 1 of q(zi_j)
 *     each an int64 taken modulo 2^64 (two's complement wrap).  A run of one
 *     output has lag 0.  No pair joins two captures: a run that rises at output
 *     0 has its first pair at j = 1.
 *   - Integer sums need no order, so the result is an exact function of the
 *     capture and the edge list, however many workgroups share a run -- the
 *     argument the levels make for the maximum of bit patterns.
 *   - The sums do not wrap for runs of up to 2^21 outputs of a full-scale
 *     SC16Q11 capture through a filter with sum |h| <= 2: |y| <= 32 sqrt 2 there,
 *     every term is at most 2^11 * 2^30 in magnitude, and 2^21 of them stay
 *     below 2^63 (the clamp bounds a term by 2^62 whatever the capture holds).
 *     Nominal signals, |y| <= 1, have room for runs just short of 2^33 outputs.
 *   - tile_outputs, tiles_total and tiles_filtered are as at ookd_run_levels, for
 *     this pass's own tile: it keeps one more output per tile than the levels'
 *     pass, so its tile may be smaller for the same filter.  decimation is D,
 *     the filter's total decimation (1 without a filter).
 *
 * The calls behave as the pulse levels' do: a by-product of a finished run that
 * launches and allocates nothing unless asked; one timed pass on the context's
 * stream for all captures or carriers at the first call about a run
 * (ookd_rx_moments_kernel_ms, the raw list's), later calls answer from what it
 * left; the refusals of ookd_rx_pulse_hist with the same codes, and the LDS
 * window's; a run of no samples is valid and launches nothing; the capture is
 * read again and stays resident and unchanged until the first call has returned;
 * the _clean forms read the cleaned list, keep their own pass, and make a new
 * pass when ookd_rx_clean_edges has made another list.
 * ookd_rx_get_run_moments follows the ookd_rx_get_edges convention.
 *
 * ookd_run_moments_of is the contract on the host, pure C++ (no GPU), given the
 * filter's output y[n_out][2] and one list: out[0..R), R = ceil(E / 2).
 * OOKD_ERR_ARG for a NULL array that is not empty, R != ceil(E / 2), or edges
 * that do not ascend strictly below n_out.
 *
 * ookd_message_carriers is host only.  edges, moments and msg_samples are one
 * capture's, as at ookd_message_levels, and message m takes the on-runs that
 * rule takes: the last `pulses` of those rising in (msg_samples[m - 1],
 * msg_samples[m]].  Their three sums and their lengths (an open last run ends
 * at n_out) are added as doubles in ascending r to P, Zr, Zi and `outputs`:
 *     mean_power = P / 2^30 / outputs          (0 without a run)
 *     coherence  = hypot(Zr, Zi) / P           (0 when P = 0): 1 for one clean
 *                  carrier, less with noise or a second signal in the band
 *     carrier    = nu + wrap(atan2(Zi, Zr) / 2 pi - nu D) / D, wrap into
 *                  [-1/2, 1/2), in cycles per INPUT sample -- the unit of
 *                  ookd_rx tuning.  The tuned filter is a band-pass, not a
 *                  mixer: y advances by 2 pi f D per output whatever nu is, so
 *                  the estimate is absolute modulo 1 / D and the branch nearest
 *                  nu is taken (nu = 0 for an untuned context).
 * Without a pair (Zr = Zi = 0) carrier = nu and coherence = 0.  OOKD_ERR_ARG for
 * what ookd_message_levels refuses, decimation = 0, or an open last run that
 * begins at or beyond n_out.
 *
 * Limits: on-runs only; lag 1 only; the estimate is unambiguous within
 * +-1 / (2 D) of nu; a DC term or a second carrier inside the filter's band
 * biases it; shard and pipelined runs are refused.
 * ---------------------------------------------------------------------- */
typedef struct ookd_run_moment {
    int64_t power, lag_re, lag_im;  /* fixed point, 30 fraction bits          */
} ookd_run_moment;

typedef struct ookd_run_moments {
    uint64_t num_runs;              /* R                                      */
    uint64_t tiles_total;
    uint64_t tiles_filtered;
    uint32_t tile_outputs;
    uint32_t decimation;            /* D                                      */
} ookd_run_moments;

typedef struct ookd_message_carrier {
    double carrier;                 /* cycles per input sample                */
    double mean_power;
    double coherence;
    uint64_t outputs;
} ookd_message_carrier;

int ookd_rx_run_moments(ookd_rx *rx, uint32_t capture, ookd_run_moments *out);
int ookd_rx_run_moments_clean(ookd_rx *rx, uint32_t capture, ookd_run_moments *out);
int ookd_rx_get_run_moments(ookd_rx *rx, uint32_t capture, ookd_run_moment *moments,
                            uint64_t capacity, uint64_t *num_runs);
int ookd_rx_get_run_moments_clean(ookd_rx *rx, uint32_t capture, ookd_run_moment *moments,
                                  uint64_t capacity, uint64_t *num_runs);
float ookd_rx_moments_kernel_ms(const ookd_rx *rx);
int ookd_run_moments_of(const float *y, uint64_t n_out, const uint64_t *edges, uint64_t E,
                        ookd_run_moment *out, uint64_t R);
int ookd_message_carriers(const uint64_t *edges, uint64_t E, uint64_t n_out,
                          const ookd_run_moment *moments, uint64_t R, const uint64_t *msg_samples,
                          uint64_t M, uint32_t pulses, uint32_t decimation, double nu,
                          ookd_message_carrier *out);

/* ------------------------------------------------------------------------
 * Burst extraction: the on-stretches of the last run's captures, cut out of
 * the capture on the GPU.  A run says where the transmissions are and what
 * they hold; this hands back the signal itself -- only the part that matters,
 * in the capture's own sample format -- without the whole capture crossing
 * PCIe.  The counterpart of a recorder that writes only what was keyed.
 *
 * The contract.  Take capture (or carrier) c of the context's last run: its edge
 * list e[0..E) as ookd_rx_get_edges returns it (the cleaned list with
 * OOKD_BURSTS_CLEAN), n_out = ookd_rx_stats.decimated_samples, D the filter's
 * total decimation (1 without a filter) and n the samples per capture that
 * exist in memory (the run's n_valid).
 *   - On-run r, 0 <= r < R = ceil(E / 2), covers outputs [a_r, f_r): a_r = e[2r],
 *     f_r = e[2r + 1], or n_out for an open last run (as at ookd_rx_run_levels).
 *     g_r = a_{r+1} - f_r is the off-run behind run r.
 *   - pre, post and max_gap are in decimated samples.  max_gap < pre + post is
 *     refused (OOKD_ERR_ARG): bursts can then never overlap.
 *   - A burst begins at run 0 and at every run r + 1 with g_r > max_gap (strict:
 *     a gap of exactly max_gap joins).  Burst b with runs [r0, r1] covers outputs
 *     [lo, hi), lo = a_r0 - min(a_r0, pre), hi = min(n_out, f_r1 + post), and in
 *     input samples [first, end), first = min(n, lo D), end = min(n, hi D).
 *     num_samples = end - first; it is 0 for a burst that lies wholly in the
 *     padding behind n, and such a burst stays in the table.
 *     offset_b = the sum of num_samples over the capture's bursts before b, and
 *     total = the sum over all of them.
 *   - The table is one ookd_burst per burst.  The cut is `total` samples in the
 *     capture's own format (4 bytes for SC16Q11, 2 for CS8 / CU8, never
 *     widened): sample offset_b + i of the cut is sample first_b + i of the
 *     capture, byte for byte.  Samples at or beyond n are never read: the
 *     capture's allocation may end at n.  In a carrier context list k cuts the
 *     one capture it was decoded from.
 *   - Everything is an exact function of the edge list and the capture's bytes.
 *
 * ookd_find_bursts is the rule on the host, pure C++ (no GPU), over one list.
 * It follows the ookd_rx_get_edges convention: *num_bursts receives the count,
 * at most `capacity` entries are stored, table may be NULL; *total (may be
 * NULL) receives the cut's length.  OOKD_ERR_ARG for max_gap < pre + post, a
 * NULL edge array that is not empty, or D = 0.
 *
 * ookd_rx_bursts makes the table for all captures (or carriers) of the last
 * run in one timed pass on the context's stream (ookd_rx_bursts_kernel_ms: its
 * HIP-event time, 0 while nobody has asked or there was nothing to launch).
 * Like ookd_rx_pulse_hist it is a by-product of a finished run: a run nobody
 * asks about launches and allocates nothing.  It refuses what
 * ookd_rx_pulse_hist refuses, with the same codes.  OOKD_BURSTS_CLEAN reads the
 * cleaned list of the last run (ookd_rx_clean_edges, or a debounced context's
 * own) and is refused without one, as ookd_rx_run_levels_clean is.  The same
 * parameters on the same run launch nothing; other parameters, or another
 * cleaned list of the same run, make a new table.  The raw and the clean form
 * keep a table each; ookd_rx_get_burst_info, ookd_rx_get_bursts and the two
 * copy calls are about the form ookd_rx_bursts was last called with for this
 * run, and are refused (OOKD_ERR_ARG) when the last run has no table.
 * ookd_rx_bursts_kernel_ms is the time of that form's pass.
 *
 * ookd_rx_copy_bursts_device writes the cut of one capture to device memory of
 * the context's device: capacity_samples < total is OOKD_ERR_CAPACITY and
 * nothing is written; nothing at or beyond `total` samples is written either.
 * The kernel moves 16-byte vectors when d_out is 16-byte aligned (any hipMalloc
 * pointer is) and single samples otherwise.  ookd_rx_copy_bursts_host does the
 * same through a device buffer of exactly `total` samples that it allocates and
 * frees.  ookd_rx_burst_copy_kernel_ms is the HIP-event time of the last copy
 * kernel about the last run (0: none, or a cut of no samples).
 *
 * The capture is read again by the copy, through the pointer and stride the
 * context recorded at submit: the caller of ookd_rx_process_device /
 * ookd_rx_submit_device keeps the capture resident and unchanged until the
 * copy has returned.  After ookd_rx_process_host it is the context's own copy.
 * The table pass reads the edge list only.
 *
 * Limits: shard and pipelined runs are refused; one cut per call (no batch of
 * captures in one launch); the cut is not resampled or filtered ("Burst
 * basebands" hands back the filter's output over the same bursts).
 * ---------------------------------------------------------------------- */
typedef struct ookd_burst {
    uint64_t first_sample;          /* input sample of the capture the burst begins at */
    uint64_t num_samples;
    uint64_t offset;                /* sample of the cut the burst begins at  */
    uint64_t first_run;             /* r0                                     */
    uint64_t num_runs;              /* r1 - r0 + 1                            */
} ookd_burst;

typedef struct ookd_burst_info {
    uint64_t num_bursts;
    uint64_t total_samples;
    uint64_t num_runs;              /* R                                      */
    uint64_t pre, post, max_gap;    /* as given to ookd_rx_bursts             */
    uint32_t flags;                 /* OOKD_BURSTS_*                          */
    uint32_t sample_bytes;          /* of one sample of the cut: 4 or 2       */
    uint32_t tile_edges;            /* edges of one tile of the table pass    */
    uint32_t decimation;            /* D                                      */
} ookd_burst_info;

enum {
    OOKD_BURSTS_CLEAN = 1           /* read the cleaned list of the last run  */
};

int ookd_find_bursts(const uint64_t *edges, uint64_t E, uint64_t n_out, uint64_t D, uint64_t n,
                     uint64_t pre, uint64_t post, uint64_t max_gap, ookd_burst *table,
                     uint64_t capacity, uint64_t *num_bursts, uint64_t *total);
int ookd_rx_bursts(ookd_rx *rx, uint64_t pre, uint64_t post, uint64_t max_gap, uint32_t flags);
int ookd_rx_get_burst_info(const ookd_rx *rx, uint32_t capture, ookd_burst_info *out);
int ookd_rx_get_bursts(const ookd_rx *rx, uint32_t capture, ookd_burst *table, uint64_t capacity,
                       uint64_t *num_bursts);
int ookd_rx_copy_bursts_device(ookd_rx *rx, uint32_t capture, void *d_out, uint64_t capacity_samples);
int ookd_rx_copy_bursts_host(ookd_rx *rx, uint32_t capture, void *out, uint64_t capacity_samples);
float ookd_rx_bursts_kernel_ms(const ookd_rx *rx);
float ookd_rx_burst_copy_kernel_ms(const ookd_rx *rx);

/* ------------------------------------------------------------------------
 * Burst spectra: a Welch spectrum and the carrier of every burst of the burst
 * table, on the GPU -- which transmitter keyed when in a wide-band capture.
 * ookd_spectrum_* sums over the whole capture: it names the carriers, not the
 * bursts they belong to, and a transmitter's ratio to the median falls with
 * its duty cycle.  Here a context without a filter (threshold on |x|^2) cuts
 * every transmitter's bursts, each burst gets its own spectrum, and the host
 * rule ookd_suggest_burst_carriers groups the bursts by their peak bin.
 *
 * The contract.  Take capture (or carrier list) c and the burst table that
 * ookd_rx_bursts last made for this run: the raw or the clean form, whichever
 * was last called.  With no table the call is OOKD_ERR_ARG.
 *   - Burst b has first_sample, num_samples and F_b = floor(num_samples / 1024)
 *     whole frames; frame f of burst b is capture samples
 *     [first_sample + 1024 f, first_sample + 1024 f + 1024).  Nothing is padded
 *     and nothing outside the burst is read; the ragged rest behind the last
 *     whole frame is not counted.
 *   - Unpack, window, transform and |X|^2 are exactly those of ookd_spectrum_*
 *     (v / 2048, 16 v for the 8-bit formats first, periodic Hann, FFT order,
 *     the sign convention of ookd_tune.nu).
 *   - power_b[k] = sum_f |X_{b,f}[k]|^2.  fp32 inside a frame, at most 32 frames
 *     in fp32 between folds into double, double beyond: the spectrum section's
 *     budget, so its bound holds per burst with S and E taken over that burst,
 *         |power_b[k] - S_b[k]| <= 2 EPS sqrt(S_b[k] E_b) + EPS^2 E_b + EPS S_b[k],
 *     EPS = OOKD_SPECTRUM_EPS.
 *   - Per burst one ookd_burst_spectrum.  A constant through the periodic Hann
 *     window lands on bins -1, 0, +1 exactly: those three are set apart as
 *     dc_power = (power_b[1023] + power_b[0]) + power_b[1], and the peak is the
 *     largest power_b[k] over k = 2 .. 1022, ties going to the lowest k.
 *     peak_bin and peak_power are exact functions of the power_b[] this library
 *     computed: power[peak_bin] == peak_power bit for bit, with power[] from
 *     ookd_rx_burst_spectrum.  total_power is within 1024 * 2^-53 (relative) of
 *     the float64 sum of that power_b[].  With frames = 0 everything is 0.
 *   - The keyed spectrum of the capture is an ookd_spectrum_result with
 *     frames = sum_b F_b and power[k] = sum_b power_b[k]: the Welch spectrum of
 *     the keyed part alone, which ookd_suggest_carriers takes unchanged.  It has
 *     the same kind of bound, with S and E over all bursts.
 *   - No floating-point atomics, no workgroup waits for another, every sum has
 *     a fixed order: two calls with the same arguments on the same run return
 *     bitwise identical results.  The order depends on span_frames; results at
 *     different spans agree within the bound, not bit for bit.
 *
 * span_frames.  The cut's coordinate offset_b + 1024 f orders all frames of a
 * capture; workgroup g takes the frames whose coordinate lies in
 * [g S 1024, (g + 1) S 1024), S = span_frames, so there are
 * spans = ceil(total / (1024 S)) workgroups.  A burst whose frames lie in more
 * than one span leaves a row of 1024 doubles per span, at most two rows per
 * span; a second kernel adds them in span order.  partial_rows = 2 spans rows
 * of 8 KiB are kept, capped at 64 MiB (8192 rows), beside 8 KiB per span for
 * the keyed spectrum.  span_frames must be 0 or a power of two >= 32, anything
 * else is OOKD_ERR_ARG; 0 takes the smallest that fits the cap: 32 for every
 * cut of up to 2^27 samples.  A span whose rows exceed the cap is
 * OOKD_ERR_CAPACITY and the error text names the smallest span that fits.
 * Buffers are grown, never shrunk, and freed with the context.
 *
 * A by-product of a finished run like ookd_rx_bursts: nothing is launched or
 * allocated until it is asked for, it refuses what ookd_rx_pulse_hist refuses
 * with the same codes, one capture per call.  The same run, table, capture and
 * span_frames launch nothing; a new run, a new table (other margins, another
 * cleaned list) or another span makes a new result.  The getters are
 * OOKD_ERR_ARG while the last run's table has no result for that capture.  The
 * capture is read again through the pointer the run recorded: the residency
 * rule is that of ookd_rx_copy_bursts_*.  Frames are loaded sample by sample
 * (a burst's first sample is rarely 16-byte aligned), so no byte outside a
 * frame is touched: the capture's allocation may end at n.
 *
 * ookd_rx_burst_spectrum returns all 1024 doubles of one burst: the same
 * kernels over that burst alone, at the span the summaries were made with, so
 * it is the power_b[] the summary was taken from.  It needs the summaries of
 * that capture first (OOKD_ERR_ARG otherwise, and for burst >= num_bursts).
 *
 * Limits: this needs the signal above DC plus noise in the full band (with a
 * receiver's DC term a quarter-level signal may sit below the threshold that
 * clears it).  Not part of it: a spectrum per on-run, other frame lengths,
 * overlapping or zero-padded frames, more than one peak per burst (two
 * transmitters keying at once show as a lower share), interpolated peaks, shard
 * and pipelined runs, all captures of a batch in one launch.
 * ---------------------------------------------------------------------- */
typedef struct ookd_burst_spectrum {
    uint64_t frames;                /* F_b                                             */
    double total_power;             /* sum over all k of power_b[k]                    */
    double dc_power;                /* power_b[1023] + power_b[0] + power_b[1]         */
    double peak_power;              /* the largest power_b[k] over k in 2 .. 1022      */
    uint32_t peak_bin;              /* its k; ties go to the lowest k; 0 when frames = 0 */
    uint32_t reserved;
} ookd_burst_spectrum;

typedef struct ookd_burst_spectra_info {
    uint64_t num_bursts;
    uint64_t total_frames;          /* sum of F_b                                      */
    uint64_t spans;                 /* workgroups of the first kernel                  */
    uint64_t partial_rows;          /* rows of 1024 doubles kept for bursts across spans: 2 spans */
    uint32_t span_frames;           /* S as used                                       */
    uint32_t flags;                 /* OOKD_BURSTS_* of the table that was read        */
    float reduce_kernel_ms;         /* of kernel_ms: the second kernel and the keyed sum */
    uint32_t reserved;
} ookd_burst_spectra_info;

#define OOKD_BURST_SPECTRA_MIN_SPAN 32
#define OOKD_BURST_SPECTRA_MAX_ROWS 8192        /* 64 MiB of partial rows */

int ookd_rx_burst_spectra(ookd_rx *rx, uint32_t capture, uint32_t span_frames /* 0 = chosen */);
/* the ookd_rx_get_edges convention: *num_bursts receives the count, at most
 * `capacity` entries are stored, out may be NULL */
int ookd_rx_get_burst_spectra(const ookd_rx *rx, uint32_t capture, ookd_burst_spectrum *out,
                              uint64_t capacity, uint64_t *num_bursts);
int ookd_rx_get_keyed_spectrum(const ookd_rx *rx, uint32_t capture, ookd_spectrum_result *out);
int ookd_rx_get_burst_spectra_info(const ookd_rx *rx, uint32_t capture, ookd_burst_spectra_info *out);
int ookd_rx_burst_spectrum(ookd_rx *rx, uint32_t capture, uint64_t burst, ookd_spectrum_result *out);
/* HIP-event time of the last ookd_rx_burst_spectra pass about the last run (0: none, or nothing to launch) */
float ookd_rx_burst_spectra_kernel_ms(const ookd_rx *rx);
/* The span ookd_rx_burst_spectra takes for a cut of total_samples with span_frames = 0, and the check it makes
 * of a given one (host only): OOKD_OK and *span_used, OOKD_ERR_ARG, or OOKD_ERR_CAPACITY. */
int ookd_burst_spectra_span(uint64_t total_samples, uint32_t span_frames, uint32_t *span_used);

/* Carriers of a burst table's spectra, pure host code (no GPU needed).  The
 * rule, a contract:
 *   1. Burst b qualifies when frames >= 1, total_power - dc_power > 0 and
 *      peak_power >= min_share * (total_power - dc_power).
 *   2. weight[k] = the sum of peak_power over the qualifying bursts with
 *      peak_bin = k, added in burst order.
 *   3. Repeat, as ookd_suggest_carriers does: take the live bin of largest
 *      weight, ties going to the lowest k; stop when that weight is not > 0 or
 *      `capacity` carriers have been emitted; emit it -- its members are the
 *      qualifying bursts whose peak_bin lies within circular distance
 *      <= min_spacing_bins of it and is still live -- and kill those bins.
 *   4. Output is in decreasing weight.  carrier_of_burst[b] is the index in out,
 *      or -1 for a burst that does not qualify or was not reached before
 *      `capacity`.
 * A carrier's bursts and frames count its members, power is the sum of their
 * peak_power in burst order; nu is the centre of the emitted bin.
 * OOKD_BURST_MIN_SHARE, 1/8 of the power outside the DC bins: a tone on a bin
 * centre keeps 2/3 of its power in the peak bin under Hann, a tone midway
 * between two bins 0.48; the largest of 1021 bins of one frame of white noise
 * holds about ln(1021) / 1021 ~ 0.007 of the total, and P(one bin > 1/8 of the
 * total) is of the order e^-127.
 * 0, or OOKD_ERR_ARG for NULL s with num_bursts > 0, NULL count, NULL out with
 * capacity > 0, a negative or NaN min_share, or a peak_bin >= 1024. */
typedef struct ookd_burst_carrier {
    double nu;                      /* ookd_spectrum_bin_nu of the bin                 */
    int32_t bin;                    /* -512 .. 511                                     */
    uint32_t reserved;
    uint64_t bursts, frames;        /* members and their frames                        */
    double power;                   /* sum of the members' peak_power                  */
} ookd_burst_carrier;
#define OOKD_BURST_MIN_SHARE 0.125
int ookd_suggest_burst_carriers(const ookd_burst_spectrum *s, uint64_t num_bursts,
                                double min_share /* 0 = OOKD_BURST_MIN_SHARE */,
                                uint32_t min_spacing_bins /* 0 = OOKD_CARRIER_MIN_SPACING */,
                                ookd_burst_carrier *out, uint32_t capacity, uint32_t *count,
                                int32_t *carrier_of_burst /* [num_bursts] or NULL; -1 = none */);

/* ------------------------------------------------------------------------
 * Burst basebands: the filtered, decimated signal of every burst of the burst
 * table -- the slicer's own input, transmitter by transmitter.  The raw cut of
 * "Burst extraction" is wide-band input at the capture's rate: every carrier
 * list of a carrier context gets the same samples, and behind a filter of
 * decimation D it has D times the bytes that survive the channel filter.
 * Here the cut is the complex filter output y over the bursts' outputs, in a
 * carrier context through list k's own taps: transmitter k alone, at rate
 * fs / D, ready for a second decoder or a file.
 *
 * The contract.  Take capture (or carrier list) c of the context's last run
 * and the burst table the copy calls are about: the raw or the clean form,
 * whichever ookd_rx_bursts was last called with for this run.  D, n_out and n
 * are as in "Burst extraction".
 *   - The baseband table.  Burst b of the burst table covers outputs
 *     [first_output_b, first_output_b + num_outputs_b):
 *         first_output_b = ceil(first_sample_b / D)
 *         num_outputs_b  = ceil((first_sample_b + num_samples_b) / D) - first_output_b
 *     offset_b = the sum of num_outputs over the capture's bursts before b, and
 *     total_outputs = the sum over all of them.  In the terms of the burst rule
 *     that is [min(lo_b, m), min(hi_b, m)) with m = min(n_out, ceil(n / D)): the
 *     outputs whose newest input exists.  The table is a function of the burst
 *     table and D alone; a burst in the padding behind n has 0 outputs and
 *     stays in the table.  Bursts ascend and never overlap: two bursts with
 *     outputs lie at least one output apart.
 *   - The cut.  Element offset_b + i is y_j at output j = first_output_b + i:
 *     the float32 complex filter output exactly as "Pulse moments" defines y_j
 *     -- by the context's kind the untuned survey contract, the tuned survey
 *     contract with the list's own nu and taps, or the unpacked sample without
 *     a filter; inputs in front of the capture and at or beyond n are zero, the
 *     latter never loaded.
 *       OOKD_BASEBAND_CF32:     (re, im) as two float32, the bits of y_j.
 *       OOKD_BASEBAND_SC16Q11:  (s(re), s(im)) as two int16; s(v) is v * 2048
 *           formed in float32, a NaN taken as 0, clamped to [-32768, 32767],
 *           rounded to the nearest integer with ties to even.  The file reads
 *           back as an SC16Q11 capture at rate fs / D.
 *   - turn = nu D - rint(nu D), in cycles per output sample: where the list's
 *     carrier sits in the cut.  The tuned filter is a band-pass, not a mixer, so
 *     nothing is derotated: y advances by 2 pi nu D per output.  0 for an
 *     untuned context.  Informative, computed on the host in double.
 *   - Everything is an exact function of the burst table and the capture's
 *     bytes.  Every element has one writer: two calls leave the same bytes.
 *   - tile_outputs, tiles_total and tiles_filtered are as at ookd_run_levels: a
 *     tile is filtered when it holds an output of a burst.
 *
 * ookd_baseband_bursts is the table rule on the host, pure C++ (no GPU), over
 * one burst table.  It follows the ookd_rx_get_edges convention: at most
 * `capacity` entries are stored, out may be NULL, *total_outputs (may be NULL)
 * receives the cut's length.  OOKD_ERR_ARG for a NULL table that is not empty,
 * or D = 0.
 *
 * ookd_baseband_of is the contract on the host, pure C++ (no GPU), given the
 * filter's output y[n_out][2] and a baseband table: out receives the cut in
 * `format`.  OOKD_ERR_ARG for an unknown format, a NULL array that is not
 * empty, or a table that reaches beyond n_out; OOKD_ERR_CAPACITY, with nothing
 * written, when the table's outputs exceed capacity_outputs.
 *
 * The ookd_rx_* calls behave as ookd_rx_copy_bursts_* do.  They are about the
 * table ookd_rx_bursts was last called with for the last run and are
 * OOKD_ERR_ARG without one.  A by-product of a finished run: nothing is
 * launched or allocated before the first ookd_rx_burst_baseband_* call, which
 * builds the filter as the pulse levels' pass does and refuses, in the same
 * words, a filter whose history does not fit the kernel's LDS window.
 * ookd_rx_get_baseband_info and ookd_rx_get_baseband_bursts are host work over
 * the burst table.  capacity_outputs < total_outputs is OOKD_ERR_CAPACITY and
 * nothing is written; nothing at or beyond total_outputs elements is written
 * either.  d_out must be aligned to its element, 8 bytes for CF32 and 4 for
 * SC16Q11 (OOKD_ERR_ARG).  A cut of no outputs launches nothing.  The derived
 * table is kept per burst table and made again when ookd_rx_bursts has made
 * another.  ookd_rx_burst_baseband_host goes through a device buffer of exactly
 * the cut's size that it allocates and frees.  ookd_rx_baseband_kernel_ms is
 * the HIP-event time, on the context's stream, of the filtering kernel of the
 * last such call about the last run (0: none, or nothing to launch);
 * tiles_filtered is that kernel's count, 0 until it has run for this table.
 * The capture is read again through the pointer the run recorded: the
 * residency rule is that of ookd_rx_copy_bursts_*.
 *
 * Limits: no derotation to 0 Hz and no resampling to other rates (both need
 * an oscillator and a contract for it); shard and pipelined runs are refused,
 * as for every reader of the edge list; one capture per call.
 * ---------------------------------------------------------------------- */
enum {
    OOKD_BASEBAND_CF32 = 0,
    OOKD_BASEBAND_SC16Q11 = 1
};

typedef struct ookd_baseband_burst {
    uint64_t first_output;          /* output of the capture the burst begins at */
    uint64_t num_outputs;
    uint64_t offset;                /* element of the cut the burst begins at  */
} ookd_baseband_burst;

typedef struct ookd_baseband_info {
    uint64_t num_bursts;
    uint64_t total_outputs;
    uint64_t tiles_total;
    uint64_t tiles_filtered;        /* of the last pass about this table, else 0 */
    uint32_t tile_outputs;
    uint32_t decimation;            /* D                                       */
    double nu;                      /* the list's tuning, cycles per input sample */
    double turn;                    /* nu D - rint(nu D), cycles per output    */
} ookd_baseband_info;

int ookd_baseband_bursts(const ookd_burst *table, uint64_t num_bursts, uint64_t D,
                         ookd_baseband_burst *out, uint64_t capacity, uint64_t *total_outputs);
int ookd_baseband_of(const float *y, uint64_t n_out, const ookd_baseband_burst *table,
                     uint64_t num_bursts, uint32_t format, void *out, uint64_t capacity_outputs);
int ookd_rx_get_baseband_info(ookd_rx *rx, uint32_t capture, ookd_baseband_info *out);
int ookd_rx_get_baseband_bursts(ookd_rx *rx, uint32_t capture, ookd_baseband_burst *table,
                                uint64_t capacity, uint64_t *num_bursts);
int ookd_rx_burst_baseband_device(ookd_rx *rx, uint32_t capture, uint32_t format, void *d_out,
                                  uint64_t capacity_outputs);
int ookd_rx_burst_baseband_host(ookd_rx *rx, uint32_t capture, uint32_t format, void *out,
                                uint64_t capacity_outputs);
float ookd_rx_baseband_kernel_ms(const ookd_rx *rx);

/* ------------------------------------------------------------------------
 * Host side of a decoded message: payload bits -> per-field text -> stdout
 * text.  Replaces formatter_data_to_keyval
 * (src/formatter.c:715-739, field rules :425-573), rx_print
 * (src/ookiedokie.c:181-220) and, for the tx side, formatter_default_data /
 * formatter_keyval_to_data (formatter.c:793-846).  Pure host code: a few
 * fields per message.  The text is byte-identical to the reference's except
 * for the optional "Decode Timestamp" value (wall clock).
 * ---------------------------------------------------------------------- */
typedef struct ookd_formatter ookd_formatter;

enum {                              /* enum ookiedokie_rx_fmt, ookiedokie_cfg.h:41-45 */
    OOKD_RX_FMT_PRETTY = 0,
    OOKD_RX_FMT_CSV = 1
};

/* create_formatter (device.c:424-499) from the device's "fields" / "ts_mode". */
ookd_formatter *ookd_formatter_create(const ookd_device *device);
void ookd_formatter_free(ookd_formatter *f);
uint32_t ookd_formatter_num_fields(const ookd_formatter *f);
const char *ookd_formatter_field_name(const ookd_formatter *f, uint32_t field);
int ookd_formatter_ts_mode(const ookd_formatter *f); /* 0 none, 1 unix, 2 unix-frac,
                                                        3 datetime-24, 4 datetime-ampm */
/* The value text of one field of a payload (at most 79 characters, the
 * reference's char buf[80]). */
int ookd_formatter_field_to_str(const ookd_formatter *f, uint32_t field,
                                const uint8_t *payload, char *out, size_t capacity);
/* formatter_default_data: every field's "default" deposited into payload;
 * formatter_keyval_to_data for one (name, value) pair.  `len` = bytes at
 * payload, at least (num_bits + 7) / 8. */
int ookd_formatter_default_data(const ookd_formatter *f, uint8_t *payload, size_t len);
int ookd_formatter_set_field(const ookd_formatter *f, const char *name, const char *value,
                             uint8_t *payload, size_t len);

/* What rx_print writes for ONE keyval list = the `count` messages decoded
 * from one sdr_rx buffer (device_process appends them to the same list,
 * device.c:634-658).  snprintf convention: returns the number of characters
 * the full text has, stores at most capacity - 1 of them plus a NUL.
 * *first_print (CSV heading pending) is read and cleared like the
 * reference's flag. */
size_t ookd_print_record(const ookd_formatter *f, int rx_fmt, int *first_print,
                         const uint8_t *const *payloads, size_t count,
                         char *out, size_t capacity);
/* The whole stdout text of a run: messages grouped into records by the
 * buffer their OUTPUT_READY sample fell into, exactly as the reference's
 * per-buffer loop prints them (ookiedokie.c:279-286). */
size_t ookd_print_messages(const ookd_formatter *f, int rx_fmt, int *first_print,
                           const ookd_message *msgs, uint64_t num_messages,
                           uint32_t samples_per_buffer, uint32_t total_decimation,
                           char *out, size_t capacity);

/* ------------------------------------------------------------------------
 * Streaming FIR with the reference's call shape: replaces
 * fir_filter_and_decimate / fir_reset (src/fir.h:68-81): history carried
 * across calls, result independent of chunking.  Host pointers in and out
 * (PCIe-bound); exists so the fine-grained reference API has a GPU-backed
 * equivalent and for the FIR float parity tests.
 * ---------------------------------------------------------------------- */
typedef struct ookd_fir ookd_fir;
ookd_fir *ookd_fir_create(int32_t hip_device, const ookd_filter *filter,
                          size_t max_input, uint32_t flags);
void ookd_fir_reset(ookd_fir *f);
void ookd_fir_destroy(ookd_fir *f);
size_t ookd_fir_filter_and_decimate(ookd_fir *f, const ookd_complexf *input,
                                    size_t count, ookd_complexf *output);

/* ------------------------------------------------------------------------
 * Synthetic capture generator: envelope = the device's tx
 * state machine walk (sm_generate, src/state_machine.c:825-873) for
 * pseudo-random payloads, on-amplitude 1945 (device.c:675 0.95f,
 * complexf.h:93 truncation), per-message carrier phase, uniform integer
 * noise, occasional glitch pulses; counter-based PRNG so the same capture
 * can be produced on the device (fills HBM directly) and on the host.
 * ---------------------------------------------------------------------- */
typedef struct ookd_synth ookd_synth;

typedef struct ookd_synth_config {
    uint64_t seed;
    uint32_t sample_rate;           /* rate of the generated capture (Hz)    */
    uint32_t amplitude;             /* on level, default 1945                */
    uint32_t noise;                 /* +-noise LSB uniform, default 40       */
    uint32_t gap_min_us, gap_max_us;/* inter-message gap, default 4000..20000*/
    uint32_t glitch_every;          /* 1 message in N gets a glitch, 0 = off */
    uint32_t random_phase;          /* 0: I only (reference tx); 1: random   */
} ookd_synth_config;

ookd_synth *ookd_synth_create(const ookd_device *device,
                              const ookd_synth_config *cfg,
                              uint64_t num_samples);
void ookd_synth_free(ookd_synth *s);
uint64_t ookd_synth_num_messages(const ookd_synth *s);
/* Expected payloads in transmit order and the input-sample index at which
 * each message's waveform starts. */
int ookd_synth_message(const ookd_synth *s, uint64_t i, uint64_t *start_sample,
                       uint8_t *payload /* OOKD_MAX_PAYLOAD_BYTES */);
/* Fill samples [first, first+count) of the capture into host memory. */
int ookd_synth_fill_host(const ookd_synth *s, uint64_t first, uint64_t count,
                         int16_t *iq);
/* Same into device memory d_iq (which receives sample `first` at offset 0). */
int ookd_synth_fill_device(const ookd_synth *s, int32_t hip_device,
                           uint64_t first, uint64_t count, void *d_iq,
                           void *stream);

/* ------------------------------------------------------------------------
 * SDR backend: the five functions the reference's backend table binds
 * (SDR_PROTOTYPES / SDR_INTERFACE, src/sdr/supported_devices.h:32-48;
 * vtable src/sdr/sdr.c:50-122).  Registered as
 *     SDR_INTERFACE(hip_file, hip_file, "fs128_fs16_dec4")
 * it is a file handler for SC16Q11 captures like bladerf_file
 * (src/sdr/bladeRF_file.c) whose unpack runs on the GPU and whose handle
 * also keeps the raw capture resident in HBM for ookd_rx_process_device.
 * `cfg` is the reference's `const struct ookiedokie_cfg *`
 * (src/ookiedokie_cfg.h:50-91); only direction, sdr_args and
 * samples_per_buffer are read (as bladeRF_file.c:63,71,79 does).  The
 * struct layout is mirrored in ookd_host_cfg below for hosts that do not
 * include the reference header.
 * ---------------------------------------------------------------------- */
typedef struct ookd_host_cfg {
    const char *sdr_type;
    int direction;                  /* 0 = rx, 1 = tx (ookiedokie_cfg.h:32-36) */
    const char *sdr_args;           /* file name                              */
    unsigned int frequency, bandwidth, samplerate;
    int gain;
    const char *device;
    unsigned int tx_count, tx_delay_us;
    void *device_params;
    int rx_fmt;
    float rx_threshold;
    const char *rx_rec_filename, *rx_rec_type, *rx_filter, *rx_rec_dig;
    unsigned char rx_rec_input;     /* bool in the reference struct */
    unsigned int samples_per_buffer, num_buffers, num_transfers;
    unsigned int stream_timeout_ms, sync_timeout_ms;
    int verbosity;
} ookd_host_cfg;

/* Declared with the reference's own type names (forward declarations only), so that a translation unit
 * which also includes the reference's headers and says SDR_PROTOTYPES(hip_file) -- as sdr.c does
 * after INTEGRATION.md section 1 -- sees the very same declarations (tests/test_boundary.py compiles
 * exactly that).  struct complexf (src/complexf.h:31-34) and ookd_complexf are layout-identical;
 * a host without the reference headers passes (const struct ookiedokie_cfg *)&its_ookd_host_cfg. */
struct ookiedokie_cfg;
struct complexf;
void *sdr_hip_file_init(const struct ookiedokie_cfg *cfg);
void sdr_hip_file_deinit(void *handle);
int sdr_hip_file_rx(void *handle, struct complexf *samples, unsigned int count);
int sdr_hip_file_tx(void *handle, const struct complexf *samples,
                    unsigned int count);
int sdr_hip_file_flush(void *handle);
/* The capture's format follows its file name: `.cs8` / `.cu8` (any case) are 8-bit I,Q pairs as
 * OOKD_RX_SAMPLES_CS8 / _CU8 describe them, anything else is SC16Q11.  sdr_hip_file_rx unpacks an
 * 8-bit sample to v / 128.0f. */
/* Extra, beyond the vtable: the whole capture as a device pointer
 * (raw, in the file's format) for the fused path; loads the file to HBM on
 * first use. */
int sdr_hip_file_capture(void *handle, const void **d_iq,
                         uint64_t *num_samples);
/* 0, OOKD_RX_SAMPLES_CS8 or OOKD_RX_SAMPLES_CU8: what to OR into ookd_rx_config.flags for a
 * context that takes sdr_hip_file_capture's pointer. */
int sdr_hip_file_sample_flags(void *handle);

#ifdef __cplusplus
}
#endif

#endif /* OOKIEDOKIE_AMD_H */
