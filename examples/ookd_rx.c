/*
 * ookd_rx.c -- a C99 host on top of libookiedokie_amd.so: the shape of
 *     ookiedokie --rx hip_file -A <capture> -d <device> -F <filter> -s <rate> -f csv|pretty
 * reduced to what the library's boundary covers.  Shows the calls a maintainer
 * of the reference would make from ookiedokie_rx():
 * SDR backend handle -> capture resident in HBM -> fused demodulation ->
 * formatter / rx_print text on stdout, optional --rx-rec-dig file.
 *
 * Build (see tests/test_gpu_parity.py::test_c_host_example):
 *   gcc -std=c99 -Wall -Iinclude examples/ookd_rx.c -o ookd_rx \
 *       -Lookiedokie_amd/lib -lookiedokie_amd -Wl,-rpath,$PWD/ookiedokie_amd/lib
 *
 * ookd_rx [--threshold <value>|auto] [--tune <hz>|auto] [--min-on-us <us>] [--min-off-us <us>] [--levels] [--carriers]
 *         [--bursts <file> [--burst-pre-us <us>] [--burst-post-us <us>] [--burst-gap-us <us>] [--burst-carriers]]
 *         [--baseband <file.cf32|.sc16q11>]
 *         <capture.sc16q11|.cs8|.cu8> <device.json> <filter.json|none> <samplerate> [csv|pretty] [dig.csv]
 *
 * --threshold (anywhere on the line; default 0.1, the reference's --rx-threshold default): a number is used as
 * it is; `auto` surveys the capture's envelope levels first (ookd_survey_*, ookd_suggest_threshold), reports
 * the two levels and the threshold between them on stderr and decodes with that -- or, when the capture does
 * not show two levels, says so and exits non-zero without decoding.
 *
 * --tune <hz>: the carrier sits <hz> beside the capture's centre (a receiver tuned next to the transmitter to keep
 * its DC spike out of the way): the context filters with taps tuned to hz / samplerate cycles per sample
 * (ookd_rx_create_tuned).  Not together with `--threshold auto`: the survey filters with the real taps around
 * 0 Hz and would measure the DC term, not the carrier.
 *
 * --tune auto: one spectrum pass over the capture finds the carriers (ookd_spectrum_*, ookd_suggest_carriers);
 * every one is reported on stderr and the context is tuned to the strongest that is not the peak at DC.  Without
 * such a carrier a line says so and the decode is untuned.
 *
 * --min-on-us, --min-off-us: debounce.  "on" / "off" runs shorter than this many microseconds are deleted from the
 * edge list on the GPU as part of the run and the state machine decodes the cleaned list (ookd_rx_set_debounce; the
 * sample rate and the filter's decimation turn them into decimated samples, as in ookd_pulses): a glitch in front of
 * a message no longer costs the message.  The dig file stays the raw stream's.
 *
 * --levels: after the messages, one line per message on stderr, `level <capture> <sample> <dBFS>`: the lower median of
 * the peak powers of the message's last num_bits + 2 pulses (ookd_rx_get_run_peaks, ookd_message_levels) as
 * 10 log10(power), 0 dBFS being a full-scale carrier.  Of the list the state machine decoded: the cleaned one when a
 * debounce is on.  stdout is what it is without the option.
 *
 * --carriers: after the messages (and the level lines), one line per message on stderr,
 * `carrier <capture> <sample> <Hz> <dBFS> <coherence>`: which transmitter sent it.  The carrier is the phase step between
 * neighbouring filter outputs summed over the message's last num_bits + 2 pulses (ookd_rx_get_run_moments,
 * ookd_message_carriers), in Hz beside the capture's centre (in cycles per sample when the sample rate is given as 0),
 * on the branch nearest --tune; the level is the mean power of the same pulses as 10 log10(power); the coherence is 1 for
 * one clean carrier and less with noise or a second signal in the band.  Of the list the state machine decoded, as with
 * --levels.  stdout is what it is without the option.
 *
 * --bursts <file>: after the messages, the keyed stretches of the capture alone are cut out on the GPU
 * (ookd_rx_bursts, ookd_rx_copy_bursts_host) and written to <file> in the capture's own sample format: give it the
 * capture's extension and it reads back like the input (the hip_file backend picks the format from the extension).
 * <file>.idx gets one text line per burst, `first_sample num_samples offset`, in input samples.  On-runs whose gaps
 * are at most --burst-gap-us (default 20000) form one burst, which begins --burst-pre-us (default 500) in front of
 * its first rise and ends --burst-post-us (default 19500) behind its last fall; the gap is raised to pre + post when
 * it is given smaller.  Of the list the state machine decoded, as with --levels.  stdout is what it is without the option.
 *
 * --burst-carriers (with --bursts): a Welch spectrum of every burst of that table is summed on the GPU
 * (ookd_rx_burst_spectra) and ookd_suggest_burst_carriers groups the bursts by their peak bin -- which transmitter
 * keyed when, for a capture without a filter and a threshold above the noise of the whole band.  stderr gets a line
 * `burst carrier <k>: <Hz> Hz, <bursts> bursts, <frames> frames` per carrier and a line
 * `burst <first_sample> <num_samples> <carrier Hz|none> <share>` per burst, share = peak / (total - DC bins).  The
 * files and stdout are what they are without the option.
 *
 * --baseband <file>: after the messages, the filter's complex output over the same bursts is cut out on the GPU
 * (ookd_rx_burst_baseband_host) and written to <file>: float32 pairs for a name ending in .cf32, int16 pairs for one
 * ending in .sc16q11 -- which reads back as a capture at samplerate / decimation for a context without a filter; any
 * other extension is refused.  <file>.idx gets one text line per burst, `first_output num_outputs offset`, in
 * filter outputs.  With or without --bursts, and with the same --burst-*-us margins.  stderr names the cut's sample
 * rate and where the carrier sits in it: a tuned filter is a band-pass, not a mixer.  stdout is what it is without the
 * option.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "ookiedokie_amd.h"

static int fail(const char *what)
{
    fprintf(stderr, "%s: %s\n", what, ookd_last_error());
    return EXIT_FAILURE;
}

/* 10 log10(p) for p > 0 without libm (the build line above links none): p = m 2^e with m in [1, 2), and
 * ln m = 2 atanh((m - 1) / (m + 1)) by its series: |y| <= 1/3, so 20 terms leave less than 3^-41 */
static double decibel(double p)
{
    int e = 0;
    while (p >= 2.0) { p *= 0.5; ++e; }
    while (p < 1.0) { p *= 2.0; --e; }
    const double y = (p - 1.0) / (p + 1.0), y2 = y * y;
    double term = y, sum = 0.0;
    for (int k = 1; k < 40; k += 2) { sum += term / k; term *= y2; }
    const double ln2 = 0.69314718055994530942, ln10 = 2.30258509299404568402;
    return 10.0 * (2.0 * sum + e * ln2) / ln10;
}

int main(int argc, char **argv)
{
    /* --threshold <value>|auto is taken out of argv; what is left is positional, as before */
    float threshold = 0.1f;                 /* ookiedokie_cfg.h default */
    int threshold_auto = 0, tune_auto = 0, bad_option = 0, levels = 0, carriers = 0, burst_carriers = 0;
    double tune_hz = 0.0, min_on_us = 0.0, min_off_us = 0.0;
    double burst_pre_us = 500.0, burst_post_us = 19500.0, burst_gap_us = 20000.0;
    const char *bursts_path = NULL, *baseband_path = NULL;
    uint32_t baseband_format = OOKD_BASEBAND_CF32;
    int kept = 1;
    for (int i = 1; i < argc; ++i) {
        if (!strcmp(argv[i], "--threshold")) {
            char *end = NULL;
            if (++i >= argc) { bad_option = 1; break; }
            if (!strcmp(argv[i], "auto")) { threshold_auto = 1; continue; }
            threshold_auto = 0;
            threshold = strtof(argv[i], &end);
            if (end == argv[i] || *end != '\0') { bad_option = 1; break; }
        } else if (!strcmp(argv[i], "--tune")) {
            char *end = NULL;
            if (++i >= argc) { bad_option = 1; break; }
            if (!strcmp(argv[i], "auto")) { tune_auto = 1; tune_hz = 0.0; continue; }
            tune_auto = 0;
            tune_hz = strtod(argv[i], &end);
            if (end == argv[i] || *end != '\0') { bad_option = 1; break; }
        } else if (!strcmp(argv[i], "--min-on-us") || !strcmp(argv[i], "--min-off-us")) {
            char *end = NULL;
            double *us = !strcmp(argv[i], "--min-on-us") ? &min_on_us : &min_off_us;
            if (++i >= argc) { bad_option = 1; break; }
            *us = strtod(argv[i], &end);
            if (end == argv[i] || *end != '\0' || !(*us >= 0.0)) { bad_option = 1; break; }
        } else if (!strcmp(argv[i], "--burst-pre-us") || !strcmp(argv[i], "--burst-post-us") || !strcmp(argv[i], "--burst-gap-us")) {
            char *end = NULL;
            double *us = !strcmp(argv[i], "--burst-pre-us") ? &burst_pre_us : !strcmp(argv[i], "--burst-post-us") ? &burst_post_us : &burst_gap_us;
            if (++i >= argc) { bad_option = 1; break; }
            *us = strtod(argv[i], &end);
            if (end == argv[i] || *end != '\0' || !(*us >= 0.0)) { bad_option = 1; break; }
        } else if (!strcmp(argv[i], "--bursts")) {
            if (++i >= argc) { bad_option = 1; break; }
            bursts_path = argv[i];
        } else if (!strcmp(argv[i], "--baseband")) {
            if (++i >= argc) { bad_option = 1; break; }
            baseband_path = argv[i];
        } else if (!strcmp(argv[i], "--levels")) {
            levels = 1;
        } else if (!strcmp(argv[i], "--carriers")) {
            carriers = 1;
        } else if (!strcmp(argv[i], "--burst-carriers")) {
            burst_carriers = 1;
        } else {
            argv[kept++] = argv[i];
        }
    }
    argc = kept;
    if (burst_carriers && !bursts_path) {
        fprintf(stderr, "%s: --burst-carriers needs --bursts <file>: it is the spectra of that burst table\n", argv[0]);
        return EXIT_FAILURE;
    }
    if (argc < 5 || bad_option) {
        fprintf(stderr, "usage: %s [--threshold <value>|auto] [--tune <hz>|auto] [--min-on-us <us>] [--min-off-us <us>] "
                        "[--levels] [--carriers] [--bursts <file> [--burst-pre-us <us>] [--burst-post-us <us>] [--burst-gap-us <us>] "
                        "[--burst-carriers]] [--baseband <file.cf32|.sc16q11>] <capture.sc16q11|.cs8|.cu8> <device.json> <filter.json|none> <samplerate> [csv|pretty] [dig.csv]\n",
                argv[0]);
        return EXIT_FAILURE;
    }
    if (baseband_path) {
        const size_t len = strlen(baseband_path);
        if (len >= 5 && !strcmp(baseband_path + len - 5, ".cf32")) baseband_format = OOKD_BASEBAND_CF32;
        else if (len >= 8 && !strcmp(baseband_path + len - 8, ".sc16q11")) baseband_format = OOKD_BASEBAND_SC16Q11;
        else {
            fprintf(stderr, "%s: --baseband %s: the extension names the format, .cf32 or .sc16q11\n", argv[0], baseband_path);
            return EXIT_FAILURE;
        }
    }
    if (threshold_auto && (tune_auto || tune_hz != 0.0)) {
        char where[48];
        if (tune_auto) snprintf(where, sizeof where, "that --tune auto finds");
        else snprintf(where, sizeof where, "at %g Hz", tune_hz);
        fprintf(stderr, "%s: --threshold auto cannot be combined with --tune: the survey filters with the real taps "
                        "around 0 Hz and would measure the DC term, not the carrier %s; give a threshold\n",
                argv[0], where);
        return EXIT_FAILURE;
    }
    const int fmt = (argc > 5 && !strcmp(argv[5], "csv")) ? OOKD_RX_FMT_CSV : OOKD_RX_FMT_PRETTY;
    const unsigned rate = (unsigned) strtoul(argv[4], NULL, 0);
    int status = EXIT_FAILURE;

    ookd_host_cfg cfg;                      /* struct ookiedokie_cfg, field for field */
    memset(&cfg, 0, sizeof(cfg));
    cfg.sdr_type = "hip_file";
    cfg.direction = 0;
    cfg.sdr_args = argv[1];
    cfg.samplerate = rate;
    cfg.rx_threshold = threshold;
    cfg.samples_per_buffer = 8192;

    ookd_filter *filter = NULL;
    ookd_device *device = NULL;
    ookd_formatter *formatter = NULL;
    ookd_rx *rx = NULL;
    ookd_survey *survey = NULL;
    ookd_spectrum *spectrum = NULL;
    char *text = NULL;
    uint64_t *edges = NULL, *at = NULL;
    float *peaks = NULL, *level = NULL;
    ookd_run_moment *moments = NULL;
    ookd_message_carrier *sent = NULL;
    ookd_burst *bursts = NULL;
    ookd_baseband_burst *basebands = NULL;
    ookd_burst_spectrum *spectra = NULL;
    int32_t *carrier_of = NULL;
    void *cut = NULL;
    char *idx_path = NULL;

    void *sdr = sdr_hip_file_init((const struct ookiedokie_cfg *)&cfg);   /* same layout: see ookd_host_cfg */
    if (!sdr) return fail("sdr_hip_file_init");

    const void *d_iq = NULL;
    uint64_t n = 0;
    if (sdr_hip_file_capture(sdr, &d_iq, &n) != 0) { fail("sdr_hip_file_capture"); goto out; }

    if (strcmp(argv[3], "none")) {
        filter = ookd_filter_load(argv[3]);
        if (!filter) { fail("ookd_filter_load"); goto out; }
    }
    const unsigned decimation = filter ? ookd_filter_total_decimation(filter) : 1;
    device = ookd_device_load(argv[2], rate / decimation);      /* main.c:683 */
    if (!device) { fail("ookd_device_load"); goto out; }
    formatter = ookd_formatter_create(device);
    if (!formatter) { fail("ookd_formatter_create"); goto out; }

    if (threshold_auto) {                   /* the capture is in HBM already: one pass over it */
        ookd_level_hist hist;
        ookd_threshold_suggestion sug;
        survey = ookd_survey_create(0, filter, (uint32_t) sdr_hip_file_sample_flags(sdr), 1, NULL);
        if (!survey) { fail("ookd_survey_create"); goto out; }
        if (ookd_survey_device(survey, d_iq, 1, n, n) != 0) { fail("ookd_survey_device"); goto out; }
        if (ookd_survey_get_hist(survey, 0, &hist) != 0) { fail("ookd_survey_get_hist"); goto out; }
        if (ookd_suggest_threshold(&hist, &sug) != 0) { fail("ookd_suggest_threshold"); goto out; }
        if (!sug.found) {
            fprintf(stderr, "threshold auto: no two envelope levels in %llu samples (bins %u and %u, %.1f %% above "
                            "the split): nothing decoded\n", (unsigned long long) hist.samples, sug.off_bin,
                    sug.on_bin, 100.0 * sug.on_fraction);
            goto out;
        }
        fprintf(stderr, "threshold auto: %.6g (off level %.6g, on level %.6g, %.1f %% on, survey %.3f ms)\n",
                sug.threshold, sug.off_level, sug.on_level, 100.0 * sug.on_fraction,
                ookd_survey_kernel_ms(survey));
        cfg.rx_threshold = sug.threshold;
    }

    if (tune_auto) {                        /* the capture is in HBM already: one pass over it */
        static ookd_spectrum_result sp;
        ookd_carrier found[16];
        uint32_t nfound = 0, chosen = 0;
        double noise_floor = 0.0;
        spectrum = ookd_spectrum_create(0, (uint32_t) sdr_hip_file_sample_flags(sdr), 1, NULL);
        if (!spectrum) { fail("ookd_spectrum_create"); goto out; }
        if (ookd_spectrum_device(spectrum, d_iq, 1, n, n) != 0) { fail("ookd_spectrum_device"); goto out; }
        if (ookd_spectrum_get(spectrum, 0, &sp) != 0) { fail("ookd_spectrum_get"); goto out; }
        if (ookd_suggest_carriers(&sp, 0.0, 0, found, 16, &nfound, &noise_floor) != 0) {
            fail("ookd_suggest_carriers");
            goto out;
        }
        for (uint32_t i = 0; i < nfound; ++i)
            fprintf(stderr, "tune auto: carrier at %.6g Hz, %.4g x the floor%s\n", found[i].nu * (double) rate,
                    found[i].ratio, found[i].at_dc ? ", at DC" : "");
        while (chosen < nfound && found[chosen].at_dc) ++chosen;
        if (chosen < nfound) {
            tune_hz = found[chosen].nu * (double) rate;
            fprintf(stderr, "tune auto: tuned to %.6g Hz (%llu frames, spectrum %.3f ms)\n", tune_hz,
                    (unsigned long long) sp.frames, ookd_spectrum_kernel_ms(spectrum));
        } else {
            fprintf(stderr, "tune auto: no carrier beside DC in %llu frames (spectrum %.3f ms): decoding untuned\n",
                    (unsigned long long) sp.frames, ookd_spectrum_kernel_ms(spectrum));
        }
    }

    ookd_rx_config rc;
    memset(&rc, 0, sizeof(rc));
    rc.threshold = cfg.rx_threshold;
    rc.samples_per_buffer = cfg.samples_per_buffer;
    rc.max_samples = n ? n : 1;
    rc.flags = (uint32_t) sdr_hip_file_sample_flags(sdr);   /* a .cs8 / .cu8 capture: an 8-bit context */
    /* a tuned decode of a 2 x decimate-by-2 filter (the backend default) runs the fused kernel; without effect on
     * every other context */
    rc.flags |= OOKD_RX_TUNED_FIR2;
    ookd_tune tune;
    memset(&tune, 0, sizeof(tune));
    tune.nu = rate ? tune_hz / (double) rate : 0.0;     /* cycles per input sample; 0 = ookd_rx_create */
    rx = ookd_rx_create_tuned(&rc, filter, device, &tune);
    if (!rx) { fail("ookd_rx_create_tuned"); goto out; }
    {
        const double out_rate = (double) rate / (double) decimation;    /* the rate the state machine sees */
        const uint64_t min_on = (uint64_t) (min_on_us * 1e-6 * out_rate), min_off = (uint64_t) (min_off_us * 1e-6 * out_rate);
        if ((min_on > 1 || min_off > 1) && ookd_rx_set_debounce(rx, min_on, min_off) != 0) {
            fail("ookd_rx_set_debounce");
            goto out;
        }
    }

    if (ookd_rx_process_device(rx, d_iq, 1, n, n) != 0) { fail("ookd_rx_process_device"); goto out; }

    int first_print = 1;
    const uint64_t nmsg = ookd_rx_num_messages(rx);
    const ookd_message *msgs = ookd_rx_messages(rx);
    const size_t len = ookd_print_messages(formatter, fmt, &first_print, msgs, nmsg,
                                           cfg.samples_per_buffer, decimation, NULL, 0);
    text = malloc(len + 1);
    if (!text) goto out;
    first_print = 1;
    ookd_print_messages(formatter, fmt, &first_print, msgs, nmsg, cfg.samples_per_buffer, decimation,
                        text, len + 1);
    fputs(text, stdout);

    if (argc > 6 && ookd_rx_record_dig(rx, 0, argv[6]) != 0) { fail("ookd_rx_record_dig"); goto out; }

    ookd_rx_stats st;
    if (ookd_rx_get_stats(rx, &st) == 0) {
        ookd_clean_info ci;
        fprintf(stderr, "%llu samples, %llu edges, %llu messages, front end %.3f ms\n",
                (unsigned long long) st.input_samples, (unsigned long long) st.num_edges,
                (unsigned long long) st.num_messages, st.fir_kernel_ms);
        if (ookd_rx_get_clean_info(rx, 0, &ci) == 0) {      /* a debounced run: its cleaned list exists */
            fprintf(stderr, "debounce %llu / %llu samples: %llu pulses and %llu gaps deleted, %llu edges decoded\n",
                    (unsigned long long) ci.min_on, (unsigned long long) ci.min_off, (unsigned long long) ci.deleted[1],
                    (unsigned long long) ci.deleted[0], (unsigned long long) ci.edges_out);
        }
    }
    if (levels && nmsg) {                   /* one more pass over the capture, which is still in HBM */
        ookd_clean_info ci;
        const int clean = ookd_rx_get_clean_info(rx, 0, &ci) == 0;
        uint64_t ne = 0, nr = 0;
        if ((clean ? ookd_rx_get_clean_edges(rx, 0, NULL, 0, &ne) : ookd_rx_get_edges(rx, 0, NULL, 0, &ne)) != 0) {
            fail("ookd_rx_get_edges");
            goto out;
        }
        if ((clean ? ookd_rx_get_run_peaks_clean(rx, 0, NULL, 0, &nr) : ookd_rx_get_run_peaks(rx, 0, NULL, 0, &nr)) != 0) {
            fail("ookd_rx_get_run_peaks");
            goto out;
        }
        edges = malloc((ne + 1) * sizeof *edges);
        peaks = malloc((nr + 1) * sizeof *peaks);
        at = malloc(nmsg * sizeof *at);
        level = malloc(nmsg * sizeof *level);
        if (!edges || !peaks || !at || !level) goto out;
        if ((clean ? ookd_rx_get_clean_edges(rx, 0, edges, ne, &ne) : ookd_rx_get_edges(rx, 0, edges, ne, &ne)) != 0 ||
            (clean ? ookd_rx_get_run_peaks_clean(rx, 0, peaks, nr, &nr) : ookd_rx_get_run_peaks(rx, 0, peaks, nr, &nr)) != 0) {
            fail("ookd_rx_get_run_peaks");
            goto out;
        }
        for (uint64_t m = 0; m < nmsg; ++m) at[m] = msgs[m].sample;
        if (ookd_message_levels(edges, ne, peaks, nr, at, nmsg, ookd_device_num_bits(device) + 2, level) != 0) {
            fail("ookd_message_levels");
            goto out;
        }
        for (uint64_t m = 0; m < nmsg; ++m) {
            if (level[m] > 0.0f)
                fprintf(stderr, "level %u %llu %.2f\n", msgs[m].capture, (unsigned long long) at[m], decibel((double) level[m]));
            else
                fprintf(stderr, "level %u %llu -inf\n", msgs[m].capture, (unsigned long long) at[m]);
        }
    }
    if (carriers && nmsg) {                 /* the same pass with another epilogue: sums in the place of a maximum */
        ookd_clean_info ci;
        ookd_run_moments info;
        const int clean = ookd_rx_get_clean_info(rx, 0, &ci) == 0;
        uint64_t ne = 0, nr = 0;
        if (ookd_rx_get_stats(rx, &st) != 0) { fail("ookd_rx_get_stats"); goto out; }   /* n_out ends an open last run */
        if ((clean ? ookd_rx_get_clean_edges(rx, 0, NULL, 0, &ne) : ookd_rx_get_edges(rx, 0, NULL, 0, &ne)) != 0) {
            fail("ookd_rx_get_edges");
            goto out;
        }
        if ((clean ? ookd_rx_run_moments_clean(rx, 0, &info) : ookd_rx_run_moments(rx, 0, &info)) != 0) {
            fail("ookd_rx_run_moments");
            goto out;
        }
        nr = info.num_runs;
        free(edges);
        free(at);
        edges = malloc((ne + 1) * sizeof *edges);
        at = malloc(nmsg * sizeof *at);
        moments = malloc((nr + 1) * sizeof *moments);
        sent = malloc(nmsg * sizeof *sent);
        if (!edges || !at || !moments || !sent) goto out;
        if ((clean ? ookd_rx_get_clean_edges(rx, 0, edges, ne, &ne) : ookd_rx_get_edges(rx, 0, edges, ne, &ne)) != 0 ||
            (clean ? ookd_rx_get_run_moments_clean(rx, 0, moments, nr, &nr) : ookd_rx_get_run_moments(rx, 0, moments, nr, &nr)) != 0) {
            fail("ookd_rx_get_run_moments");
            goto out;
        }
        for (uint64_t m = 0; m < nmsg; ++m) at[m] = msgs[m].sample;
        if (ookd_message_carriers(edges, ne, st.decimated_samples, moments, nr, at, nmsg, ookd_device_num_bits(device) + 2,
                                  info.decimation, tune.nu, sent) != 0) {
            fail("ookd_message_carriers");
            goto out;
        }
        for (uint64_t m = 0; m < nmsg; ++m) {
            const double where = rate ? sent[m].carrier * (double) rate : sent[m].carrier;
            if (sent[m].mean_power > 0.0)
                fprintf(stderr, "carrier %u %llu %.*f %.2f %.4f\n", msgs[m].capture, (unsigned long long) at[m], rate ? 1 : 9, where,
                        decibel(sent[m].mean_power), sent[m].coherence);
            else
                fprintf(stderr, "carrier %u %llu %.*f -inf %.4f\n", msgs[m].capture, (unsigned long long) at[m], rate ? 1 : 9, where,
                        sent[m].coherence);
        }
    }
    if (bursts_path) {                      /* the table from the edge list, then the cut from the capture in HBM */
        ookd_clean_info ci;
        ookd_burst_info bi;
        const double out_rate = (double) rate / (double) decimation;
        const uint64_t pre = (uint64_t) (burst_pre_us * 1e-6 * out_rate), post = (uint64_t) (burst_post_us * 1e-6 * out_rate);
        uint64_t max_gap = (uint64_t) (burst_gap_us * 1e-6 * out_rate), nb = 0;
        FILE *f;
        if (max_gap < pre + post) max_gap = pre + post;
        if (ookd_rx_bursts(rx, pre, post, max_gap, ookd_rx_get_clean_info(rx, 0, &ci) == 0 ? OOKD_BURSTS_CLEAN : 0) != 0 ||
            ookd_rx_get_burst_info(rx, 0, &bi) != 0) {
            fail("ookd_rx_bursts");
            goto out;
        }
        bursts = malloc((bi.num_bursts + 1) * sizeof *bursts);
        cut = malloc((size_t) (bi.total_samples + 1) * bi.sample_bytes);
        idx_path = malloc(strlen(bursts_path) + 5);
        if (!bursts || !cut || !idx_path) goto out;
        if (ookd_rx_get_bursts(rx, 0, bursts, bi.num_bursts, &nb) != 0) { fail("ookd_rx_get_bursts"); goto out; }
        if (ookd_rx_copy_bursts_host(rx, 0, cut, bi.total_samples) != 0) { fail("ookd_rx_copy_bursts_host"); goto out; }
        f = fopen(bursts_path, "wb");
        if (!f || fwrite(cut, bi.sample_bytes, (size_t) bi.total_samples, f) != (size_t) bi.total_samples || fclose(f) != 0) {
            fprintf(stderr, "%s: cannot write\n", bursts_path);
            goto out;
        }
        strcpy(idx_path, bursts_path);
        strcat(idx_path, ".idx");
        f = fopen(idx_path, "w");
        if (!f) { fprintf(stderr, "%s: cannot write\n", idx_path); goto out; }
        for (uint64_t b = 0; b < nb; ++b)
            fprintf(f, "%llu %llu %llu\n", (unsigned long long) bursts[b].first_sample,
                    (unsigned long long) bursts[b].num_samples, (unsigned long long) bursts[b].offset);
        if (fclose(f) != 0) { fprintf(stderr, "%s: cannot write\n", idx_path); goto out; }
        fprintf(stderr, "bursts: %llu of %llu samples in %llu bursts (pre %llu, post %llu, gap %llu outputs; table %.3f ms, "
                        "copy %.3f ms)\n", (unsigned long long) bi.total_samples, (unsigned long long) n,
                (unsigned long long) nb, (unsigned long long) pre, (unsigned long long) post, (unsigned long long) max_gap,
                ookd_rx_bursts_kernel_ms(rx), ookd_rx_burst_copy_kernel_ms(rx));
        if (burst_carriers) {               /* a spectrum per burst of that table, and whose burst is whose */
            ookd_burst_carrier found[16];
            uint32_t count = 0;
            uint64_t ns = 0;
            spectra = malloc((size_t) (nb + 1) * sizeof *spectra);
            carrier_of = malloc((size_t) (nb + 1) * sizeof *carrier_of);
            if (!spectra || !carrier_of) goto out;
            if (ookd_rx_burst_spectra(rx, 0, 0) != 0 || ookd_rx_get_burst_spectra(rx, 0, spectra, nb, &ns) != 0 || ns != nb) {
                fail("ookd_rx_burst_spectra");
                goto out;
            }
            if (ookd_suggest_burst_carriers(spectra, nb, 0.0, 0, found, 16, &count, carrier_of) != 0) {
                fail("ookd_suggest_burst_carriers");
                goto out;
            }
            for (uint32_t k = 0; k < count; ++k)
                fprintf(stderr, "burst carrier %u: %.6g Hz, %llu bursts, %llu frames\n", k, found[k].nu * (double) rate,
                        (unsigned long long) found[k].bursts, (unsigned long long) found[k].frames);
            for (uint64_t b = 0; b < nb; ++b) {
                const double rest = spectra[b].total_power - spectra[b].dc_power;
                char hz[32];
                if (carrier_of[b] >= 0) snprintf(hz, sizeof hz, "%.6g", found[carrier_of[b]].nu * (double) rate);
                else snprintf(hz, sizeof hz, "none");
                fprintf(stderr, "burst %llu %llu %s %.4f\n", (unsigned long long) bursts[b].first_sample,
                        (unsigned long long) bursts[b].num_samples, hz, rest > 0.0 ? spectra[b].peak_power / rest : 0.0);
            }
            fprintf(stderr, "burst spectra: %.3f ms\n", ookd_rx_burst_spectra_kernel_ms(rx));
        }
    }
    if (baseband_path) {                    /* the filter's output over the same bursts: the same table (made once) */
        ookd_clean_info ci;
        ookd_baseband_info info;
        const double out_rate = (double) rate / (double) decimation;
        const uint64_t pre = (uint64_t) (burst_pre_us * 1e-6 * out_rate), post = (uint64_t) (burst_post_us * 1e-6 * out_rate);
        uint64_t max_gap = (uint64_t) (burst_gap_us * 1e-6 * out_rate), count = 0;
        const size_t element = baseband_format == OOKD_BASEBAND_CF32 ? 8 : 4;
        FILE *f;
        if (max_gap < pre + post) max_gap = pre + post;
        if (ookd_rx_bursts(rx, pre, post, max_gap, ookd_rx_get_clean_info(rx, 0, &ci) == 0 ? OOKD_BURSTS_CLEAN : 0) != 0) {
            fail("ookd_rx_bursts");
            goto out;
        }
        if (ookd_rx_get_baseband_info(rx, 0, &info) != 0) { fail("ookd_rx_get_baseband_info"); goto out; }
        free(cut);
        free(idx_path);
        basebands = malloc((size_t) (info.num_bursts + 1) * sizeof *basebands);
        cut = malloc((size_t) (info.total_outputs + 1) * element);
        idx_path = malloc(strlen(baseband_path) + 5);
        if (!basebands || !cut || !idx_path) goto out;
        if (ookd_rx_get_baseband_bursts(rx, 0, basebands, info.num_bursts, &count) != 0) { fail("ookd_rx_get_baseband_bursts"); goto out; }
        if (ookd_rx_burst_baseband_host(rx, 0, baseband_format, cut, info.total_outputs) != 0) { fail("ookd_rx_burst_baseband_host"); goto out; }
        f = fopen(baseband_path, "wb");
        if (!f || fwrite(cut, element, (size_t) info.total_outputs, f) != (size_t) info.total_outputs || fclose(f) != 0) {
            fprintf(stderr, "%s: cannot write\n", baseband_path);
            goto out;
        }
        strcpy(idx_path, baseband_path);
        strcat(idx_path, ".idx");
        f = fopen(idx_path, "w");
        if (!f) { fprintf(stderr, "%s: cannot write\n", idx_path); goto out; }
        for (uint64_t b = 0; b < count; ++b)
            fprintf(f, "%llu %llu %llu\n", (unsigned long long) basebands[b].first_output,
                    (unsigned long long) basebands[b].num_outputs, (unsigned long long) basebands[b].offset);
        if (fclose(f) != 0) { fprintf(stderr, "%s: cannot write\n", idx_path); goto out; }
        fprintf(stderr, "baseband: %llu outputs in %llu bursts at %.6g Hz, carrier at %.6g Hz (%.3f ms)\n",
                (unsigned long long) info.total_outputs, (unsigned long long) count, out_rate, info.turn * out_rate,
                ookd_rx_baseband_kernel_ms(rx));
    }
    status = EXIT_SUCCESS;

out:
    free(carrier_of);
    free(spectra);
    free(idx_path);
    free(cut);
    free(bursts);
    free(basebands);
    free(sent);
    free(moments);
    free(level);
    free(at);
    free(peaks);
    free(edges);
    free(text);
    ookd_rx_destroy(rx);
    ookd_survey_destroy(survey);
    ookd_spectrum_destroy(spectrum);
    ookd_formatter_free(formatter);
    ookd_device_free(device);
    ookd_filter_free(filter);
    sdr_hip_file_deinit(sdr);
    return status;
}
