/*
 * ookd_scan.c -- a C99 host on top of libookiedokie_amd.so that uses the whole chain on one capture whose
 * carriers are NOT at its centre:
 *     spectrum (ookd_spectrum_*, ookd_suggest_carriers)        which carriers are there
 *  -> ONE carriers survey (ookd_survey_create_carriers; ookd_suggest_threshold per carrier)
 *                                                              which threshold does each carrier want
 *  -> per device ONE carrier context (ookd_rx_create_carriers) that decodes every carrier at its own threshold in
 *     one pass over the capture
 *  -> formatter / rx_print text on stdout.
 * The capture is loaded once and stays in HBM; every pass reads it there.
 *
 * Build:
 *   gcc -std=c99 -Wall -Werror -Iinclude examples/ookd_scan.c -o ookd_scan \
 *       -Lookiedokie_amd/lib -lookiedokie_amd -Wl,-rpath,$PWD/ookiedokie_amd/lib
 *
 * ookd_scan [--survey-stride N] <capture.sc16q11|.cs8|.cu8> <samplerate> <filter.json> <device.json>
 *           [<device.json> ...] [csv|pretty]
 * --survey-stride N: the survey counts every N-th filter output (a power of two, 1 .. 64; default 1, every output;
 * N > 1 needs a one-stage filter without decimation, or two decimate-by-2 stages of <= 16 and <= 32 taps such as
 * the backend default fs128_fs16_dec4).
 *
 * stderr: one line per carrier -- the peak at DC (the receiver's own) is reported and skipped, every other one
 * with its threshold and the two envelope levels, or "no two envelope levels" --, and one line per carrier and
 * device that decoded messages.  stdout: those messages, block by block as ookd_rx prints them (a CSV block
 * starts with its device's heading).  Without a carrier beside DC a
 * line says so, stdout stays empty and the exit status is 0.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "ookiedokie_amd.h"

#define MAX_CARRIERS 8
#define MAX_DEVICES 16

static int fail(const char *what)
{
    fprintf(stderr, "%s: %s\n", what, ookd_last_error());
    return EXIT_FAILURE;
}

int main(int argc, char **argv)
{
    int fmt = OOKD_RX_FMT_PRETTY;
    uint32_t survey_stride = 1;
    for (int i = 1; i + 1 < argc; ++i) {        /* the option may stand anywhere; it is taken out of argv */
        if (strcmp(argv[i], "--survey-stride")) continue;
        survey_stride = (uint32_t) strtoul(argv[i + 1], NULL, 0);
        for (int j = i; j + 2 < argc; ++j) argv[j] = argv[j + 2];
        argc -= 2;
        break;
    }
    if (argc > 1 && (!strcmp(argv[argc - 1], "csv") || !strcmp(argv[argc - 1], "pretty"))) {
        fmt = !strcmp(argv[argc - 1], "csv") ? OOKD_RX_FMT_CSV : OOKD_RX_FMT_PRETTY;
        --argc;
    }
    const unsigned rate = argc > 2 ? (unsigned) strtoul(argv[2], NULL, 0) : 0;
    const int ndev = argc - 4;
    if (argc < 5 || ndev > MAX_DEVICES || rate == 0) {
        fprintf(stderr, "usage: %s [--survey-stride N] <capture.sc16q11|.cs8|.cu8> <samplerate> <filter.json> "
                        "<device.json> [<device.json> ... up to %d] [csv|pretty]\n", argv[0], MAX_DEVICES);
        return EXIT_FAILURE;
    }
    int status = EXIT_FAILURE;

    ookd_host_cfg cfg;                      /* struct ookiedokie_cfg, field for field */
    memset(&cfg, 0, sizeof(cfg));
    cfg.sdr_type = "hip_file";
    cfg.direction = 0;
    cfg.sdr_args = argv[1];
    cfg.samplerate = rate;
    cfg.rx_threshold = 0.1f;
    cfg.samples_per_buffer = 8192;

    ookd_filter *filter = NULL;
    ookd_device *device[MAX_DEVICES] = { NULL };
    ookd_formatter *formatter[MAX_DEVICES] = { NULL };
    ookd_spectrum *spectrum = NULL;
    ookd_survey *survey = NULL;
    ookd_rx *rx = NULL;
    ookd_message *msgs[MAX_DEVICES] = { NULL };     /* per device: the messages of all carriers */
    uint64_t nmsgs[MAX_DEVICES] = { 0 };
    char *text = NULL;

    void *sdr = sdr_hip_file_init((const struct ookiedokie_cfg *)&cfg);   /* same layout: see ookd_host_cfg */
    if (!sdr) return fail("sdr_hip_file_init");
    const uint32_t sample_flags = (uint32_t) sdr_hip_file_sample_flags(sdr);

    const void *d_iq = NULL;
    uint64_t n = 0;
    if (sdr_hip_file_capture(sdr, &d_iq, &n) != 0) { fail("sdr_hip_file_capture"); goto out; }

    filter = ookd_filter_load(argv[3]);
    if (!filter) { fail("ookd_filter_load"); goto out; }
    const unsigned decimation = ookd_filter_total_decimation(filter);
    for (int d = 0; d < ndev; ++d) {
        device[d] = ookd_device_load(argv[4 + d], rate / decimation);   /* main.c:683 */
        if (!device[d]) { fail("ookd_device_load"); goto out; }
        formatter[d] = ookd_formatter_create(device[d]);
        if (!formatter[d]) { fail("ookd_formatter_create"); goto out; }
    }

    /* 1. which carriers */
    static ookd_spectrum_result sp;
    ookd_carrier found[MAX_CARRIERS];
    uint32_t nfound = 0, beside = 0;
    spectrum = ookd_spectrum_create(0, sample_flags, 1, NULL);
    if (!spectrum) { fail("ookd_spectrum_create"); goto out; }
    if (ookd_spectrum_device(spectrum, d_iq, 1, n, n) != 0) { fail("ookd_spectrum_device"); goto out; }
    if (ookd_spectrum_get(spectrum, 0, &sp) != 0) { fail("ookd_spectrum_get"); goto out; }
    if (ookd_suggest_carriers(&sp, 0.0, 0, found, MAX_CARRIERS, &nfound, NULL) != 0) {
        fail("ookd_suggest_carriers");
        goto out;
    }
    for (uint32_t c = 0; c < nfound; ++c) {
        if (found[c].at_dc)
            fprintf(stderr, "carrier %+.6g Hz: at DC, skipped\n", found[c].nu * (double) rate);
        else
            ++beside;
    }
    if (!beside) {
        fprintf(stderr, "no carrier beside DC in %llu frames: nothing decoded\n", (unsigned long long) sp.frames);
        status = EXIT_SUCCESS;
        goto out;
    }

    ookd_rx_carrier carrier[MAX_CARRIERS];  /* the carriers that have a threshold, in the order they were found */
    double carrier_hz[MAX_CARRIERS];
    uint32_t ncar = 0;
    memset(carrier, 0, sizeof(carrier));
    /* 2. which threshold: the envelope every carrier has behind the filter tuned to it -- ONE carriers survey, one
     * pass over the capture for all of them, counting every survey_stride-th output */
    ookd_tune tunes[MAX_CARRIERS];
    uint32_t ntunes = 0;
    memset(tunes, 0, sizeof(tunes));
    for (uint32_t c = 0; c < nfound; ++c)
        if (!found[c].at_dc) tunes[ntunes++].nu = found[c].nu;
    /* (OOKD_RX_TUNED_FIR2: a 2 x decimate-by-2 filter, the backend default, is surveyed by the fused kernel too) */
    survey = ookd_survey_create_carriers(0, filter, sample_flags | OOKD_RX_TUNED_FIR2, 1, NULL, tunes, ntunes,
                                         survey_stride);
    if (!survey) { fail("ookd_survey_create_carriers"); goto out; }
    if (ookd_survey_device(survey, d_iq, 1, n, n) != 0) { fail("ookd_survey_device"); goto out; }
    for (uint32_t k = 0; k < ntunes; ++k) {
        const double hz = tunes[k].nu * (double) rate;
        ookd_level_hist hist;
        ookd_threshold_suggestion sug;
        if (ookd_survey_get_carrier_hist(survey, 0, k, &hist) != 0) { fail("ookd_survey_get_carrier_hist"); goto out; }
        if (ookd_suggest_threshold(&hist, &sug) != 0) { fail("ookd_suggest_threshold"); goto out; }
        if (!sug.found) {
            fprintf(stderr, "carrier %+.6g Hz: no two envelope levels\n", hz);
            continue;
        }
        fprintf(stderr, "carrier %+.6g Hz: threshold %.6g (off %.6g, on %.6g)\n", hz, sug.threshold, sug.off_level,
                sug.on_level);
        carrier[ncar].nu = tunes[k].nu;
        carrier[ncar].threshold = sug.threshold;
        carrier_hz[ncar] = hz;
        ++ncar;
    }
    ookd_survey_destroy(survey);
    survey = NULL;

    /* 3. decode: per device ONE carrier context, which reads the capture once for all carriers.  Its messages come
     * in carrier order, ookd_message.capture being the carrier index. */
    for (int d = 0; d < ndev && ncar; ++d) {
        ookd_rx_config rc;
        memset(&rc, 0, sizeof(rc));
        rc.samples_per_buffer = cfg.samples_per_buffer;
        rc.max_samples = n ? n : 1;
        /* (a 2 x decimate-by-2 filter, the backend default, runs the fused tuned kernel once per carrier) */
        rc.flags = sample_flags | OOKD_RX_TUNED_FIR2;
        rx = ookd_rx_create_carriers(&rc, filter, device[d], carrier, ncar);
        if (!rx) { fail("ookd_rx_create_carriers"); goto out; }
        if (ookd_rx_process_device(rx, d_iq, 1, n, n) != 0) { fail("ookd_rx_process_device"); goto out; }
        nmsgs[d] = ookd_rx_num_messages(rx);
        if (nmsgs[d]) {
            msgs[d] = malloc(nmsgs[d] * sizeof(ookd_message));
            if (!msgs[d]) goto out;
            memcpy(msgs[d], ookd_rx_messages(rx), nmsgs[d] * sizeof(ookd_message));
        }
        ookd_rx_destroy(rx);
        rx = NULL;
    }
    /* one block per carrier and device, carrier by carrier */
    for (uint32_t c = 0; c < ncar; ++c) {
        for (int d = 0; d < ndev; ++d) {
            uint64_t first = 0, nmsg = 0;
            while (first < nmsgs[d] && msgs[d][first].capture < c) ++first;
            while (first + nmsg < nmsgs[d] && msgs[d][first + nmsg].capture == c) ++nmsg;
            if (!nmsg) continue;
            int fp = 1;                 /* every block has its device's own CSV heading, as ookd_rx prints it */
            const size_t len = ookd_print_messages(formatter[d], fmt, &fp, msgs[d] + first, nmsg, cfg.samples_per_buffer,
                                                   decimation, NULL, 0);
            text = malloc(len + 1);
            if (!text) goto out;
            fp = 1;
            ookd_print_messages(formatter[d], fmt, &fp, msgs[d] + first, nmsg, cfg.samples_per_buffer, decimation,
                                text, len + 1);
            fprintf(stderr, "carrier %+.6g Hz, %s: %llu messages\n", carrier_hz[c], ookd_device_name(device[d]),
                    (unsigned long long) nmsg);
            fputs(text, stdout);
            free(text);
            text = NULL;
        }
    }
    status = EXIT_SUCCESS;

out:
    free(text);
    ookd_rx_destroy(rx);
    ookd_survey_destroy(survey);
    ookd_spectrum_destroy(spectrum);
    for (int d = 0; d < MAX_DEVICES; ++d) {
        free(msgs[d]);
        ookd_formatter_free(formatter[d]);
        ookd_device_free(device[d]);
    }
    ookd_filter_free(filter);
    sdr_hip_file_deinit(sdr);
    return status;
}
