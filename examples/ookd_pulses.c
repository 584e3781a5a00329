/*
 * ookd_pulses.c -- a C99 host on top of libookiedokie_amd.so that answers the third question about an unknown
 * capture, after "which carrier" and "which threshold" (examples/ookd_scan.c): which timings?  It runs the capture
 * through a context WITHOUT a device (filter, threshold, edges), asks for the run-length histogram of its edge list
 * (ookd_rx_pulse_hist, computed on the GPU) and prints the timing classes ookd_suggest_pulses groups it into: the
 * pulse and gap durations somebody who writes a device JSON has to type in.
 *
 * Build:
 *   gcc -std=c99 -Wall -Werror -Iinclude examples/ookd_pulses.c -o ookd_pulses \
 *       -Lookiedokie_amd/lib -lookiedokie_amd -Wl,-rpath,$PWD/ookiedokie_amd/lib
 *
 * ookd_pulses <capture.sc16q11|.cs8|.cu8> <filter.json|none> [--threshold <amplitude>] [--tune <hz>] [--rate <hz>]
 *             [--min-on-us <us>] [--min-off-us <us>] [--suggest-device <file.json>]
 *
 *   --threshold  slicer level, default 0.1 (ookd_scan's stderr names one per carrier)
 *   --tune       carrier offset in Hz (needs a filter), default 0
 *   --rate       sample rate of the capture, default 3000000; the table's microseconds and --tune depend on it
 *   --min-on-us, --min-off-us  drop glitches first: "on" / "off" runs shorter than this many microseconds are deleted
 *                from the edge list on the GPU (ookd_rx_clean_edges; --rate and the filter's decimation turn them into
 *                decimated samples), and the table and --suggest-device read the cleaned list.  Default 0: nothing
 *   --suggest-device  the fourth question, which device: count the capture's pulse/gap symbols and the distances
 *                between its sync symbols (ookd_rx_symbol_survey, on the GPU), print the device ookd_suggest_coding and
 *                ookd_suggest_device make of them and write it as a device JSON -- or say why there is none
 *
 * stdout: with a minimum, one line on what the cleaning deleted; then one line with the edge count and the two open runs, then per level ("on", "off") one line per class:
 * runs, mean length in decimated samples and in microseconds, and the range of lengths its bins cover.  With
 * --suggest-device one more line: the suggested device, or the reason for none.
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

static const char *reason_text(uint32_t reason)
{
    switch (reason) {
    case OOKD_CODING_KINDS: return "fewer than three kinds of pulse/gap symbols";
    case OOKD_CODING_NOT_DISTANCE: return "the two commonest symbols differ in their pulse: not distance coded";
    case OOKD_CODING_AMBIGUOUS: return "the two data gaps lie too close together for +-15 % windows";
    case OOKD_CODING_NO_SYNC: return "no third kind of symbol occurs at least twice: no sync";
    case OOKD_CODING_NO_FRAMES: return "no distance between syncs that half of the frames of 3 to 510 symbols share";
    case OOKD_CODING_TOO_LONG: return "more bits between two syncs than a message holds";
    default: return "unknown";
    }
}

/* symbols -> coding -> frames -> device; prints it and writes the JSON.  0 when the file was written. */
static int suggest_device(ookd_rx *rx, int clean, const ookd_pulse_suggestion *sug, double out_rate, const char *path)
{
    int (*const symbol_survey)(ookd_rx *, uint32_t, const ookd_symbol_table *, const ookd_symbol_roles *,
                               ookd_symbol_survey *) = clean ? ookd_rx_symbol_survey_clean : ookd_rx_symbol_survey;
    static ookd_symbol_table table;
    static ookd_symbol_roles roles;
    static ookd_symbol_survey survey;
    static char json[16384];
    ookd_coding coding;
    ookd_device_suggestion dev;
    if (ookd_symbol_table_from_pulses(sug, &table) != 0) return fail("ookd_symbol_table_from_pulses");
    if (symbol_survey(rx, 0, &table, NULL, &survey) != 0) return fail("ookd_rx_symbol_survey");
    if (ookd_suggest_coding(sug, &survey, &roles, &coding) != 0) return fail("ookd_suggest_coding");
    if (coding.found && symbol_survey(rx, 0, &table, &roles, &survey) != 0) return fail("ookd_rx_symbol_survey");
    if (ookd_suggest_device(sug, &survey, &coding, out_rate, &dev) != 0) return fail("ookd_suggest_device");
    if (!dev.found) {
        printf("no device suggested: %s\n", reason_text(dev.reason));
        return EXIT_FAILURE;
    }
    printf("device: %u bits; sync %llu us on, %llu us off; bit %llu us on, then %llu us (0) or %llu us (1); "
           "%llu syncs, %llu frames of 3 to 510 symbols, %llu of them clean and %u symbols long\n", dev.num_bits,
           (unsigned long long) dev.sync_on_us, (unsigned long long) dev.sync_off_us, (unsigned long long) dev.bit_on_us,
           (unsigned long long) dev.zero_off_us, (unsigned long long) dev.one_off_us, (unsigned long long) dev.num_syncs,
           (unsigned long long) dev.frames_counted, (unsigned long long) dev.frames_clean, dev.frame_symbols);
    size_t n = ookd_device_suggestion_json(&dev, "suggested", json, sizeof(json));
    if (n == 0 || n >= sizeof(json)) return fail("ookd_device_suggestion_json");
    FILE *f = fopen(path, "w");
    if (!f || fwrite(json, 1, n, f) != n) {
        fprintf(stderr, "cannot write %s\n", path);
        if (f) fclose(f);
        return EXIT_FAILURE;
    }
    fclose(f);
    printf("written to %s\n", path);
    return EXIT_SUCCESS;
}

int main(int argc, char **argv)
{
    double threshold = 0.1, tune_hz = 0.0, rate = 3000000.0, min_on_us = 0.0, min_off_us = 0.0;
    const char *suggest_path = NULL;
    int bad = argc < 3;
    for (int i = 3; i < argc && !bad; i += 2) {
        if (i + 1 >= argc) bad = 1;
        else if (!strcmp(argv[i], "--threshold")) threshold = strtod(argv[i + 1], NULL);
        else if (!strcmp(argv[i], "--tune")) tune_hz = strtod(argv[i + 1], NULL);
        else if (!strcmp(argv[i], "--rate")) rate = strtod(argv[i + 1], NULL);
        else if (!strcmp(argv[i], "--min-on-us")) min_on_us = strtod(argv[i + 1], NULL);
        else if (!strcmp(argv[i], "--min-off-us")) min_off_us = strtod(argv[i + 1], NULL);
        else if (!strcmp(argv[i], "--suggest-device")) suggest_path = argv[i + 1];
        else bad = 1;
    }
    if (bad || !(rate > 0.0) || !(threshold > 0.0) || !(min_on_us >= 0.0) || !(min_off_us >= 0.0)) {
        fprintf(stderr, "usage: %s <capture.sc16q11|.cs8|.cu8> <filter.json|none> [--threshold <amplitude>] "
                        "[--tune <hz>] [--rate <hz>] [--min-on-us <us>] [--min-off-us <us>] [--suggest-device <file.json>]\n",
                argv[0]);
        return EXIT_FAILURE;
    }
    int status = EXIT_FAILURE;

    ookd_host_cfg cfg;                      /* struct ookiedokie_cfg, field for field */
    memset(&cfg, 0, sizeof(cfg));
    cfg.sdr_type = "hip_file";
    cfg.direction = 0;
    cfg.sdr_args = argv[1];
    cfg.samplerate = (unsigned) rate;
    cfg.rx_threshold = (float) threshold;
    cfg.samples_per_buffer = 8192;

    ookd_filter *filter = NULL;
    ookd_rx *rx = NULL;
    static ookd_pulse_hist hist;
    static ookd_pulse_suggestion sug;

    void *sdr = sdr_hip_file_init((const struct ookiedokie_cfg *)&cfg);   /* same layout: see ookd_host_cfg */
    if (!sdr) return fail("sdr_hip_file_init");
    const void *d_iq = NULL;
    uint64_t n = 0;
    if (sdr_hip_file_capture(sdr, &d_iq, &n) != 0) { fail("sdr_hip_file_capture"); goto out; }

    unsigned decimation = 1;
    if (strcmp(argv[2], "none") != 0) {
        filter = ookd_filter_load(argv[2]);
        if (!filter) { fail("ookd_filter_load"); goto out; }
        decimation = ookd_filter_total_decimation(filter);
    }

    ookd_rx_config rc;
    memset(&rc, 0, sizeof(rc));
    rc.threshold = cfg.rx_threshold;
    rc.samples_per_buffer = cfg.samples_per_buffer;
    rc.max_samples = n ? n : 1;
    rc.max_captures = 1;
    rc.flags = (uint32_t) sdr_hip_file_sample_flags(sdr) | OOKD_RX_NO_PIPELINE;
    ookd_tune tune;
    memset(&tune, 0, sizeof(tune));
    tune.nu = tune_hz / rate;
    rx = ookd_rx_create_tuned(&rc, filter, NULL /* no device: edges only */, &tune);
    if (!rx) { fail("ookd_rx_create_tuned"); goto out; }
    if (ookd_rx_process_device(rx, d_iq, 1, n, n) != 0) { fail("ookd_rx_process_device"); goto out; }
    const double out_rate = rate / (double) decimation;     /* the rate the state machine sees (main.c:683) */
    const uint64_t min_on = (uint64_t) (min_on_us * 1e-6 * out_rate), min_off = (uint64_t) (min_off_us * 1e-6 * out_rate);
    const int clean = min_on > 1 || min_off > 1;
    if (clean) {
        ookd_clean_info info;
        if (ookd_rx_clean_edges(rx, min_on, min_off) != 0) { fail("ookd_rx_clean_edges"); goto out; }
        if (ookd_rx_get_clean_info(rx, 0, &info) != 0) { fail("ookd_rx_get_clean_info"); goto out; }
        printf("cleaned: on-runs under %llu and off-runs under %llu samples deleted, %llu and %llu of them; %llu of %llu "
               "edges stay\n", (unsigned long long) min_on, (unsigned long long) min_off, (unsigned long long) info.deleted[1],
               (unsigned long long) info.deleted[0], (unsigned long long) info.edges_out, (unsigned long long) info.edges_in);
    }
    if ((clean ? ookd_rx_pulse_hist_clean : ookd_rx_pulse_hist)(rx, 0, &hist) != 0) { fail("ookd_rx_pulse_hist"); goto out; }
    if (ookd_suggest_pulses(&hist, out_rate, &sug) != 0) { fail("ookd_suggest_pulses"); goto out; }

    printf("%llu edges in %llu samples at %.6g Hz; before the first edge %llu samples, after the last %llu (%s)\n",
           (unsigned long long) hist.num_edges, (unsigned long long) hist.samples, out_rate,
           (unsigned long long) hist.open_head, (unsigned long long) hist.open_tail, hist.tail_level ? "on" : "off");
    for (int level = 1; level >= 0; --level) {
        printf("%s-runs: %llu in %u classes%s\n", level ? "on" : "off", (unsigned long long) hist.runs[level],
               sug.num_classes[level], sug.found ? "" : (level ? "" : "  (no repeating timing on both levels)"));
        printf("  %10s %14s %12s   %s\n", "runs", "mean samples", "mean us", "range samples (us)");
        for (uint32_t c = 0; c < sug.num_classes[level]; ++c) {
            const ookd_pulse_class *k = &sug.classes[level][c];
            printf("  %10llu %14.2f %12.2f   %llu .. %llu (%.2f .. %.2f)\n", (unsigned long long) k->runs, k->mean,
                   k->mean_us, (unsigned long long) k->lower, (unsigned long long) k->upper, k->lower_us, k->upper_us);
        }
        if (sug.dropped_runs[level])
            printf("  %llu runs in further classes not listed\n", (unsigned long long) sug.dropped_runs[level]);
    }
    status = suggest_path ? suggest_device(rx, clean, &sug, out_rate, suggest_path) : EXIT_SUCCESS;

out:
    ookd_rx_destroy(rx);
    ookd_filter_free(filter);
    sdr_hip_file_deinit(sdr);
    return status;
}
