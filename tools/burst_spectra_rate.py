"""Time of the burst spectra (ookd_rx_burst_spectra) beside what a user can do without them on the same run: cut the
bursts out (ookd_rx_copy_bursts_device) and run the carrier survey (ookd_spectrum_device) over the cut as one capture.

    python tools/burst_spectra_rate.py [--log2-samples 32] [--steps 12] [--warmup 2] [--out profiles/burst_spectra_rate.json]

The capture and the margins are those of tools/bursts_rate.py: synthetic p3l-nexa2012 traffic made like bench.py's
north_star capture (2^32 samples) through fs32_fs4 and the p3l-nexa2012 decoder at threshold 0.1; the device's margins
(200 us in front, its longest timeout and 600 us behind, max_gap = pre + post) and tight ones (200 us either side).
Every step is a fresh run and then, one at a time on the device in one process: the table pass, the burst spectra --
the first ookd_rx_burst_spectra after the run, the one that launches --, the copy of the cut into device memory, and
the Welch spectrum of that cut.  All times are HIP events.

Recorded per cut: the bursts, the frames, the span chosen, the partial rows, the medians of the times, and of the burst
spectra's time the part behind the first kernel (the rows of the bursts that cross spans and the keyed sum).
One condition, on the device's margins, against a neighbour and never against this code itself; the tool exits with
status 1 when it fails:
    spectra_ms.median <= 2 spectrum_ms.median: the same frames, at unaligned starts, with two rows per span and the
    serial row loop of the long bursts on top.
The tight margins (hundreds of thousands of bursts of about two frames, the per-burst epilogue at work) are recorded
and not judged.  The kernel has one load form (sample by sample), so there is no second one to record.
"""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
RATE, SPB, THRESHOLD, SEED = 3000000, 8192, 0.1, 0x00C0FFEE + 22
PRE_US, POST_EXTRA_US = 200, 600
TIGHT_US = 200


def summary(v):
    v = sorted(v)
    m = len(v) // 2
    med = v[m] if len(v) % 2 else 0.5 * (v[m - 1] + v[m])
    return {"median": round(med, 5), "min": round(v[0], 5), "max": round(v[-1], 5)}


def longest_timeout_us(path):
    with open(path) as f:
        states = json.load(f)["device"]["states"]
    return max(int(s.get("timeout_us", 0)) for s in states)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2-samples", type=int, default=32)
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(HERE, "..", "profiles", "burst_spectra_rate.json"))
    args = ap.parse_args()
    if args.steps < 12:
        raise SystemExit("--steps: the median is taken over at least 12 calls")

    sys.path.insert(0, os.path.abspath(os.path.join(HERE, "..")))
    import torch
    import ookiedokie_amd as ok
    golden = os.path.join(HERE, "..", "tests", "golden")
    n = 1 << args.log2_samples
    device_json = os.path.join(golden, "devices", "p3l-nexa2012.json")

    flt = ok.Filter.load(os.path.join(golden, "filters", "fs32_fs4.json"))
    D = flt.total_decimation
    dev = ok.Device.load(device_json, RATE // D)
    out_rate = RATE // D
    pre = PRE_US * out_rate // 1000000
    post = (longest_timeout_us(device_json) + POST_EXTRA_US) * out_rate // 1000000
    max_gap = pre + post
    syn = ok.Synth(dev, n, seed=SEED, sample_rate=RATE)
    cap = torch.empty(2 * n + 64, dtype=torch.int16, device="cuda")
    syn.fill_device(cap.data_ptr())
    torch.cuda.synchronize()
    rx = ok.Receiver(flt, dev, max_samples=n, threshold=THRESHOLD, samples_per_buffer=SPB)
    spectrum = ok.Spectrum()

    def measure(pre, post, max_gap):
        # one run ahead of the timed ones sizes the cut's buffer
        rx.process_device(cap.data_ptr(), n)
        info = rx.bursts(pre, post, max_gap)[0]
        total = info["total_samples"]
        cut = torch.empty(2 * max(total, 1) + 64, dtype=torch.int16, device="cuda")
        t = {k: [] for k in ("spectra_ms", "spectra_reduce_ms", "bursts_ms", "copy_ms", "spectrum_ms", "fir_kernel_ms")}
        sp = None
        for k in range(args.warmup + args.steps):
            rx.process_device(cap.data_ptr(), n)
            st = rx.raw_stats()
            info = rx.bursts(pre, post, max_gap)[0]
            assert info["total_samples"] == total
            sp = rx.burst_spectra(0)
            spectra_ms = rx.burst_spectra_kernel_ms
            rx.burst_samples_device(0, cut.data_ptr(), total)
            spectrum.spectrum_device(cut.data_ptr(), total)
            if k >= args.warmup:
                t["spectra_ms"].append(spectra_ms)
                t["spectra_reduce_ms"].append(sp["reduce_kernel_ms"])
                t["bursts_ms"].append(rx.bursts_kernel_ms)
                t["copy_ms"].append(rx.burst_copy_kernel_ms)
                t["spectrum_ms"].append(spectrum.kernel_ms)
                t["fir_kernel_ms"].append(float(st.fir_kernel_ms))
        del cut
        s = {k: summary(v) for k, v in t.items()}
        frames = int(sp["total_frames"])
        carriers, _ = ok.suggest_burst_carriers(sp)
        return {
            "samples": n, "edges": int(st.num_edges), "messages": int(st.num_messages), "front_form": int(st.front_form),
            "pre": pre, "post": post, "max_gap": max_gap,
            "num_bursts": info["num_bursts"], "total_samples": total, "cut_share": round(total / n, 5),
            "total_frames": frames, "frames_of_the_cut_as_one_capture": total // 1024,
            "longest_burst_frames": int(sp["frames"].max()) if sp["num_bursts"] else 0,
            "bursts_without_frames": int((sp["frames"] == 0).sum()),
            "span_frames": sp["span_frames"], "spans": sp["spans"], "partial_rows": sp["partial_rows"],
            "partial_row_bytes": sp["partial_rows"] * 8192, "keyed_row_bytes": sp["spans"] * 8192,
            "load_form": "sample by sample",
            "burst_carriers": [[c.bin, c.bursts, c.frames] for c in carriers],
            "times": s,
            "spectra_over_spectrum": round(s["spectra_ms"]["median"] / s["spectrum_ms"]["median"], 4),
            "spectra_over_copy": round(s["spectra_ms"]["median"] / s["copy_ms"]["median"], 4),
            "reduce_share_of_spectra": round(s["spectra_reduce_ms"]["median"] / s["spectra_ms"]["median"], 4),
            "spectra_gb_per_s_read": round(frames * 4096 / 1e9 / (s["spectra_ms"]["median"] * 1e-3), 1),
            "spectrum_gb_per_s_read": round((total // 1024) * 4096 / 1e9 / (s["spectrum_ms"]["median"] * 1e-3), 1),
        }

    a = measure(pre, post, max_gap)
    holds = a["times"]["spectra_ms"]["median"] <= 2.0 * a["times"]["spectrum_ms"]["median"]
    a.update(condition="spectra_ms.median <= 2 spectrum_ms.median", condition_holds=bool(holds))
    tight = TIGHT_US * out_rate // 1000000
    b = measure(tight, tight, 2 * tight)
    b.update(note="tight margins: recorded, not judged")
    rx.close()
    spectrum.close()

    out = {
        "steps": args.steps, "warmup": args.warmup,
        "command": "python tools/burst_spectra_rate.py --log2-samples %d --steps %d --warmup %d" % (args.log2_samples, args.steps, args.warmup),
        "filter": "fs32_fs4", "device": "p3l-nexa2012", "threshold": THRESHOLD,
        "spectra_ms": "ookd_rx_burst_spectra_kernel_ms: hipMemsetAsync of the results + the three kernels",
        "spectra_reduce_ms": "of spectra_ms, what follows the first kernel: the rows of the bursts across spans, the keyed sum",
        "bursts_ms": "ookd_rx_bursts_kernel_ms: the table pass",
        "copy_ms": "ookd_rx_burst_copy_kernel_ms: the copy kernel of the same cut into device memory",
        "spectrum_ms": "ookd_spectrum_kernel_ms of ookd_spectrum_device over that cut as one capture (16-byte aligned)",
        "fir_kernel_ms": "the run's front end (ookd_rx_stats.fir_kernel_ms)",
        "device_margins": a, "tight_margins": b,
    }
    path = os.path.abspath(args.out)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(out))
    if not holds:
        raise SystemExit(1)


if __name__ == "__main__":
    main()
