"""Time of the pulse levels' pass (ookd_rx_run_levels) beside the generic envelope survey of the same capture and the
run's front end.

    python tools/run_levels_rate.py [--log2-samples 32] [--steps 12] [--warmup 2] [--out profiles/run_levels_rate.json]

(a) judged.  One seeded capture made like bench.py's north_star capture (synthetic p3l-nexa2012 traffic, 2^32
    samples) through fs32_fs4 and the p3l-nexa2012 decoder at threshold 0.1.  Every step is a fresh run, the first
    run_levels call after it -- the one that launches -- and a Survey(fs32_fs4) of the same capture: the three take
    turns in one process, one at a time on the device.  Recorded: the pass's HIP-event time (zeroing the result, the
    sparse kernel, the histogram of the peaks) beside the survey's kernel time and the run's fir_kernel_ms; the share of
    tiles the pass filtered; the runs; the on bin of suggest_threshold(survey histogram) beside the occupied bins of the
    peaks' histogram.
    Condition: median pass < median survey.  The pass does a subset of the survey kernel's tile work -- the tiles with
    an on sample, well under half of them here -- plus a look at the edge list per tile and a short epilogue.  The
    ratio to the front end is recorded, not judged.  The tool exits with status 1 when the condition fails.
(b) recorded, not judged.  The same number of samples, on throughout: every tile is filtered and every tile's maximum
    goes to the one run -- the pass's worst case.
"""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
RATE, SPB, THRESHOLD, SEED = 3000000, 8192, 0.1, 0x00C0FFEE + 21


def summary(v):
    v = sorted(v)
    m = len(v) // 2
    med = v[m] if len(v) % 2 else 0.5 * (v[m - 1] + v[m])
    return {"median": round(med, 5), "min": round(v[0], 5), "max": round(v[-1], 5)}


def measure(ok, rx, sv, ptr, n, steps, warmup):
    t_lv, t_sv, t_fir = [], [], []
    for k in range(warmup + steps):
        rx.process_device(ptr, n)
        st = rx.raw_stats()
        lv = rx.run_levels(0)
        sv.survey_device(ptr, n)
        if k >= warmup:
            t_lv.append(rx.levels_kernel_ms)
            t_sv.append(sv.kernel_ms)
            t_fir.append(float(st.fir_kernel_ms))
    sug = ok.suggest_threshold(sv.hist())
    a, b, c = summary(t_lv), summary(t_sv), summary(t_fir)
    return {
        "samples": n, "edges": int(st.num_edges), "messages": int(st.num_messages), "front_form": int(st.front_form),
        "levels_ms": a, "survey_kernel_ms": b, "fir_kernel_ms": c,
        "levels_over_survey": round(a["median"] / b["median"], 4), "levels_over_fir": round(a["median"] / c["median"], 4),
        "num_runs": lv["num_runs"], "tile_outputs": lv["tile_outputs"], "tiles_total": lv["tiles_total"],
        "tiles_filtered": lv["tiles_filtered"], "tiles_filtered_share": round(lv["tiles_filtered"] / max(lv["tiles_total"], 1), 5),
        "survey_on_bin": int(sug["on_bin"]), "survey_found": int(sug["found"]),
        "peak_bins": [[int(b_), int(lv["hist"][b_])] for b_ in lv["hist"].nonzero()[0]],
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2-samples", type=int, default=32)
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(HERE, "..", "profiles", "run_levels_rate.json"))
    args = ap.parse_args()
    if args.steps < 12:
        raise SystemExit("--steps: the median is taken over at least 12 calls")

    sys.path.insert(0, os.path.abspath(os.path.join(HERE, "..")))
    import torch
    import ookiedokie_amd as ok
    golden = os.path.join(HERE, "..", "tests", "golden")
    n = 1 << args.log2_samples
    out = {"steps": args.steps, "warmup": args.warmup,
           "command": "python tools/run_levels_rate.py --log2-samples %d --steps %d --warmup %d"
                      % (args.log2_samples, args.steps, args.warmup),
           "levels_ms": "HIP-event time of the pass behind the first ookd_rx_run_levels after a run: hipMemsetAsync of "
                        "the result + run_levels_kernel + run_level_hist_kernel (ookd_rx_levels_kernel_ms)",
           "survey_kernel_ms": "ookd_survey_kernel_ms of Survey(fs32_fs4) on the same capture, in the same process, in turns",
           "fir_kernel_ms": "the run's front end (ookd_rx_stats.fir_kernel_ms)"}

    flt = ok.Filter.load(os.path.join(golden, "filters", "fs32_fs4.json"))
    dev = ok.Device.load(os.path.join(golden, "devices", "p3l-nexa2012.json"), RATE // flt.total_decimation)
    syn = ok.Synth(dev, n, seed=SEED, sample_rate=RATE)
    cap = torch.empty(2 * n + 64, dtype=torch.int16, device="cuda")
    syn.fill_device(cap.data_ptr())
    torch.cuda.synchronize()
    rx = ok.Receiver(flt, dev, max_samples=n, threshold=THRESHOLD, samples_per_buffer=SPB)
    sv = ok.Survey(flt)

    # ---- (a) the bench recipe's capture ------------------------------------------------------------------
    a = measure(ok, rx, sv, cap.data_ptr(), n, args.steps, args.warmup)
    holds = a["levels_ms"]["median"] < a["survey_kernel_ms"]["median"]
    a.update(filter="fs32_fs4", device="p3l-nexa2012", threshold=THRESHOLD,
             condition="levels_ms.median < survey_kernel_ms.median", condition_holds=bool(holds))
    out["bench_capture"] = a

    # ---- (b) on throughout: every tile filtered, one run ---------------------------------------------------
    step = 1 << 28
    for lo in range(0, 2 * n, step):
        hi = min(lo + step, 2 * n)
        cap[lo:hi:2] = 1945
        cap[lo + 1:hi:2] = 0
    torch.cuda.synchronize()
    b = measure(ok, rx, sv, cap.data_ptr(), n, args.steps, args.warmup)
    b.update(filter="fs32_fs4", note="on throughout: recorded, not judged")
    out["on_throughout"] = b
    rx.close()
    sv.close()

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
