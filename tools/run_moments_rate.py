"""Time of the pulse moments' pass (ookd_rx_run_moments) beside the pulse levels' pass of the same run and the run's
front end.

    python tools/run_moments_rate.py [--log2-samples 32] [--steps 12] [--warmup 2] [--out profiles/run_moments_rate.json]

(a) judged.  The capture of tools/run_levels_rate.py: seeded synthetic p3l-nexa2012 traffic made like bench.py's
    north_star capture (2^32 samples) through fs32_fs4 and the p3l-nexa2012 decoder at threshold 0.1.  Every step is a
    fresh run, then the first run_moments call after it and the first run_levels call after it -- the ones that launch
    --, one at a time on the device.  Recorded: the two passes' HIP-event times (zeroing the result and the kernels)
    beside the run's fir_kernel_ms, the tiles each pass filtered, the runs.
(b) judged.  The same number of samples, on throughout: every tile is filtered and every tile's sums go to the one
    run -- the worst case of both passes.
Condition: median moments pass <= 2 x median levels pass, on both captures.  The tool exits with status 1 when it fails.

OOKD_DEVELOPER=1 OOKD_MOMENTS_TABLE=0 in the environment times the form without the LDS segment table (every wave adds
its segments to global memory); --out then names another file.
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


def measure(rx, ptr, n, steps, warmup):
    t_mo, t_lv, t_fir = [], [], []
    for k in range(warmup + steps):
        rx.process_device(ptr, n)
        st = rx.raw_stats()
        mo = rx.run_moments(0)
        lv = rx.run_levels(0)
        if k >= warmup:
            t_mo.append(rx.moments_kernel_ms)
            t_lv.append(rx.levels_kernel_ms)
            t_fir.append(float(st.fir_kernel_ms))
    a, b, c = summary(t_mo), summary(t_lv), summary(t_fir)
    ratio = a["median"] / b["median"]
    return {
        "samples": n, "edges": int(st.num_edges), "messages": int(st.num_messages), "front_form": int(st.front_form),
        "moments_ms": a, "levels_ms": b, "fir_kernel_ms": c,
        "moments_over_levels": round(ratio, 4), "moments_over_fir": round(a["median"] / c["median"], 4),
        "num_runs": mo["num_runs"], "tile_outputs": mo["tile_outputs"], "levels_tile_outputs": lv["tile_outputs"],
        "tiles_total": mo["tiles_total"], "tiles_filtered": mo["tiles_filtered"],
        "tiles_filtered_share": round(mo["tiles_filtered"] / max(mo["tiles_total"], 1), 5),
        "power_sum": int(mo["power"].astype(object).sum()) if mo["num_runs"] else 0,
        "condition": "moments_ms.median <= 2 * levels_ms.median", "condition_holds": bool(ratio <= 2.0),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2-samples", type=int, default=32)
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(HERE, "..", "profiles", "run_moments_rate.json"))
    args = ap.parse_args()
    if args.steps < 12:
        raise SystemExit("--steps: the median is taken over at least 12 calls")

    sys.path.insert(0, os.path.abspath(os.path.join(HERE, "..")))
    import torch
    import ookiedokie_amd as ok
    golden = os.path.join(HERE, "..", "tests", "golden")
    n = 1 << args.log2_samples
    table = os.environ.get("OOKD_MOMENTS_TABLE") if os.environ.get("OOKD_DEVELOPER", "0") not in ("", "0") else None
    out = {"steps": args.steps, "warmup": args.warmup,
           "command": "python tools/run_moments_rate.py --log2-samples %d --steps %d --warmup %d"
                      % (args.log2_samples, args.steps, args.warmup),
           "segment_table": "the library's" if table is None else "OOKD_MOMENTS_TABLE=%s" % table,
           "moments_ms": "HIP-event time of the pass behind the first ookd_rx_run_moments after a run: hipMemsetAsync of "
                         "the result + run_moments_kernel (ookd_rx_moments_kernel_ms)",
           "levels_ms": "the same of the first ookd_rx_run_levels after the same run (ookd_rx_levels_kernel_ms), in turns",
           "fir_kernel_ms": "the run's front end (ookd_rx_stats.fir_kernel_ms)"}

    flt = ok.Filter.load(os.path.join(golden, "filters", "fs32_fs4.json"))
    dev = ok.Device.load(os.path.join(golden, "devices", "p3l-nexa2012.json"), RATE // flt.total_decimation)
    syn = ok.Synth(dev, n, seed=SEED, sample_rate=RATE)
    cap = torch.empty(2 * n + 64, dtype=torch.int16, device="cuda")
    syn.fill_device(cap.data_ptr())
    torch.cuda.synchronize()
    rx = ok.Receiver(flt, dev, max_samples=n, threshold=THRESHOLD, samples_per_buffer=SPB)

    a = measure(rx, cap.data_ptr(), n, args.steps, args.warmup)
    a.update(filter="fs32_fs4", device="p3l-nexa2012", threshold=THRESHOLD)
    out["bench_capture"] = a

    step = 1 << 28
    for lo in range(0, 2 * n, step):
        hi = min(lo + step, 2 * n)
        cap[lo:hi:2] = 1945
        cap[lo + 1:hi:2] = 0
    torch.cuda.synchronize()
    b = measure(rx, cap.data_ptr(), n, args.steps, args.warmup)
    b.update(filter="fs32_fs4", note="on throughout")
    out["on_throughout"] = b
    rx.close()

    path = os.path.abspath(args.out)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(out))
    if not (a["condition_holds"] and b["condition_holds"]):
        raise SystemExit(1)


if __name__ == "__main__":
    main()
