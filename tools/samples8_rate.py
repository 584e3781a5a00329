"""One-context step times of 8-bit (CS8, CU8) runs against the 16-bit run on the widened capture.

    python tools/samples8_rate.py [--log2-samples 32] [--steps 20] [--warmup 3] [--out profiles/samples8_rate.json]
                                  [--baseline-tree DIR]

One seeded capture made like bench.py's north_star capture (synthetic p3l-nexa2012 traffic), cut to 8 bits
(iq >> 4) and widened back (16 v): the three captures hold the same values.  Per filter (fs32_fs4,
fs128_fs16_dec4) three contexts -- cs8, cu8, sc16q11 -- take turns, one run in flight at a time, `steps` timed steps
each after `warmup`.  A step's time is the library's own HIP-event span of the run (stats total_device_ms: first
kernel start to last kernel end) and the front-end kernel's (fir_kernel_ms); medians and min-max are written, with the
bytes each form reads per sample (from the window geometry) and the share of the 8 TB/s HBM peak the kernel time means.

--baseline-tree DIR: a built checkout of the commit to compare against (its 16-bit kernels).  Its 16-bit run on the
same widened capture is timed first, in a child process of its own, and reported as `baseline_sc16q11`.
--only16 is that child's mode: the 16-bit runs alone, of whatever tree is first on the path, result on stdout.
"""
import argparse
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
HBM_PEAK_GBS = 8000.0
RATE, SPB, THRESHOLD, SEED = 3000000, 8192, 0.1, 0x00C0FFEE + 8
# window samples read per 1024 input samples: 1024 + 32 of tap history (fs32_fs4), 1024 + 96 (the folded dec4 filter)
WINDOW = {"fs32_fs4": 1056.0 / 1024.0, "fs128_fs16_dec4": 1120.0 / 1024.0}


def summary(v):
    v = sorted(v)
    m = len(v) // 2
    med = v[m] if len(v) % 2 else 0.5 * (v[m - 1] + v[m])
    return {"median": round(med, 4), "min": round(v[0], 4), "max": round(v[-1], 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2-samples", type=int, default=32)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(HERE, "..", "profiles", "samples8_rate.json"))
    ap.add_argument("--baseline-tree", default=None)
    ap.add_argument("--only16", action="store_true")
    ap.add_argument("--tree", default=os.path.join(HERE, ".."))
    args = ap.parse_args()
    n = 1 << args.log2_samples

    baseline = None
    if args.baseline_tree:
        # before this process touches the GPU: the other build, alone on it
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--only16", "--tree", args.baseline_tree,
                            "--log2-samples", str(args.log2_samples), "--steps", str(args.steps), "--warmup",
                            str(args.warmup)], capture_output=True, text=True)
        if r.returncode != 0:
            raise SystemExit("baseline run failed:\n" + r.stdout[-2000:] + r.stderr[-2000:])
        baseline = json.loads(r.stdout.strip().splitlines()[-1])

    sys.path.insert(0, os.path.abspath(args.tree))
    import torch
    import ookiedokie_amd as ok
    golden = os.path.join(os.path.abspath(args.tree), "tests", "golden")

    dev = ok.Device.load(os.path.join(golden, "devices", "p3l-nexa2012.json"), RATE)
    syn = ok.Synth(dev, n, seed=SEED, sample_rate=RATE)
    w16 = torch.empty(2 * n + 64, dtype=torch.int16, device="cuda")
    syn.fill_device(w16.data_ptr())
    torch.cuda.synchronize()
    cs8 = cu8 = None
    if not args.only16:
        cs8 = torch.empty(2 * n + 64, dtype=torch.int8, device="cuda")
        cu8 = torch.empty(2 * n + 64, dtype=torch.uint8, device="cuda")
    step = 1 << 28
    for lo in range(0, 2 * n, step):            # cut to 8 bits; the 16-bit capture becomes the widened one, in place
        hi = min(lo + step, 2 * n)
        v = w16[lo:hi] >> 4
        if cs8 is not None:
            cs8[lo:hi] = v.to(torch.int8)
            cu8[lo:hi] = (v + 128).to(torch.uint8)
        w16[lo:hi] = v * 16
        del v
    torch.cuda.synchronize()
    captures = {"sc16q11": w16} if args.only16 else {"cs8": cs8, "cu8": cu8, "sc16q11": w16}

    out = {"samples": n, "steps": args.steps, "warmup": args.warmup, "hbm_peak_gbs": HBM_PEAK_GBS,
           "step_time": "one context, one run in flight: HIP-event span of the run's kernels (total_device_ms)",
           "filters": {}}
    for name in ("fs32_fs4", "fs128_fs16_dec4"):
        flt = ok.Filter.load(os.path.join(golden, "filters", name + ".json"))
        d = ok.Device.load(os.path.join(golden, "devices", "p3l-nexa2012.json"), RATE // flt.total_decimation)
        rxs = {}
        for fmt in captures:
            kw = {} if fmt == "sc16q11" else {"sample_format": fmt}
            rxs[fmt] = ok.Receiver(flt, d, max_samples=n, threshold=THRESHOLD, samples_per_buffer=SPB, **kw)
        times = {fmt: ([], []) for fmt in captures}
        results = {}
        for k in range(args.warmup + args.steps):
            for fmt, buf in captures.items():           # alternating
                rx = rxs[fmt]
                rx.process_device(buf.data_ptr(), n)
                st = rx.raw_stats()
                if k >= args.warmup:
                    times[fmt][0].append(float(st.total_device_ms))
                    times[fmt][1].append(float(st.fir_kernel_ms))
                results[fmt] = (int(st.num_messages), int(st.num_edges), int(st.guard_recomputes), int(st.front_form))
        per = {}
        for fmt in captures:
            bps = WINDOW[name] * (4.0 if fmt == "sc16q11" else 2.0)
            kern = summary(times[fmt][1])
            per[fmt] = {"step_ms": summary(times[fmt][0]), "fir_kernel_ms": kern, "bytes_read_per_sample": round(bps, 4),
                        "hbm_peak_share": round(bps * n / (kern["median"] * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
                        "gsamples_per_s": round(n / (summary(times[fmt][0])["median"] * 1e-3) / 1e9, 1),
                        "messages": results[fmt][0], "edges": results[fmt][1], "guard_recomputes": results[fmt][2],
                        "front_form": results[fmt][3]}
            rxs[fmt].close()
        assert len({results[f][:3] for f in captures}) == 1, "the formats disagree: %s" % (results,)
        out["filters"][name] = per

    if args.only16:
        print(json.dumps(out))
        return
    if baseline:
        for name in out["filters"]:
            b = baseline["filters"][name]["sc16q11"]
            per = out["filters"][name]
            per["baseline_sc16q11"] = b
            spread = b["step_ms"]["max"] - b["step_ms"]["min"]
            for fmt in ("cs8", "cu8"):
                per[fmt]["over_baseline_median_ms"] = round(per[fmt]["step_ms"]["median"] - b["step_ms"]["median"], 4)
                per[fmt]["not_slower_than_baseline"] = per[fmt]["step_ms"]["median"] <= b["step_ms"]["median"] + spread
            per["baseline_spread_ms"] = round(spread, 4)
    path = os.path.abspath(args.out)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
