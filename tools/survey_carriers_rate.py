"""Kernel time of the carriers survey (several carriers in one pass, every S-th output counted) beside the single
tuned surveys it replaces, on the same capture.

    python tools/survey_carriers_rate.py [--log2-samples 32] [--steps 8] [--warmup 2]
                                         [--sweep] [--out profiles/survey_carriers_rate.json]

One process, one seeded capture made like bench.py's north_star capture (synthetic p3l-nexa2012 traffic) and the same
capture cut to 8 bits (CS8), filter fs32_fs4.  The legs take turns on it, one run in flight at a time:
  K4_S<S>       Survey(carriers=4 nus, stride=S), S = 1, 2, 4, 8, 16, 32, 64       form 4, survey_tuned_multi_kernel
  K<K>_S8       the same for K = 1, 2, 8, 16 carriers at stride 8
  single_<k>    Survey(tune=nu_k) of each of the 4 nus                          form 3, survey_tuned_fir1_kernel
Written: ookd_survey_kernel_ms of each leg as median with min and max, the GB/s of capture read per leg, the sum of
the four single passes, the ratios (K4_S8 / sum, K4_S1 / sum) and the two conditions on them (<= 0.5, <= 1.05), and
whether K4_S1 gave the singles' histograms bin for bin.  --sweep also times the K = 4 pass at every stride with 8, 16
and (where the stride allows) 32 and 64 output positions per lane (the OOKD_SURVEY_MULTI_R experiment hook) -- what survey_multi_R was chosen from.
"""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
RATE, SEED = 3000000, 0x00C0FFEE + 8
NUS = [0.2, -0.3, 0.11, -0.07, 0.33, -0.41, 0.25, -0.125, 0.05, -0.02, 0.45, -0.48, 0.15, -0.22, 0.38, -0.35]
STRIDES = (1, 2, 4, 8, 16, 32, 64)
KS = (1, 2, 8, 16)


def summary(v):
    v = sorted(v)
    m = len(v) // 2
    med = v[m] if len(v) % 2 else 0.5 * (v[m - 1] + v[m])
    return {"median": round(med, 4), "min": round(v[0], 4), "max": round(v[-1], 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2-samples", type=int, default=32)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--out", default=os.path.join(HERE, "..", "profiles", "survey_carriers_rate.json"))
    args = ap.parse_args()
    n = 1 << args.log2_samples
    if args.sweep:
        os.environ["OOKD_DEVELOPER"] = "1"

    sys.path.insert(0, os.path.abspath(os.path.join(HERE, "..")))
    import torch
    import ookiedokie_amd as ok
    golden = os.path.join(HERE, "..", "tests", "golden")

    dev = ok.Device.load(os.path.join(golden, "devices", "p3l-nexa2012.json"), RATE)
    syn = ok.Synth(dev, n, seed=SEED, sample_rate=RATE)
    c16 = torch.empty(2 * n + 64, dtype=torch.int16, device="cuda")
    syn.fill_device(c16.data_ptr())
    torch.cuda.synchronize()
    cs8 = torch.empty(2 * n + 64, dtype=torch.int8, device="cuda")
    step = 1 << 28
    for lo in range(0, 2 * n, step):
        hi = min(lo + step, 2 * n)
        cs8[lo:hi] = (c16[lo:hi] >> 4).to(torch.int8)
    torch.cuda.synchronize()
    flt = ok.Filter.load(os.path.join(golden, "filters", "fs32_fs4.json"))

    out = {"samples": n, "steps": args.steps, "warmup": args.warmup, "filter": "fs32_fs4", "nus": NUS,
           "kernel_ms": "ookd_survey_kernel_ms: HIP-event time of the histogram kernel; median, min, max over the steps, "
                        "the legs alternating",
           "formats": {}}
    for fmt, buf, sample_bytes in (("sc16q11", c16, 4), ("cs8", cs8, 2)):
        os.environ.pop("OOKD_SURVEY_MULTI_R", None)
        legs = {}
        for S in STRIDES:
            legs["K4_S%d" % S] = ok.Survey(flt, sample_format=fmt, carriers=NUS[:4], stride=S)
        for K in KS:
            legs["K%d_S8" % K] = ok.Survey(flt, sample_format=fmt, carriers=NUS[:K], stride=8)
        for k in range(4):
            legs["single_%d" % k] = ok.Survey(flt, sample_format=fmt, tune=NUS[k])
        times = {k: [] for k in legs}
        for it in range(args.warmup + args.steps):
            for k, sv in legs.items():
                sv.survey_device(buf.data_ptr(), n)
                if it >= args.warmup:
                    times[k].append(sv.kernel_ms)
        per = {}
        for k, sv in legs.items():
            t = summary(times[k])
            per[k] = {"form": sv.form, "kernel_ms": t,
                      "capture_gb_per_s": round(n * sample_bytes / (t["median"] * 1e-3) / 1e9, 1)}
        singles = sum(per["single_%d" % k]["kernel_ms"]["median"] for k in range(4))
        per["sum_of_4_singles_ms"] = round(singles, 4)
        per["K4_S8_over_singles"] = round(per["K4_S8"]["kernel_ms"]["median"] / singles, 4)
        per["K4_S1_over_singles"] = round(per["K4_S1"]["kernel_ms"]["median"] / singles, 4)
        per["K4_S8_at_most_half"] = bool(per["K4_S8_over_singles"] <= 0.5)
        per["K4_S1_at_most_1_05"] = bool(per["K4_S1_over_singles"] <= 1.05)
        per["K4_S1_equals_singles"] = bool(all((legs["K4_S1"].hist(0, k) == legs["single_%d" % k].hist()).all()
                                               for k in range(4)))
        want = [legs["K4_S%d" % S].hist(0, 3) for S in STRIDES]
        for sv in legs.values():
            sv.close()
        if args.sweep:
            shaped = {}
            for R in (8, 16, 32, 64):
                os.environ["OOKD_SURVEY_MULTI_R"] = str(R)
                for S in STRIDES:
                    if R >= 32 and S < R:
                        continue                    # the large windows hold one counted output per lane
                    shaped["R%d_K4_S%d" % (R, S)] = ok.Survey(flt, sample_format=fmt, carriers=NUS[:4], stride=S)
            os.environ.pop("OOKD_SURVEY_MULTI_R", None)
            ts = {k: [] for k in shaped}
            for it in range(args.warmup + args.steps):
                for k, sv in shaped.items():
                    sv.survey_device(buf.data_ptr(), n)
                    if it >= args.warmup:
                        ts[k].append(sv.kernel_ms)
            sweep = {}
            for k, sv in shaped.items():
                S = int(k.rsplit("S", 1)[1])
                sweep[k] = {"kernel_ms": summary(ts[k]),
                            "equals_default": bool((sv.hist(0, 3) == want[STRIDES.index(S)]).all())}
                sv.close()
            per["positions_per_lane_R"] = sweep
        out["formats"][fmt] = per

    path = os.path.abspath(args.out)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
