"""Kernel time of the carriers survey's fused two-stage form (OOKD_SURVEY_TUNED_MULTI_FIR2: several carriers in one
pass through the backend default fs128_fs16_dec4, every S-th output counted) beside the generic single tuned surveys
that serve this filter without it, on the same capture.

    python tools/survey_carriers_fir2_rate.py [--log2-samples 32] [--steps 8] [--warmup 2]
                                              [--out profiles/survey_carriers_fir2_rate.json]

One process, one seeded capture made like bench.py's north_star capture (synthetic p3l-nexa2012 traffic) and the same
capture cut to 8 bits (CS8), filter fs128_fs16_dec4.  The legs take turns on it, one run in flight at a time:
  K<K>_S<S>     Survey(carriers=K nus, stride=S, tuned_fir2=True), K = 1, 4, S = 1, 8, 32, 64 form 5
  K<K>_S<S>_all the same at S = 32, 64 with every stage-0 output computed (the OOKD_SURVEY_FIR2_THIN=0 experiment
                hook) beside the default with stage 0 thinned -- what that choice was made from
  single_<k>    Survey(tune=nu_k) of each of the 4 nus                                       form 2, survey_kernel
Written: ookd_survey_kernel_ms of each leg as median with min and max, the GB/s of capture read per leg, the sum of
the four single passes, the ratio K4_S1 / sum and the one condition on it (<= 1), the ratios of the strided passes to
K<K>_S1 beside what the arithmetic alone would give ((8 min(1, 16 / S) + 8 / S) / 16 complex multiply-adds per input
sample and carrier), and whether K4_S1 gave the singles' histograms bin for bin and the two stage-0 shapes the same.
"""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
RATE, SEED = 3000000, 0x00C0FFEE + 8
NUS = [0.2, -0.3, 0.11, -0.07]
STRIDES = (1, 8, 32, 64)
THIN_STRIDES = (32, 64)
KS = (1, 4)


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
    ap.add_argument("--out", default=os.path.join(HERE, "..", "profiles", "survey_carriers_fir2_rate.json"))
    args = ap.parse_args()
    n = 1 << args.log2_samples
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
    flt = ok.Filter.load(os.path.join(golden, "filters", "fs128_fs16_dec4.json"))

    out = {"samples": n, "steps": args.steps, "warmup": args.warmup, "filter": "fs128_fs16_dec4", "nus": NUS,
           "kernel_ms": "ookd_survey_kernel_ms: HIP-event time of the histogram kernel; median, min, max over the steps, "
                        "the legs alternating",
           "arithmetic_expectation": {"S%d" % S: round((8.0 * min(1.0, 16.0 / S) + 8.0 / S) / 16.0, 4) for S in STRIDES},
           "formats": {}}
    for fmt, buf, sample_bytes in (("sc16q11", c16, 4), ("cs8", cs8, 2)):
        legs = {}
        for K in KS:
            for S in STRIDES:
                legs["K%d_S%d" % (K, S)] = ok.Survey(flt, sample_format=fmt, carriers=NUS[:K], stride=S, tuned_fir2=True)
        os.environ["OOKD_SURVEY_FIR2_THIN"] = "0"
        for K in KS:
            for S in THIN_STRIDES:
                legs["K%d_S%d_all" % (K, S)] = ok.Survey(flt, sample_format=fmt, carriers=NUS[:K], stride=S, tuned_fir2=True)
        os.environ.pop("OOKD_SURVEY_FIR2_THIN")
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
        per["K4_S1_over_singles"] = round(per["K4_S1"]["kernel_ms"]["median"] / singles, 4)
        per["K4_S1_at_most_the_singles"] = bool(per["K4_S1_over_singles"] <= 1.0)
        for K in KS:
            for S in STRIDES[1:]:
                per["K%d_S%d_over_S1" % (K, S)] = round(per["K%d_S%d" % (K, S)]["kernel_ms"]["median"] /
                                                        per["K%d_S1" % K]["kernel_ms"]["median"], 4)
        per["K4_S1_equals_singles"] = bool(all((legs["K4_S1"].hist(0, k) == legs["single_%d" % k].hist()).all()
                                               for k in range(4)))
        per["stage_0_shapes_equal"] = bool(all((legs["K%d_S%d" % (K, S)].hist(0, K - 1) ==
                                                legs["K%d_S%d_all" % (K, S)].hist(0, K - 1)).all()
                                               for K in KS for S in THIN_STRIDES))
        for K in KS:
            for S in THIN_STRIDES:
                per["K%d_S%d_thin_over_all" % (K, S)] = round(per["K%d_S%d" % (K, S)]["kernel_ms"]["median"] /
                                                              per["K%d_S%d_all" % (K, S)]["kernel_ms"]["median"], 4)
        for sv in legs.values():
            sv.close()
        out["formats"][fmt] = per

    path = os.path.abspath(args.out)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
