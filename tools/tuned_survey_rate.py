"""Kernel time of the tuned envelope survey beside the untuned one on the same capture.

    python tools/tuned_survey_rate.py [--log2-samples 32] [--steps 8] [--warmup 2] [--sweep]
                                      [--out profiles/tuned_survey_rate.json]

One process, one seeded capture made like bench.py's north_star capture (synthetic p3l-nexa2012 traffic) and the same
capture cut to 8 bits (CS8), filter fs32_fs4.  Three surveys take turns on it, one run in flight at a time:
  (a) the untuned Survey                                  form 1, survey_kernel
  (b) the tuned Survey, nu = 0.2                          form 3, survey_tuned_fir1_kernel
  (c) the same with exact=True                            form 2, survey_kernel<FMT, true>
Written: ookd_survey_kernel_ms of each as median with min and max, (b) / (a), (b) / (c), and whether (b) and (c) gave
the same histogram.  --sweep also times form 3 in every shape the kernel is instantiated for (outputs per lane x waves
per workgroup, through the OOKD_SURVEY_TUNED_SHAPE experiment hook) -- what kSurveyFir1R / kSurveyFir1Waves were
chosen from.  A record, not a gate: nothing here asserts a rate.
"""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
RATE, SEED, NU = 3000000, 0x00C0FFEE + 8, 0.2
SHAPES = ("8x1", "8x2", "8x4", "16x1", "16x2", "16x4")


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
    ap.add_argument("--out", default=os.path.join(HERE, "..", "profiles", "tuned_survey_rate.json"))
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

    out = {"samples": n, "steps": args.steps, "warmup": args.warmup, "filter": "fs32_fs4", "nu": NU,
           "kernel_ms": "ookd_survey_kernel_ms: HIP-event time of the histogram kernel; median, min, max over the steps, "
                        "the three surveys alternating",
           "formats": {}}
    for fmt, buf in (("sc16q11", c16), ("cs8", cs8)):
        os.environ.pop("OOKD_SURVEY_TUNED_SHAPE", None)
        svs = {"a_untuned": ok.Survey(flt, sample_format=fmt),
               "b_tuned_fir1": ok.Survey(flt, sample_format=fmt, tune=NU),
               "c_tuned_generic": ok.Survey(flt, sample_format=fmt, tune=NU, exact=True)}
        times = {k: [] for k in svs}
        for it in range(args.warmup + args.steps):
            for k, sv in svs.items():
                sv.survey_device(buf.data_ptr(), n)
                if it >= args.warmup:
                    times[k].append(sv.kernel_ms)
        per = {k: {"form": svs[k].form, "kernel_ms": summary(times[k])} for k in svs}
        a, b, c = (per[k]["kernel_ms"]["median"] for k in ("a_untuned", "b_tuned_fir1", "c_tuned_generic"))
        per["b_over_a"] = round(b / a, 4)
        per["b_over_c"] = round(b / c, 4)
        per["b_not_above_a"] = bool(b <= a)
        hb, hc = svs["b_tuned_fir1"].hist(), svs["c_tuned_generic"].hist()
        per["b_equals_c"] = bool((hb == hc).all())
        per["gsamples_per_s_b"] = round(n / (b * 1e-3) / 1e9, 1)
        per["suggestion_b"] = {k2: (round(v, 6) if isinstance(v, float) else v)
                               for k2, v in ok.suggest_threshold(hb).items()}
        for sv in svs.values():
            sv.close()
        if args.sweep:
            sweep = {}
            shaped = {}
            for shape in SHAPES:
                os.environ["OOKD_SURVEY_TUNED_SHAPE"] = shape
                shaped[shape] = ok.Survey(flt, sample_format=fmt, tune=NU)
            os.environ.pop("OOKD_SURVEY_TUNED_SHAPE", None)
            ts = {s: [] for s in SHAPES}
            for it in range(args.warmup + args.steps):
                for s, sv in shaped.items():
                    sv.survey_device(buf.data_ptr(), n)
                    if it >= args.warmup:
                        ts[s].append(sv.kernel_ms)
            for s, sv in shaped.items():
                sweep[s] = {"kernel_ms": summary(ts[s]), "equals_c": bool((sv.hist() == hc).all())}
                sv.close()
            per["fir1_shapes_R_x_waves"] = sweep
        out["formats"][fmt] = per

    path = os.path.abspath(args.out)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
