"""Kernel time of the envelope survey beside an OOKD_RX_EXACT_FIR decode of the same capture.

    python tools/survey_rate.py [--log2-samples 32] [--steps 10] [--warmup 2] [--out profiles/survey_rate.json]

One seeded capture made like bench.py's north_star capture (synthetic p3l-nexa2012 traffic) and the same capture cut to
8 bits (CS8).  Per filter (fs32_fs4, fs128_fs16_dec4) and format a Survey and an exact-FIR Receiver -- the nearest
existing kernel: the same arithmetic, a slicer instead of a histogram behind it -- take turns on it, one run in flight
at a time.  Written: the survey's HIP-event kernel time (median, min, max), the share of the 8 TB/s HBM peak that
reading the capture once in that time means, and the decode's front-end kernel time and whole-run time.  A record, not
a gate: nothing here asserts a rate.
"""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
HBM_PEAK_GBS = 8000.0
RATE, SPB, THRESHOLD, SEED = 3000000, 8192, 0.1, 0x00C0FFEE + 8


def summary(v):
    v = sorted(v)
    m = len(v) // 2
    med = v[m] if len(v) % 2 else 0.5 * (v[m - 1] + v[m])
    return {"median": round(med, 4), "min": round(v[0], 4), "max": round(v[-1], 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2-samples", type=int, default=32)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(HERE, "..", "profiles", "survey_rate.json"))
    args = ap.parse_args()
    n = 1 << args.log2_samples

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
    captures = {"sc16q11": (c16, 4), "cs8": (cs8, 2)}

    out = {"samples": n, "steps": args.steps, "warmup": args.warmup, "hbm_peak_gbs": HBM_PEAK_GBS,
           "survey_kernel_ms": "HIP-event time of the histogram kernel (ookd_survey_kernel_ms)",
           "hbm_peak_share": "capture bytes read once / survey kernel time / HBM peak",
           "exact_fir_decode": "a Receiver with exact_fir=True on the same capture: fir_kernel_ms is its front end "
                               "(for cs8 the widening copy runs before it and is not in that figure), step_ms the whole run",
           "filters": {}}
    for name in ("fs32_fs4", "fs128_fs16_dec4"):
        flt = ok.Filter.load(os.path.join(golden, "filters", name + ".json"))
        d = ok.Device.load(os.path.join(golden, "devices", "p3l-nexa2012.json"), RATE // flt.total_decimation)
        per = {}
        for fmt, (buf, nbytes) in captures.items():
            sv = ok.Survey(flt, sample_format=fmt)
            rx = ok.Receiver(flt, d, max_samples=n, threshold=THRESHOLD, samples_per_buffer=SPB, exact_fir=True,
                             sample_format=fmt)
            t_sv, t_fir, t_run = [], [], []
            for k in range(args.warmup + args.steps):
                sv.survey_device(buf.data_ptr(), n)
                rx.process_device(buf.data_ptr(), n)
                st = rx.raw_stats()
                if k >= args.warmup:
                    t_sv.append(sv.kernel_ms)
                    t_fir.append(float(st.fir_kernel_ms))
                    t_run.append(float(st.total_device_ms))
            h = sv.hist()
            sug = ok.suggest_threshold(h)
            kern = summary(t_sv)
            per[fmt] = {"survey_kernel_ms": kern,
                        "hbm_peak_share": round(nbytes * n / (kern["median"] * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
                        "gsamples_per_s": round(n / (kern["median"] * 1e-3) / 1e9, 1),
                        "exact_fir_decode": {"fir_kernel_ms": summary(t_fir), "step_ms": summary(t_run),
                                             "front_form": int(st.front_form)},
                        "survey_over_exact_front": round(kern["median"] / summary(t_fir)["median"], 3),
                        "counted": int(h.sum(dtype="uint64")), "occupied_bins": int((h != 0).sum()),
                        "suggestion": {k2: (round(v, 6) if isinstance(v, float) else v) for k2, v in sug.items()}}
            sv.close()
            rx.close()
        out["filters"][name] = per

    path = os.path.abspath(args.out)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
