"""Kernel time of the carrier survey's spectrum pass beside the envelope survey and the rx front end on one capture.

    python tools/spectrum_rate.py [--log2-samples 32] [--steps 10] [--warmup 2] [--out profiles/spectrum_rate.json]

One seeded capture made like bench.py's north_star capture (synthetic p3l-nexa2012 traffic) and the same capture cut to
8 bits (CS8, and CU8 of the same values).  Per format a Spectrum, a Survey through fs32_fs4 and a Receiver through
fs32_fs4 with quiet_skip=False (every tile filtered: a pass that reads and works on the whole capture, like the other
two) take turns on it, one run in flight at a time.  Written: the HIP-event kernel times (median, min, max) and the
share of the 8 TB/s HBM peak that reading the capture once in the median time means.  A record, not a gate: nothing
here asserts a rate.
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
    ap.add_argument("--out", default=os.path.join(HERE, "..", "profiles", "spectrum_rate.json"))
    args = ap.parse_args()
    n = 1 << args.log2_samples

    sys.path.insert(0, os.path.abspath(os.path.join(HERE, "..")))
    import torch
    import ookiedokie_amd as ok
    golden = os.path.join(HERE, "..", "tests", "golden")

    dev = ok.Device.load(os.path.join(golden, "devices", "p3l-nexa2012.json"), RATE)
    flt = ok.Filter.load(os.path.join(golden, "filters", "fs32_fs4.json"))
    syn = ok.Synth(dev, n, seed=SEED, sample_rate=RATE)
    c16 = torch.empty(2 * n + 64, dtype=torch.int16, device="cuda")
    syn.fill_device(c16.data_ptr())
    torch.cuda.synchronize()

    def share(nbytes, ms):
        return round(nbytes * n / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)

    out = {"samples": n, "steps": args.steps, "warmup": args.warmup, "hbm_peak_gbs": HBM_PEAK_GBS, "filter": "fs32_fs4",
           "spectrum_kernel_ms": "HIP-event time of the spectrum and reduce kernels (ookd_spectrum_kernel_ms)",
           "survey_kernel_ms": "HIP-event time of the envelope survey's kernel through fs32_fs4 on the same capture",
           "front_kernel_ms": "fir_kernel_ms of a Receiver through fs32_fs4 with quiet_skip=False on the same capture "
                              "(an 8-bit context's fused front end reads the 2-byte samples in place)",
           "hbm_peak_share": "capture bytes read once / median kernel time / HBM peak",
           "formats": {}}
    for fmt, nbytes in (("sc16q11", 4), ("cs8", 2), ("cu8", 2)):
        if fmt == "sc16q11":
            buf = c16
        else:
            buf = torch.empty(2 * n + 64, dtype=torch.int8 if fmt == "cs8" else torch.uint8, device="cuda")
            step = 1 << 28
            for lo in range(0, 2 * n, step):
                hi = min(lo + step, 2 * n)
                v = c16[lo:hi] >> 4
                buf[lo:hi] = v.to(torch.int8) if fmt == "cs8" else (v + 128).to(torch.uint8)
            torch.cuda.synchronize()
        sp = ok.Spectrum(sample_format=fmt)
        sv = ok.Survey(flt, sample_format=fmt)
        rx = ok.Receiver(flt, dev, max_samples=n, threshold=THRESHOLD, samples_per_buffer=SPB, quiet_skip=False,
                         sample_format=fmt)
        t_sp, t_sv, t_fir = [], [], []
        for k in range(args.warmup + args.steps):
            sp.spectrum_device(buf.data_ptr(), n)
            sv.survey_device(buf.data_ptr(), n)
            rx.process_device(buf.data_ptr(), n)
            st = rx.raw_stats()
            if k >= args.warmup:
                t_sp.append(sp.kernel_ms)
                t_sv.append(sv.kernel_ms)
                t_fir.append(float(st.fir_kernel_ms))
        frames, power = sp.result()
        carriers, floor = ok.suggest_carriers((frames, power))
        k_sp, k_sv, k_fir = summary(t_sp), summary(t_sv), summary(t_fir)
        out["formats"][fmt] = {
            "spectrum_kernel_ms": k_sp, "spectrum_hbm_peak_share": share(nbytes, k_sp["median"]),
            "spectrum_gsamples_per_s": round(n / (k_sp["median"] * 1e-3) / 1e9, 1),
            "survey_kernel_ms": k_sv, "survey_hbm_peak_share": share(nbytes, k_sv["median"]),
            "front_kernel_ms": k_fir, "front_hbm_peak_share": share(nbytes, k_fir["median"]),
            "front_form": int(st.front_form),
            "spectrum_over_survey": round(k_sp["median"] / k_sv["median"], 3),
            "spectrum_over_front": round(k_sp["median"] / k_fir["median"], 3),
            "frames": frames,
            "carriers": [{"bin": c.bin, "at_dc": c.at_dc, "ratio": round(c.ratio, 1)} for c in carriers]}
        sp.close()
        sv.close()
        rx.close()
        del buf

    path = os.path.abspath(args.out)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
