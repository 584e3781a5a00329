"""Time of the burst basebands' pass (ookd_rx_burst_baseband_device) beside the run's front end, the raw burst copy and
the pulse moments' pass of the same run.

    python tools/burst_baseband_rate.py [--log2-samples 32] [--steps 12] [--warmup 2] [--out profiles/burst_baseband_rate.json]

The capture of tools/run_moments_rate.py: seeded synthetic p3l-nexa2012 traffic made like bench.py's north_star capture
(2^32 samples) at threshold 0.1.  Every step is a fresh run, then the table (ookd_rx_bursts) and the calls that launch,
one at a time on the device; the times are HIP-event times, medians of --steps steps.  Four sections, each in a child
process of its own under `timeout`, one after the other; the first that fails ends the tool:

margins      fs32_fs4, the round trip's margins (200 us in front, 18.4 ms behind, the gap their sum), CF32: the pass
             beside the run's fir_kernel_ms and beside the raw burst copy, tiles_filtered / tiles_total, bytes written.
tuned        fs128_fs16_dec4 (D = 4) in a context tuned 30 kHz beside the carrier, tuned_fir2 off and on, both formats:
             the pass, and the cut's bytes beside the raw cut's.
judged       fs32_fs4, CF32, pre = post = max_gap = 0 -- every on-run is its own burst, so this pass and the pulse
             moments' filter the same tiles with the same arithmetic -- in turns with ookd_rx_run_moments in one process.
             Condition: median baseband pass <= 1.1 x median moments pass.  The tool exits with status 1 when it fails.
on           the same comparison on a capture that is on throughout: recorded, not judged.
"""
import argparse
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
RATE, SPB, THRESHOLD, SEED = 3000000, 8192, 0.1, 0x00C0FFEE + 21
PRE_US, POST_US = 200, 18400
TUNE_HZ = 30e3
SECTIONS = ("margins", "tuned", "judged", "on")
SECTION_TIMEOUT = 420           # seconds: a section is a few dozen runs of 2^32 samples


def summary(v):
    v = sorted(v)
    m = len(v) // 2
    med = v[m] if len(v) % 2 else 0.5 * (v[m - 1] + v[m])
    return {"median": round(med, 5), "min": round(v[0], 5), "max": round(v[-1], 5)}


def margins(decimation):
    out_rate = RATE // decimation
    pre, post = PRE_US * out_rate // 1000000, POST_US * out_rate // 1000000
    return pre, post, pre + post


def measure(torch, rx, ptr, n, steps, warmup, m, fmt, raw_copy=False, moments=False):
    """steps fresh runs; per run the table, the baseband pass into device memory and, when asked, the raw copy and the
    moments' pass"""
    element = 8 if fmt == "cf32" else 4
    rx.process_device(ptr, n)
    table = rx.bursts(*m)[0]
    info = rx.baseband_info(0)
    out = torch.empty(max(info["total_outputs"], 1) * element, dtype=torch.uint8, device="cuda")
    raw = torch.empty(max(table["total_samples"], 1) * table["sample_bytes"], dtype=torch.uint8, device="cuda") if raw_copy else None
    t_bb, t_fir, t_table, t_copy, t_mo = [], [], [], [], []
    for k in range(warmup + steps):
        rx.process_device(ptr, n)
        st = rx.raw_stats()
        rx.bursts(*m)
        if moments and k % 2:                                   # in turns: who goes first alternates
            mo = rx.run_moments(0)
        rx.burst_baseband_device(0, out.data_ptr(), info["total_outputs"], fmt)
        if moments and not k % 2:
            mo = rx.run_moments(0)
        if raw_copy:
            rx.burst_samples_device(0, raw.data_ptr(), table["total_samples"])
        if k >= warmup:
            t_bb.append(rx.baseband_kernel_ms)
            t_fir.append(float(st.fir_kernel_ms))
            t_table.append(rx.bursts_kernel_ms)
            if raw_copy:
                t_copy.append(rx.burst_copy_kernel_ms)
            if moments:
                t_mo.append(rx.moments_kernel_ms)
    info = rx.baseband_info(0)
    bb, fir = summary(t_bb), summary(t_fir)
    r = {
        "samples": n, "edges": int(st.num_edges), "messages": int(st.num_messages), "front_form": int(st.front_form),
        "format": fmt, "pre": m[0], "post": m[1], "max_gap": m[2], "decimation": info["decimation"],
        "baseband_ms": bb, "fir_kernel_ms": fir, "table_ms": summary(t_table),
        "baseband_over_fir": round(bb["median"] / fir["median"], 4),
        "num_bursts": info["num_bursts"], "total_outputs": info["total_outputs"], "bytes_written": info["total_outputs"] * element,
        "raw_cut_bytes": int(table["total_samples"]) * int(table["sample_bytes"]),
        "cut_over_raw_cut_bytes": round(info["total_outputs"] * element / max(int(table["total_samples"]) * int(table["sample_bytes"]), 1), 5),
        "tile_outputs": info["tile_outputs"], "tiles_total": info["tiles_total"], "tiles_filtered": info["tiles_filtered"],
        "tiles_filtered_share": round(info["tiles_filtered"] / max(info["tiles_total"], 1), 5),
        "nu": info["nu"], "turn": info["turn"],
    }
    if raw_copy:
        c = summary(t_copy)
        r.update(raw_copy_ms=c, baseband_over_raw_copy=round(bb["median"] / c["median"], 4))
    if moments:
        a = summary(t_mo)
        ratio = bb["median"] / a["median"]
        r.update(moments_ms=a, baseband_over_moments=round(ratio, 4), moments_tiles_filtered=mo["tiles_filtered"],
                 moments_tile_outputs=mo["tile_outputs"], num_runs=mo["num_runs"])
    del out, raw
    return r


def section(name, args):
    sys.path.insert(0, os.path.abspath(os.path.join(HERE, "..")))
    import torch
    import ookiedokie_amd as ok
    golden = os.path.join(HERE, "..", "tests", "golden")
    n = 1 << args.log2_samples
    filt = "fs128_fs16_dec4" if name == "tuned" else "fs32_fs4"
    flt = ok.Filter.load(os.path.join(golden, "filters", filt + ".json"))
    D = flt.total_decimation
    dev = ok.Device.load(os.path.join(golden, "devices", "p3l-nexa2012.json"), RATE // D)
    cap = torch.empty(2 * n + 64, dtype=torch.int16, device="cuda")
    if name == "on":
        step = 1 << 28
        for lo in range(0, 2 * n, step):
            hi = min(lo + step, 2 * n)
            cap[lo:hi:2] = 1945
            cap[lo + 1:hi:2] = 0
    else:
        ok.Synth(dev if D == 1 else ok.Device.load(os.path.join(golden, "devices", "p3l-nexa2012.json"), RATE), n, seed=SEED,
                 sample_rate=RATE).fill_device(cap.data_ptr())
    torch.cuda.synchronize()
    out = {"filter": filt, "device": "p3l-nexa2012", "threshold": THRESHOLD}
    if name == "margins":
        rx = ok.Receiver(flt, dev, max_samples=n, threshold=THRESHOLD, samples_per_buffer=SPB)
        out.update(measure(torch, rx, cap.data_ptr(), n, args.steps, args.warmup, margins(D), "cf32", raw_copy=True))
        rx.close()
    elif name == "tuned":
        for fir2 in (False, True):
            rx = ok.Receiver(flt, dev, max_samples=n, threshold=THRESHOLD, samples_per_buffer=SPB, tune=TUNE_HZ / RATE, tuned_fir2=fir2)
            for fmt in ("cf32", "sc16q11"):
                out["%s_%s" % ("tuned_fir2" if fir2 else "generic", fmt)] = measure(torch, rx, cap.data_ptr(), n, args.steps,
                                                                                  args.warmup, margins(D), fmt)
            rx.close()
    else:
        rx = ok.Receiver(flt, dev, max_samples=n, threshold=THRESHOLD, samples_per_buffer=SPB)
        out.update(measure(torch, rx, cap.data_ptr(), n, args.steps, args.warmup, (0, 0, 0), "cf32", moments=True))
        rx.close()
        if name == "judged":
            out["condition"] = "baseband_ms.median <= 1.1 * moments_ms.median"
            out["condition_holds"] = bool(out["baseband_over_moments"] <= 1.1)
        else:
            out["note"] = "on throughout: recorded, not judged"
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2-samples", type=int, default=32)
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(HERE, "..", "profiles", "burst_baseband_rate.json"))
    ap.add_argument("--section", choices=SECTIONS, help="(internal) run one section in this process and print its result")
    args = ap.parse_args()
    if args.steps < 12:
        raise SystemExit("--steps: the median is taken over at least 12 calls")
    if args.section:
        return section(args.section, args)

    out = {"steps": args.steps, "warmup": args.warmup,
           "command": "python tools/burst_baseband_rate.py --log2-samples %d --steps %d --warmup %d"
                      % (args.log2_samples, args.steps, args.warmup),
           "baseband_ms": "HIP-event time of the pass behind ookd_rx_burst_baseband_device after a fresh run and its table: "
                          "hipMemsetAsync of the result word + burst_baseband_kernel (ookd_rx_baseband_kernel_ms)",
           "moments_ms": "the same of the first ookd_rx_run_moments after the same run (ookd_rx_moments_kernel_ms), in turns",
           "raw_copy_ms": "the raw burst copy of the same table (ookd_rx_burst_copy_kernel_ms)",
           "table_ms": "the burst table's pass (ookd_rx_bursts_kernel_ms)",
           "fir_kernel_ms": "the run's front end (ookd_rx_stats.fir_kernel_ms)"}
    path = os.path.abspath(args.out)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    status = 0
    for name in SECTIONS:
        cmd = ["timeout", "-k", "10", str(SECTION_TIMEOUT), sys.executable, os.path.abspath(__file__), "--section", name,
               "--log2-samples", str(args.log2_samples), "--steps", str(args.steps), "--warmup", str(args.warmup)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            sys.stderr.write(r.stdout + r.stderr)
            sys.stderr.write("section %s ended with status %d: nothing further is started\n" % (name, r.returncode))
            raise SystemExit(r.returncode if r.returncode > 1 else 2)
        out[name] = json.loads(r.stdout.strip().split("\n")[-1])
        sys.stderr.write("section %s: done\n" % name)
        sys.stderr.flush()
        with open(path, "w") as f:                              # (what is measured so far survives a later section)
            json.dump(out, f, indent=1, sort_keys=True)
            f.write("\n")
    print(json.dumps(out))
    if not out["judged"]["condition_holds"]:
        status = 1
    raise SystemExit(status)


if __name__ == "__main__":
    main()
