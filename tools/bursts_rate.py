"""Time of burst extraction (ookd_rx_bursts, ookd_rx_copy_bursts_device) beside its neighbours on the same run.

    python tools/bursts_rate.py [--log2-samples 32] [--steps 12] [--warmup 2] [--out profiles/bursts_rate.json]

One seeded capture made like bench.py's north_star capture (synthetic p3l-nexa2012 traffic, 2^32 samples) through
fs32_fs4 and the p3l-nexa2012 decoder at threshold 0.1; pre / post / max_gap from the device: 200 us in front, its
longest timeout and 600 us behind, max_gap = pre + post.  Every step is a fresh run and then, one at a time on the
device in one process: the stand-alone clean pass (ookd_rx_clean_edges 2 / 2), the pulse pass, the table pass -- the
first ookd_rx_bursts after the run, the one that launches --, the copy into device memory, and a hipMemcpyAsync
device-to-device of the same number of bytes between the same two allocations, timed with HIP events like the rest.

Recorded: the bursts, the cut's share of the capture, the medians of the five times and the run's front end.
The same again, recorded and not judged, with tight margins -- 200 us in front and behind, max_gap = 400 us -- which
split the capture's traffic into its single messages and pulses: many short bursts, the copy's search and walk at work.
Two conditions, on the device's margins, each against a neighbour and never against this code itself; the tool exits
with status 1 when one fails:
    table pass   bursts_ms.median <= 2 clean_ms.median: the same three launches and one read of the list, less written;
                 the factor two covers the wider aggregate.
    copy         copy_ms.median <= 2 memcpy_ms.median: one search per workgroup and sample-aligned sources may cost
                 something; a pass that moved a sample per lane would miss this by more.
"""
import argparse
import ctypes as C
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
    ap.add_argument("--out", default=os.path.join(HERE, "..", "profiles", "bursts_rate.json"))
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

    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpyAsync.restype = C.c_int
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def measure(pre, post, max_gap):
        # one run ahead of the timed ones sizes the cut's buffer
        rx.process_device(cap.data_ptr(), n)
        info = rx.bursts(pre, post, max_gap)[0]
        total = info["total_samples"]
        cut = torch.empty(2 * max(total, 1) + 64, dtype=torch.int16, device="cuda")
        t = {k: [] for k in ("clean_ms", "pulse_ms", "bursts_ms", "copy_ms", "memcpy_ms", "fir_kernel_ms")}
        for k in range(args.warmup + args.steps):
            rx.process_device(cap.data_ptr(), n)
            st = rx.raw_stats()
            rx.clean_edges(2, 2)
            rx.pulse_hist(0)
            info = rx.bursts(pre, post, max_gap)[0]
            assert info["total_samples"] == total
            rx.burst_samples_device(0, cut.data_ptr(), total)
            torch.cuda.synchronize()
            e0.record()
            if hip.hipMemcpyAsync(cut.data_ptr(), cap.data_ptr(), total * 4, 3, None) != 0:      # hipMemcpyDeviceToDevice
                raise SystemExit("hipMemcpyAsync failed")
            e1.record()
            torch.cuda.synchronize()
            if k >= args.warmup:
                t["clean_ms"].append(rx.clean_kernel_ms)
                t["pulse_ms"].append(rx.pulse_kernel_ms)
                t["bursts_ms"].append(rx.bursts_kernel_ms)
                t["copy_ms"].append(rx.burst_copy_kernel_ms)
                t["memcpy_ms"].append(e0.elapsed_time(e1))
                t["fir_kernel_ms"].append(float(st.fir_kernel_ms))
        del cut
        s = {k: summary(v) for k, v in t.items()}
        gb = total * 4 / 1e9
        return {
            "samples": n, "edges": int(st.num_edges), "messages": int(st.num_messages), "front_form": int(st.front_form),
            "pre": pre, "post": post, "max_gap": max_gap,
            "num_bursts": info["num_bursts"], "num_runs": info["num_runs"], "total_samples": total,
            "cut_share": round(total / n, 5), "cut_bytes": total * 4,
            "times": s,
            "bursts_over_clean": round(s["bursts_ms"]["median"] / s["clean_ms"]["median"], 4),
            "bursts_over_pulse": round(s["bursts_ms"]["median"] / s["pulse_ms"]["median"], 4),
            "copy_over_memcpy": round(s["copy_ms"]["median"] / s["memcpy_ms"]["median"], 4),
            "copy_gb_per_s_read_plus_write": round(2.0 * gb / (s["copy_ms"]["median"] * 1e-3), 1),
            "memcpy_gb_per_s_read_plus_write": round(2.0 * gb / (s["memcpy_ms"]["median"] * 1e-3), 1),
        }

    a = measure(pre, post, max_gap)
    table_holds = a["times"]["bursts_ms"]["median"] <= 2.0 * a["times"]["clean_ms"]["median"]
    copy_holds = a["times"]["copy_ms"]["median"] <= 2.0 * a["times"]["memcpy_ms"]["median"]
    a.update(table_condition="bursts_ms.median <= 2 clean_ms.median", table_condition_holds=bool(table_holds),
             copy_condition="copy_ms.median <= 2 memcpy_ms.median", copy_condition_holds=bool(copy_holds))
    tight = TIGHT_US * out_rate // 1000000
    b = measure(tight, tight, 2 * tight)
    b.update(note="tight margins: recorded, not judged")
    rx.close()

    out = {
        "steps": args.steps, "warmup": args.warmup,
        "command": "python tools/bursts_rate.py --log2-samples %d --steps %d --warmup %d" % (args.log2_samples, args.steps, args.warmup),
        "filter": "fs32_fs4", "device": "p3l-nexa2012", "threshold": THRESHOLD,
        "clean_ms": "ookd_rx_clean_kernel_ms of ookd_rx_clean_edges(2, 2) on the same run", "pulse_ms": "ookd_rx_pulse_kernel_ms",
        "bursts_ms": "ookd_rx_bursts_kernel_ms: hipMemsetAsync of the counts + the three kernels of the table pass",
        "copy_ms": "ookd_rx_burst_copy_kernel_ms: the copy kernel into device memory",
        "memcpy_ms": "hipMemcpyAsync device-to-device of cut_bytes from the capture into the same buffer, HIP events",
        "fir_kernel_ms": "the run's front end (ookd_rx_stats.fir_kernel_ms)",
        "device_margins": a, "tight_margins": b,
    }
    path = os.path.abspath(args.out)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(out))
    if not (table_holds and copy_holds):
        raise SystemExit(1)


if __name__ == "__main__":
    main()
