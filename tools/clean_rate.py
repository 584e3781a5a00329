"""Time of the edge cleaning pass (ookd_rx_clean_edges) beside the run whose edge list it reads.

    python tools/clean_rate.py [--log2-samples 32] [--log2-dense 28] [--steps 12] [--warmup 2]
                               [--out profiles/clean_rate.json]

(a) judged.  One seeded capture made like bench.py's north_star capture (synthetic p3l-nexa2012 traffic, 2^32
    samples) through fs32_fs4 and the p3l-nexa2012 decoder at threshold 0.1, cleaned with min_on = 250 us of decimated
    samples.  Every step is a fresh run followed by the first clean_edges call after it -- the one that launches; the
    cache is never what gets timed.  Recorded: the pass's HIP-event time (zeroing the counts + the three kernels)
    beside the same run's fir_kernel_ms and total_device_ms.
    Condition: median pass <= 3/16 of the median fir_kernel_ms.  A full default edge list is 1/16 of the capture's
    bytes, and the pass reads it twice and writes it at most once.  The tool exits with status 1 when the condition
    fails.
    Also recorded: what suggest_device answers on this capture without and with the cleaning.
(b) recorded, not judged.  2^28 samples without a filter, every sample an edge with probability 1/32 (runs of 32
    samples on average, geometric), so that the list nearly fills its default capacity; min_on = min_off = 8.  The
    pass beside a device-to-device hipMemcpyAsync of the same list bytes, timed the same way, and beside the pulse
    and the symbol pass over the same list.
"""
import argparse
import ctypes as C
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
RATE, SPB, THRESHOLD, SEED = 3000000, 8192, 0.1, 0x00C0FFEE + 15
MIN_ON_US = 250.0


def summary(v):
    v = sorted(v)
    m = len(v) // 2
    med = v[m] if len(v) % 2 else 0.5 * (v[m - 1] + v[m])
    return {"median": round(med, 5), "min": round(v[0], 5), "max": round(v[-1], 5)}


def answer(s, ok):
    keys = ("found", "num_bits", "frames_seen", "frames_counted", "frames_clean", "num_syncs", "sync_on_us", "sync_off_us",
            "bit_on_us", "zero_off_us", "one_off_us")
    out = {k: int(s[k]) for k in keys}
    out["reason"] = ok.CODING_REASONS[s["reason"]]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2-samples", type=int, default=32)
    ap.add_argument("--log2-dense", type=int, default=28)
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(HERE, "..", "profiles", "clean_rate.json"))
    args = ap.parse_args()
    if args.steps < 12:
        raise SystemExit("--steps: the median is taken over at least 12 calls")

    sys.path.insert(0, os.path.abspath(os.path.join(HERE, "..")))
    import torch
    import ookiedokie_amd as ok
    golden = os.path.join(HERE, "..", "tests", "golden")
    out = {"steps": args.steps, "warmup": args.warmup,
           "command": "python tools/clean_rate.py --log2-samples %d --log2-dense %d --steps %d --warmup %d"
                      % (args.log2_samples, args.log2_dense, args.steps, args.warmup),
           "clean_ms": "HIP-event time of the pass behind the first ookd_rx_clean_edges after a run: hipMemsetAsync of "
                       "the counts + clean_agg_kernel, clean_scan_kernel, clean_compact_kernel (ookd_rx_clean_kernel_ms)"}

    # ---- (a) the bench recipe's capture ------------------------------------------------------------------
    n = 1 << args.log2_samples
    flt = ok.Filter.load(os.path.join(golden, "filters", "fs32_fs4.json"))
    out_rate = RATE / flt.total_decimation
    min_on = int(MIN_ON_US * 1e-6 * out_rate)
    dev = ok.Device.load(os.path.join(golden, "devices", "p3l-nexa2012.json"), RATE // flt.total_decimation)
    syn = ok.Synth(dev, n, seed=SEED, sample_rate=RATE)
    cap = torch.empty(2 * n + 64, dtype=torch.int16, device="cuda")
    syn.fill_device(cap.data_ptr())
    torch.cuda.synchronize()
    rx = ok.Receiver(flt, dev, max_samples=n, threshold=THRESHOLD, samples_per_buffer=SPB)
    t_clean, t_fir, t_run = [], [], []
    for k in range(args.warmup + args.steps):
        rx.process_device(cap.data_ptr(), n)
        st = rx.raw_stats()
        info = rx.clean_edges(min_on, 0)[0]
        if k >= args.warmup:
            t_clean.append(rx.clean_kernel_ms)
            t_fir.append(float(st.fir_kernel_ms))
            t_run.append(float(st.total_device_ms))
    clean, fir = summary(t_clean), summary(t_fir)
    holds = clean["median"] <= 3.0 * fir["median"] / 16.0
    out["bench_capture"] = {
        "samples": n, "filter": "fs32_fs4", "device": "p3l-nexa2012", "threshold": THRESHOLD, "min_on": min_on, "min_off": 0,
        "edges": info["edges_in"], "edges_cleaned": info["edges_out"], "deleted_off_on": info["deleted"],
        "messages": int(st.num_messages), "front_form": int(st.front_form),
        "clean_ms": clean, "fir_kernel_ms": fir, "total_device_ms": summary(t_run),
        "clean_over_fir": round(clean["median"] / fir["median"], 6),
        "condition": "clean_ms.median <= 3 * fir_kernel_ms.median / 16", "condition_holds": bool(holds),
        "suggest_device": answer(rx.suggest_device(out_rate), ok),
        "suggest_device_cleaned": answer(rx.suggest_device(out_rate, min_on=min_on), ok),
    }
    rx.close()
    del cap
    torch.cuda.empty_cache()

    # ---- (b) an edge list near its default capacity ------------------------------------------------------
    n = 1 << args.log2_dense
    gen = torch.Generator(device="cuda")
    gen.manual_seed(SEED)
    cap = torch.zeros(2 * n + 64, dtype=torch.int16, device="cuda")
    step = 1 << 26
    level = 0
    for lo in range(0, n, step):                    # the level is the parity of the edges so far
        hi = min(lo + step, n)
        flips = (torch.rand(hi - lo, device="cuda", generator=gen) < 1.0 / 32.0).to(torch.int32)
        lv = (torch.cumsum(flips, 0) + level) & 1
        level = int(lv[-1])
        cap[2 * lo:2 * hi:2] = (lv * 2047).to(torch.int16)
    torch.cuda.synchronize()
    rx = ok.Receiver(None, None, max_samples=n, threshold=THRESHOLD, samples_per_buffer=SPB)
    rx.process_device(cap.data_ptr(), n)
    edges = int(rx.raw_stats().num_edges)
    nbytes = 8 * edges
    src = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    dst = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    hip.hipMemcpyAsync.restype = C.c_int
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    null = torch.cuda.default_stream()
    table = dict(lower=[[1, 16, 64], [1, 16, 64]], upper=[[15, 63, 1 << 20], [15, 63, 1 << 20]])
    t_clean, t_copy, t_pulse, t_symbol = [], [], [], []
    for k in range(args.warmup + args.steps):
        rx.process_device(cap.data_ptr(), n)
        info = rx.clean_edges(8, 8)[0]
        rx.pulse_hist(0)
        t_p = rx.pulse_kernel_ms
        rx.symbol_survey(table, None, 0)
        t_s = rx.symbol_kernel_ms
        e0.record(null)
        if hip.hipMemcpyAsync(dst.data_ptr(), src.data_ptr(), nbytes, 3, None) != 0:      # hipMemcpyDeviceToDevice
            raise SystemExit("hipMemcpyAsync failed")
        e1.record(null)
        e1.synchronize()
        if k >= args.warmup:
            t_clean.append(rx.clean_kernel_ms)
            t_copy.append(e0.elapsed_time(e1))
            t_pulse.append(t_p)
            t_symbol.append(t_s)
    clean, copy = summary(t_clean), summary(t_copy)
    out["dense_capture"] = {
        "samples": n, "filter": None, "mean_run": 32, "min_on": 8, "min_off": 8, "edges": info["edges_in"],
        "edges_cleaned": info["edges_out"], "deleted_off_on": info["deleted"], "edge_list_bytes": nbytes,
        "default_edge_capacity": n // 32 + (1 << 20),
        "clean_ms": clean, "d2d_copy_ms": copy, "pulse_ms": summary(t_pulse), "symbol_kinds_ms": summary(t_symbol),
        "clean_over_copy": round(clean["median"] / copy["median"], 3),
        "list_gbs": round(nbytes / (clean["median"] * 1e-3) / 1e9, 1),
    }
    rx.close()

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
