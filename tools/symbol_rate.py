"""Time of the symbol survey's pass (ookd_rx_symbol_survey) beside the run whose edge list it reads.

    python tools/symbol_rate.py [--log2-samples 32] [--log2-dense 28] [--steps 12] [--warmup 2]
                                [--out profiles/symbol_rate.json]

(a) judged.  One seeded capture made like bench.py's north_star capture and tools/pulse_rate.py's (synthetic p3l-nexa2012 traffic,
2^32 samples) through fs32_fs4 and the p3l-nexa2012 decoder at threshold 0.1.  Every step is a fresh run followed by
pulse_hist, a symbol survey without roles (one launch: the kind counts) and one with the roles ookd_suggest_coding
makes of those counts (three launches: aggregates, scan, frames).  Recorded: the HIP-event time of either survey
(zeroing the result + its kernels) beside the same run's fir_kernel_ms and ookd_rx_pulse_kernel_ms.

Condition: median pass with roles <= median fir_kernel_ms / 8.  A full default edge list is a sixteenth of the
capture's bytes and this pass reads the list twice.  The tool exits with status 1 when the condition fails.

Recorded, not judged: what Receiver.suggest_device answers on that capture (its default pauses of 4 .. 20 ms span the
sync gap of p3l-nexa2012).

(b) recorded, not judged.  tools/pulse_rate.py's dense capture: 2^28 samples without a filter, every sample an edge
with probability 1/32, so that the list nearly fills its default capacity.  Classes by length (1 .. 15, 16 .. 47, 48
and more on either level), roles ZERO for (0, 0), ONE for (1, 1), SYNC for (2, 2): about one symbol in twenty is a
sync and most frames hold an OTHER.  The survey with and without roles beside the same run's pulse pass.
"""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
RATE, SPB, THRESHOLD, SEED = 3000000, 8192, 0.1, 0x00C0FFEE + 15


def summary(v):
    v = sorted(v)
    m = len(v) // 2
    med = v[m] if len(v) % 2 else 0.5 * (v[m - 1] + v[m])
    return {"median": round(med, 5), "min": round(v[0], 5), "max": round(v[-1], 5)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2-samples", type=int, default=32)
    ap.add_argument("--log2-dense", type=int, default=28)
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(HERE, "..", "profiles", "symbol_rate.json"))
    args = ap.parse_args()
    if args.steps < 12:
        raise SystemExit("--steps: the median is taken over at least 12 calls")

    sys.path.insert(0, os.path.abspath(os.path.join(HERE, "..")))
    import numpy as np
    import torch
    import ookiedokie_amd as ok
    golden = os.path.join(HERE, "..", "tests", "golden")
    n = 1 << args.log2_samples
    flt = ok.Filter.load(os.path.join(golden, "filters", "fs32_fs4.json"))
    out_rate = RATE / flt.total_decimation
    dev = ok.Device.load(os.path.join(golden, "devices", "p3l-nexa2012.json"), RATE // flt.total_decimation)
    syn = ok.Synth(dev, n, seed=SEED, sample_rate=RATE)
    cap = torch.empty(2 * n + 64, dtype=torch.int16, device="cuda")
    syn.fill_device(cap.data_ptr())
    torch.cuda.synchronize()
    rx = ok.Receiver(flt, dev, max_samples=n, threshold=THRESHOLD, samples_per_buffer=SPB)
    t_kinds, t_roles, t_pulse, t_fir = [], [], [], []
    for k in range(args.warmup + args.steps):
        rx.process_device(cap.data_ptr(), n)
        st = rx.raw_stats()
        pulses = ok.suggest_pulses(rx.pulse_hist(0), out_rate)
        table = ok.symbol_table_from_pulses(pulses)
        kinds = rx.symbol_survey(table, None)
        ms_kinds = rx.symbol_kernel_ms
        coding = ok.suggest_coding(pulses, kinds)
        if not coding["found"]:
            raise SystemExit("no coding on the bench capture: %s" % ok.CODING_REASONS[coding["reason"]])
        survey = rx.symbol_survey(table, coding["roles"])
        if k >= args.warmup:
            t_kinds.append(ms_kinds)
            t_roles.append(rx.symbol_kernel_ms)
            t_pulse.append(rx.pulse_kernel_ms)
            t_fir.append(float(st.fir_kernel_ms))
    suggestion = rx.suggest_device(out_rate)
    roles, fir = summary(t_roles), summary(t_fir)
    holds = roles["median"] <= fir["median"] / 8.0
    clean, dirty = survey["frames"][1], survey["frames"][0]
    out = {
        "steps": args.steps, "warmup": args.warmup,
        "command": "python tools/symbol_rate.py --log2-samples %d --log2-dense %d --steps %d --warmup %d"
                   % (args.log2_samples, args.log2_dense, args.steps, args.warmup),
        "symbol_ms": "HIP-event time of one ookd_rx_symbol_survey call: hipMemsetAsync of the result + symbol_kinds_kernel, "
                     "and with roles symbol_scan_kernel + symbol_frames_kernel (ookd_rx_symbol_kernel_ms)",
        "samples": n, "filter": "fs32_fs4", "device": "p3l-nexa2012", "threshold": THRESHOLD,
        "edges": int(st.num_edges), "symbols": int(survey["num_symbols"]), "messages": int(st.num_messages),
        "front_form": int(st.front_form),
        "symbol_ms_without_roles": summary(t_kinds), "symbol_ms_with_roles": roles,
        "pulse_ms": summary(t_pulse), "fir_kernel_ms": fir,
        "symbol_over_fir": round(roles["median"] / fir["median"], 6),
        "condition": "symbol_ms_with_roles.median <= fir_kernel_ms.median / 8", "condition_holds": bool(holds),
        "coding": {k: (float(v) if isinstance(v, float) else int(v)) for k, v in coding.items() if k != "roles"},
        "num_syncs": int(survey["num_syncs"]), "head_symbols": int(survey["head_symbols"]),
        "tail_symbols": int(survey["tail_symbols"]),
        "frames_clean": {str(int(d)): int(clean[d]) for d in np.nonzero(clean)[0]},
        "frames_not_clean": {str(int(d)): int(dirty[d]) for d in np.nonzero(dirty)[0]},
        "suggest_device": dict(suggestion, reason_text=ok.CODING_REASONS[suggestion["reason"]]),
    }
    rx.close()
    out = {k: out.pop(k) for k in ("steps", "warmup", "command", "symbol_ms")} | {"bench_capture": out}
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
    table = dict(lower=[[1, 16, 48], [1, 16, 48]], upper=[[15, 47, (1 << 35) - 1], [15, 47, (1 << 35) - 1]])
    roles = np.zeros((ok.SYMBOL_KINDS, ok.SYMBOL_KINDS), dtype=np.uint8)
    roles[0, 0], roles[1, 1], roles[2, 2] = ok.ROLE_ZERO, ok.ROLE_ONE, ok.ROLE_SYNC
    rx = ok.Receiver(None, None, max_samples=n, threshold=THRESHOLD, samples_per_buffer=SPB)
    t_kinds, t_roles, t_pulse, t_front = [], [], [], []
    for k in range(args.warmup + args.steps):
        rx.process_device(cap.data_ptr(), n)
        st = rx.raw_stats()
        rx.pulse_hist(0)
        rx.symbol_survey(table, None)
        ms_kinds = rx.symbol_kernel_ms
        survey = rx.symbol_survey(table, roles)
        if k >= args.warmup:
            t_kinds.append(ms_kinds)
            t_roles.append(rx.symbol_kernel_ms)
            t_pulse.append(rx.pulse_kernel_ms)
            t_front.append(float(st.fir_kernel_ms))
    with_roles = summary(t_roles)
    nbytes = 8 * int(st.num_edges)
    out["dense_capture"] = {
        "samples": n, "filter": None, "mean_run": 32, "edges": int(st.num_edges), "edge_list_bytes": nbytes,
        "default_edge_capacity": n // 32 + (1 << 20), "symbols": int(survey["num_symbols"]),
        "num_syncs": int(survey["num_syncs"]), "frames": int(survey["frames"].sum()),
        "frames_clean": int(survey["frames"][1].sum()), "occupied_kinds": int((survey["kinds"] != 0).sum()),
        "symbol_ms_without_roles": summary(t_kinds), "symbol_ms_with_roles": with_roles, "pulse_ms": summary(t_pulse),
        "front_kernel_ms": summary(t_front),
        "list_gbs_with_roles": round(2 * nbytes / (with_roles["median"] * 1e-3) / 1e9, 1),
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
