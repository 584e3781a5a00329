"""What the debounced decode (ookd_rx_set_debounce) costs a run, on the bench capture.

    python tools/debounce_rate.py [--parent-root DIR] [--log2-samples 32] [--steps 12] [--warmup 2] [--rounds 3]
                                  [--out profiles/debounce_rate.json]

One seeded capture made like bench.py's north_star capture (synthetic p3l-nexa2012 traffic, 2^32 samples) through
fs32_fs4 and the p3l-nexa2012 decoder at threshold 0.1, one context, one run per step.  A step's time is the host clock
around ookd_rx_process_device, which returns when the results are in host memory; the run's own total_device_ms (HIP
events, front end start to the chain's last kernel) is recorded beside it.

Every measurement runs in a process of its own that makes the capture from the seed, and the kinds alternate, `rounds`
times over, so that whatever else the machine is doing falls on all of them alike:

    parent_off   the library of the tree at --parent-root (a checkout of the parent commit, built): today's context
    off          this tree, debounce never set
    on           this tree, min_on = 250 us of decimated samples (750)
    clean        this tree, debounce off, the first clean_edges(min_on, 0) after every run: the pass's HIP-event time

Judged (exit status 1 when one fails; both are left null without --parent-root):
    off costs nothing   |off - parent_off| <= 5 % of parent_off        (medians of the step time over all rounds)
    on costs the pass   on <= parent_off + 2 * clean                   (clean: the median pass time)
Recorded: messages and errors decoded with the debounce off and on, and what the clean pass deleted.
"""
import argparse
import json
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
RATE, SPB, THRESHOLD, SEED = 3000000, 8192, 0.1, 0x00C0FFEE + 15
MIN_ON_US = 250.0


def median(v):
    v = sorted(v)
    m = len(v) // 2
    return v[m] if len(v) % 2 else 0.5 * (v[m - 1] + v[m])


def summary(v):
    return {"median": round(median(v), 5), "min": round(min(v), 5), "max": round(max(v), 5), "n": len(v)}


def worker(args):
    """one kind in this process: prints one JSON line"""
    root = os.path.abspath(args.root)
    sys.path.insert(0, root)
    import torch
    import ookiedokie_amd as ok
    assert os.path.abspath(os.path.dirname(os.path.dirname(ok.__file__))) == root, ok.__file__
    golden = os.path.join(root, "tests", "golden")
    n = 1 << args.log2_samples
    flt = ok.Filter.load(os.path.join(golden, "filters", "fs32_fs4.json"))
    min_on = int(MIN_ON_US * 1e-6 * RATE / flt.total_decimation)
    dev = ok.Device.load(os.path.join(golden, "devices", "p3l-nexa2012.json"), RATE // flt.total_decimation)
    syn = ok.Synth(dev, n, seed=SEED, sample_rate=RATE)
    cap = torch.empty(2 * n + 64, dtype=torch.int16, device="cuda")
    syn.fill_device(cap.data_ptr())
    torch.cuda.synchronize()
    kw = dict(min_on=min_on) if args.worker == "on" else {}
    rx = ok.Receiver(flt, dev, max_samples=n, threshold=THRESHOLD, samples_per_buffer=SPB, **kw)
    step, device, clean = [], [], []
    info = None
    for k in range(args.warmup + args.steps):
        t0 = time.perf_counter()
        rx.process_device(cap.data_ptr(), n)
        t1 = time.perf_counter()
        st = rx.raw_stats()
        if args.worker == "clean":
            info = rx.clean_edges(min_on, 0)[0]
        if k >= args.warmup:
            step.append((t1 - t0) * 1e3)
            device.append(float(st.total_device_ms))
            if args.worker == "clean":
                clean.append(rx.clean_kernel_ms)
    out = {"kind": args.worker, "step_ms": step, "total_device_ms": device, "clean_ms": clean, "min_on": min_on,
           "messages": int(st.num_messages), "errors": int(st.num_errors), "edges": int(st.num_edges),
           "fsm_path": int(st.fsm_path), "pipeline_chunks": int(st.pipeline_chunks), "samples": n}
    if args.worker == "on":
        info = rx.clean_edges(min_on, 0)[0]         # (the chain's own list: nothing is launched)
        out["clean_kernel_ms_after"] = rx.clean_kernel_ms
    if info is not None:
        out["edges_cleaned"] = info["edges_out"]
        out["deleted_off_on"] = info["deleted"]
    rx.close()
    print("DEBOUNCE_RATE " + json.dumps(out))


def run_worker(kind, root, args):
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", kind, "--root", root, "--log2-samples", str(args.log2_samples),
           "--steps", str(args.steps), "--warmup", str(args.warmup)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.worker_timeout)
    if r.returncode != 0:
        # (a failed or faulted child ends the measurement: nothing more is started)
        raise SystemExit("worker %s failed (%d):\n%s%s" % (kind, r.returncode, r.stdout[-2000:], r.stderr[-2000:]))
    line = next(ln for ln in r.stdout.splitlines() if ln.startswith("DEBOUNCE_RATE "))
    return json.loads(line[len("DEBOUNCE_RATE "):])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-root", default="")
    ap.add_argument("--log2-samples", type=int, default=32)
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(HERE, "..", "profiles", "debounce_rate.json"))
    ap.add_argument("--worker-timeout", type=float, default=240.0, help="seconds one measuring process may take")
    ap.add_argument("--worker", default="", help=argparse.SUPPRESS)
    ap.add_argument("--root", default=os.path.join(HERE, ".."), help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        return worker(args)

    here = os.path.abspath(os.path.join(HERE, ".."))
    kinds = ([("parent_off", args.parent_root)] if args.parent_root else []) + [("off", here), ("on", here), ("clean", here)]
    seen = {k: [] for k, _ in kinds}
    for r in range(args.rounds):
        for kind, root in kinds:
            res = run_worker("off" if kind == "parent_off" else kind, root, args)
            seen[kind].append(res)
            print("round %d %-10s step %.3f ms device %.3f ms, %d messages %d errors"
                  % (r, kind, median(res["step_ms"]), median(res["total_device_ms"]), res["messages"], res["errors"]), flush=True)

    def pooled(kind, key):
        return [x for res in seen[kind] for x in res[key]]

    out = {"steps": args.steps, "warmup": args.warmup, "rounds": args.rounds, "samples": 1 << args.log2_samples,
           "filter": "fs32_fs4", "device": "p3l-nexa2012", "threshold": THRESHOLD, "min_on": seen["on"][0]["min_on"], "min_off": 0,
           "command": "python tools/debounce_rate.py%s --log2-samples %d --steps %d --warmup %d --rounds %d"
                      % (" --parent-root <parent checkout>" if args.parent_root else "", args.log2_samples, args.steps,
                         args.warmup, args.rounds),
           "step_ms": "host clock around ookd_rx_process_device (one context, one run a step), pooled over the rounds; "
                      "per_round: each process's median",
           "kinds": {}}
    for kind, _ in kinds:
        last = seen[kind][-1]
        out["kinds"][kind] = {
            "step_ms": summary(pooled(kind, "step_ms")), "total_device_ms": summary(pooled(kind, "total_device_ms")),
            "per_round_step_ms": [round(median(res["step_ms"]), 5) for res in seen[kind]],
            "messages": last["messages"], "errors": last["errors"], "edges": last["edges"], "fsm_path": last["fsm_path"],
            "pipeline_chunks": last["pipeline_chunks"]}
        for key in ("edges_cleaned", "deleted_off_on", "clean_kernel_ms_after"):
            if key in last:
                out["kinds"][kind][key] = last[key]
    clean = summary(pooled("clean", "clean_ms"))
    out["kinds"]["clean"]["clean_ms"] = clean
    off, on = out["kinds"]["off"]["step_ms"]["median"], out["kinds"]["on"]["step_ms"]["median"]
    out["decode"] = {"off": {k: out["kinds"]["off"][k] for k in ("messages", "errors")},
                     "on": {k: out["kinds"]["on"][k] for k in ("messages", "errors")}}
    out["on_minus_off_ms"] = round(on - off, 5)
    holds = [True]
    if args.parent_root:
        parent = out["kinds"]["parent_off"]["step_ms"]["median"]
        out["off_costs_nothing"] = {"condition": "|off - parent_off| <= 0.05 parent_off", "off": off, "parent_off": parent,
                                    "relative": round((off - parent) / parent, 5), "holds": bool(abs(off - parent) <= 0.05 * parent)}
        out["on_costs_the_pass"] = {"condition": "on <= parent_off + 2 clean_ms", "on": on, "parent_off": parent,
                                    "clean_ms": clean["median"], "bound": round(parent + 2 * clean["median"], 5),
                                    "holds": bool(on <= parent + 2 * clean["median"])}
        holds = [out["off_costs_nothing"]["holds"], out["on_costs_the_pass"]["holds"]]
    else:
        out["off_costs_nothing"] = out["on_costs_the_pass"] = None
    path = os.path.abspath(args.out)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(out))
    if not all(holds):
        raise SystemExit(1)


if __name__ == "__main__":
    main()
