"""Front-end kernel time of a carrier context (OOKD_FRONT_TUNED_MULTI) against the K single-nu tuned contexts it
replaces (OOKD_FRONT_TUNED_FIR1 each).

    python tools/carriers_rate.py [--log2-samples 32] [--steps 12] [--warmup 3] [--commit ID]
                                  [--out profiles/carriers_rate.json]

One seeded synthetic capture made by tools/tuned_rate.py's recipe (p3l-nexa2012 traffic, noise +-40 LSB), fs32_fs4,
threshold 0.1 for every carrier, carrier nu taken in order from NUS.  For the quiet shortcut and for
OOKD_RX_NO_QUIET_SKIP: eight single-nu contexts and four carrier contexts (K = 1, 2, 4, 8) in one process, taking
turns with one run in flight.  Times are the library's HIP-event span of the front-end kernel launches of a run
(stats fir_kernel_ms); medians and min-max over the steps are written.  A carrier context of K carriers is compared
with the sum of the first K single-nu contexts' times (its spread: min-max of the per-step sums).

Judged: at K = 4, in both pairs, the carrier context's median lies below that sum's median by more than the larger of
the two min-max spreads.  Recorded only: K = 1 (Receiver(tune=nu) stays the way to decode one carrier), and the
least-squares fit of the carrier contexts' medians to t0 + K t1 (what all carriers share / what each one adds).
No state machine runs (device = None): only the front end is timed, and a context's buffers stay small.
"""
import argparse
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
RATE, SPB, THRESHOLD, SEED = 3000000, 8192, 0.1, 0x00C0FFEE + 13
NUS = [0.2, -0.2, 0.35, -0.35, 0.1, -0.1, 0.45, -0.45]
KS = [1, 2, 4, 8]


def summary(v):
    v = sorted(v)
    m = len(v) // 2
    med = v[m] if len(v) % 2 else 0.5 * (v[m - 1] + v[m])
    return {"median": round(med, 4), "min": round(v[0], 4), "max": round(v[-1], 4)}


def fit_line(ks, ts):
    """least squares t = t0 + k t1"""
    n = float(len(ks))
    sk, st = sum(ks), sum(ts)
    skk, skt = sum(k * k for k in ks), sum(k * t for k, t in zip(ks, ts))
    t1 = (n * skt - sk * st) / (n * skk - sk * sk)
    return (st - t1 * sk) / n, t1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2-samples", type=int, default=32)
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--commit", default=None, help="what the run is recorded under (default: git rev-parse HEAD)")
    ap.add_argument("--out", default=os.path.join(HERE, "..", "profiles", "carriers_rate.json"))
    args = ap.parse_args()
    n = 1 << args.log2_samples
    commit = args.commit
    if commit is None:
        r = subprocess.run(["git", "-C", HERE, "rev-parse", "HEAD"], capture_output=True, text=True)
        commit = r.stdout.strip() if r.returncode == 0 else "unknown"

    # the command as recorded: what decides the measurement, not where the result was written
    shown = ["--log2-samples", str(args.log2_samples), "--steps", str(args.steps), "--warmup", str(args.warmup),
             "--commit", repr(commit)]
    command = "python tools/carriers_rate.py " + " ".join(shown)

    sys.path.insert(0, os.path.abspath(os.path.join(HERE, "..")))
    import torch
    import ookiedokie_amd as ok
    golden = os.path.join(HERE, "..", "tests", "golden")
    dev = ok.Device.load(os.path.join(golden, "devices", "p3l-nexa2012.json"), RATE)
    flt = ok.Filter.load(os.path.join(golden, "filters", "fs32_fs4.json"))
    syn = ok.Synth(dev, n, seed=SEED, sample_rate=RATE)
    buf = torch.empty(2 * n + 64, dtype=torch.int16, device="cuda")
    syn.fill_device(buf.data_ptr())
    torch.cuda.synchronize()

    out = {"samples": n, "filter": "fs32_fs4", "threshold": THRESHOLD, "nus": NUS, "steps": args.steps,
           "warmup": args.warmup, "commit": commit, "command": command,
           "time": "HIP-event span of the front-end kernel launches of one run (stats fir_kernel_ms), ms"}
    common = dict(max_samples=n, threshold=THRESHOLD, samples_per_buffer=SPB, edge_capacity=1 << 24)
    for quiet in (True, False):
        single = [ok.Receiver(flt, None, tune=nu, quiet_skip=quiet, count_quiet=True, **common) for nu in NUS]
        multi = {K: ok.Receiver(flt, None, carriers=NUS[:K], quiet_skip=quiet, count_quiet=True, **common) for K in KS}
        t_single = [[] for _ in NUS]
        t_multi = {K: [] for K in KS}
        waves = {}
        for step in range(args.warmup + args.steps):
            for i, rx in enumerate(single):                 # the forms taking turns
                rx.process_device(buf.data_ptr(), n)
                st = rx.raw_stats()
                assert int(st.front_form) == ok.FRONT_TUNED_FIR1
                if step >= args.warmup:
                    t_single[i].append(float(st.fir_kernel_ms))
                waves[("single", i)] = (int(st.quiet_waves), int(st.total_waves), int(st.front_launches))
            for K, rx in multi.items():
                rx.process_device(buf.data_ptr(), n)
                st = rx.raw_stats()
                assert int(st.front_form) == ok.FRONT_TUNED_MULTI
                if step >= args.warmup:
                    t_multi[K].append(float(st.fir_kernel_ms))
                waves[("multi", K)] = (int(st.quiet_waves), int(st.total_waves), int(st.front_launches))
        per = {"single": [dict(nu=NUS[i], fir_kernel_ms=summary(t_single[i]), quiet_waves=waves[("single", i)][0],
                               total_waves=waves[("single", i)][1], front_launches=waves[("single", i)][2])
                          for i in range(len(NUS))]}
        for K in KS:
            sums = [sum(t_single[i][s] for i in range(K)) for s in range(args.steps)]
            m, s = summary(t_multi[K]), summary(sums)
            spread = max(m["max"] - m["min"], s["max"] - s["min"])
            per["K%d" % K] = {"multi_fir_kernel_ms": m, "sum_of_singles_ms": s,
                              "multi_over_sum": round(m["median"] / s["median"], 3),
                              "saved_ms": round(s["median"] - m["median"], 4), "larger_spread_ms": round(spread, 4),
                              "below_by_more_than_the_spread": bool(s["median"] - m["median"] > spread),
                              "quiet_waves": waves[("multi", K)][0], "total_waves": waves[("multi", K)][1],
                              "front_launches": waves[("multi", K)][2]}
        t0, t1 = fit_line(KS, [per["K%d" % K]["multi_fir_kernel_ms"]["median"] for K in KS])
        per["fit_t0_plus_K_t1_ms"] = {"t0_shared": round(t0, 4), "t1_per_carrier": round(t1, 4)}
        out["quiet_shortcut" if quiet else "every_window"] = per
        for rx in single + list(multi.values()):
            rx.close()
    out["pass_K4"] = bool(out["quiet_shortcut"]["K4"]["below_by_more_than_the_spread"] and
                          out["every_window"]["K4"]["below_by_more_than_the_spread"])
    path = os.path.abspath(args.out)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
