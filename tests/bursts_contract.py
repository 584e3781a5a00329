"""The burst extraction contract (include/ookiedokie_amd.h, "Burst extraction") restated in numpy and Python integers,
independent of the library: edge list -> burst table, and table + capture bytes -> the cut.  Shared by
tests/test_bursts_host.py and tests/test_gpu_bursts.py, with the designed edge lists and the margins of the round
trip through the reference decoder."""
import numpy as np

RATE = 3000000
SPB = 8192
THR = 0.1
FIELDS = ("first_sample", "num_samples", "offset", "first_run", "burst_runs")

# The round trip's margins for the golden captures, as times: `margins` turns them into decimated samples at the
# filter's output rate (fs32_fs4: D = 1, 3 MHz; fs128_fs16_dec4: D = 4, 750 kHz).  Chosen on the CPU against the
# reference decoder:
#   pre   200 us = 600 / 150 outputs, well beyond the filter's history in outputs (fs32_fs4: one stage of 32 taps, 31
#         outputs; fs128_fs16_dec4: 16 and 32 taps in front of two decimations by 2, 20 outputs): the outputs of a cut
#         burst that see the previous burst's tail in the place of the capture's own silence all lie in this margin,
#         below the threshold either way;
#   post  the devices' longest timeout (p3l-nexa2012: 16.4 ms, unknown-remote1: 17.8 ms) and a little more, so the
#         state machine has fallen back to idle inside the burst exactly as it does in the whole capture, and a message
#         that is complete only at a timeout has its `sample` inside the burst;
#   max_gap = pre + post, the smallest the contract takes: no off-run inside a message is that long.
LONGEST_TIMEOUT_US = 17800
PRE_US = 200
POST_US = LONGEST_TIMEOUT_US + 600


def margins(decimation, rate=RATE):
    """(pre, post, max_gap) in decimated samples at rate / decimation"""
    out_rate = rate // decimation
    pre = PRE_US * out_rate // 1000000
    post = POST_US * out_rate // 1000000
    return pre, post, pre + post


def bursts_of(edges, n_out, D, n, pre, post, max_gap):
    """the rule: -> a list of dicts (first_sample, num_samples, offset, first_run, burst_runs, lo, hi), all Python ints"""
    e = [int(x) for x in np.asarray(edges, dtype=np.uint64)]
    n_out, D, n, pre, post, max_gap = int(n_out), int(D), int(n), int(pre), int(post), int(max_gap)
    assert max_gap >= pre + post and D >= 1
    E = len(e)
    R = -(-E // 2)
    a = [e[2 * r] for r in range(R)]
    f = [e[2 * r + 1] if 2 * r + 1 < E else n_out for r in range(R)]
    starts = [r for r in range(R) if r == 0 or a[r] - f[r - 1] > max_gap]
    out, offset = [], 0
    for k, r0 in enumerate(starts):
        r1 = (starts[k + 1] if k + 1 < len(starts) else R) - 1
        lo = a[r0] - min(a[r0], pre)
        hi = min(n_out, f[r1] + post)
        first, end = min(n, lo * D), min(n, hi * D)
        out.append(dict(first_sample=first, num_samples=end - first, offset=offset, first_run=r0, burst_runs=r1 - r0 + 1,
                        lo=lo, hi=hi))
        offset += end - first
    return out


def table_of(bursts):
    """the restatement's table as the library's dict of uint64 arrays"""
    return {k: np.array([b[k] for b in bursts], dtype=np.uint64) for k in FIELDS}


def total_of(bursts):
    return sum(b["num_samples"] for b in bursts)


def cut_of(capture, bursts):
    """capture: [n, 2] of the format's dtype -> the cut, [total, 2]"""
    c = np.asarray(capture).reshape(-1, 2)
    parts = [c[b["first_sample"]:b["first_sample"] + b["num_samples"]] for b in bursts]
    return np.concatenate(parts) if parts else c[:0]


def assert_table(got, bursts, what=""):
    want = table_of(bursts)
    assert got["num_bursts"] == len(bursts), (what, got["num_bursts"], len(bursts))
    assert got["total_samples"] == total_of(bursts), (what, got["total_samples"], total_of(bursts))
    for k in FIELDS:
        assert got[k].dtype == np.uint64 and got[k].tolist() == want[k].tolist(), (what, k, got[k].tolist()[:8], want[k].tolist()[:8])


def mapped_samples(msg_samples, bursts, D):
    """where the messages of the whole capture fall in the cut, in decimated samples: sample - lo_b + offset_b / D for
    the burst whose [lo, hi) holds the sample; -> (the mapped samples, each message's burst)"""
    out, which = [], []
    for s in (int(x) for x in msg_samples):
        b = [k for k, x in enumerate(bursts) if x["lo"] <= s < x["hi"]]
        assert len(b) == 1, ("a message outside every burst", s)
        x = bursts[b[0]]
        assert x["offset"] % D == 0
        out.append(s - x["lo"] + x["offset"] // D)
        which.append(b[0])
    return out, which


# ---- the designed edge lists: (name, edges, n_out, D, n, pre, post, max_gap) ---------------------------------------

def designed_cases():
    cases = [
        ("E=0", [], 1000, 1, 1000, 3, 4, 10),
        ("E=1 open", [40], 1000, 1, 1000, 3, 4, 10),
        ("E=2", [40, 50], 1000, 1, 1000, 3, 4, 10),
        ("odd E, open last run", [40, 50, 100, 120, 900], 1000, 1, 1000, 3, 4, 10),
        ("gap of exactly max_gap joins", [40, 50, 60, 70], 1000, 1, 1000, 3, 4, 10),
        ("gap of max_gap + 1 splits", [40, 50, 61, 70], 1000, 1, 1000, 3, 4, 10),
        ("pre beyond the first rise", [2, 50], 1000, 1, 1000, 30, 4, 40),
        ("rise at 0", [0, 50, 400, 410], 1000, 1, 1000, 30, 4, 40),
        ("post beyond n_out", [40, 50, 990, 998], 1000, 1, 1000, 3, 40, 50),
        ("n_out D > n: clipped at n", [40, 50, 900, 960], 1000, 4, 3700, 3, 20, 30),
        ("a burst wholly in the padding", [40, 50, 950, 960], 1000, 4, 3700, 3, 4, 10),
        ("two bursts in the padding", [40, 50, 950, 960, 980, 990], 1000, 4, 3700, 3, 4, 10),
        ("every run its own burst", [10 + 100 * k + d for k in range(9) for d in (0, 5)], 1000, 2, 2000, 2, 3, 5),
        ("all runs one burst", [10 + 100 * k + d for k in range(9) for d in (0, 5)], 1000, 2, 2000, 20, 30, 95),
        ("zero margins, adjacent bursts", [10, 20, 21, 30, 31, 40], 1000, 1, 1000, 0, 0, 0),
        ("pre + post = max_gap, bursts that touch", [10, 20, 28, 30], 1000, 3, 3000, 3, 4, 7),
    ]
    return cases


def random_case(rng):
    R = int(rng.integers(0, 40))
    D = int(rng.choice([1, 1, 2, 4, 8]))
    e, pos = [], int(rng.integers(0, 6))
    for _ in range(R):
        on = int(rng.integers(1, 30))
        off = int(rng.integers(1, 60))
        e += [pos, pos + on]
        pos += on + off
    if e and rng.integers(0, 3) == 0:
        e = e[:-1]                                              # an open last run
    n_out = (e[-1] + 1 if e else 0) + int(rng.integers(0, 50))
    n = max(0, n_out * D - int(rng.integers(0, 3)) * int(rng.integers(0, 40 * D)))
    pre, post = int(rng.integers(0, 12)), int(rng.integers(0, 12))
    max_gap = pre + post + int(rng.integers(0, 30))
    return ("random", e, n_out, D, n, pre, post, max_gap)
