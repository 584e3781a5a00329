"""The pulse survey's contract (include/ookiedokie_amd.h, "Pulse survey") restated in numpy and Python integers,
independent of the library: the bin rule, its inverse, edges + n_out -> histogram, and the class rule.  Shared by
tests/test_pulses_host.py and tests/test_gpu_pulses.py."""
import numpy as np

BINS = 512
CLASS_GAP = 2
MAX_CLASSES = 16
RATE = 3000000
THR = 0.1
SPB = 8192

# the issue's table: decimated run lengths of the golden captures at threshold 0.1, samples_per_buffer 8192, clean
# and with +-40 LSB of noise alike: {(capture, filter): (edges, on-runs, off-runs)}, runs as {length: count}
TABLE = {
    ("G1", "fs32_fs4"): (228, {1503: 114}, {5997: 60, 11997: 50, 26097: 3}),
    ("G1", "fs128_fs16_dec4"): (228, {378: 114}, {1497: 60, 2997: 50, 6522: 3}),
    ("G2", "fs32_fs4"): (136, {1653: 66, 26703: 2}, {1647: 34, 5097: 30, 11997: 1, 13197: 2}),
    ("G2", "fs128_fs16_dec4"): (136, {415: 32, 416: 34, 6678: 2}, {(409, 410): 34, 1272: 30, 2997: 1, 3297: 2}),
}


def py_bin(d):
    """1 .. 31 -> d; d >= 32 -> 32 + 16 (o - 5) + ((d >> (o - 4)) & 15) with o = floor(log2 d), clamped to 511"""
    d = int(d)
    if d < 32:
        return d
    o = d.bit_length() - 1
    return min(32 + 16 * (o - 5) + ((d >> (o - 4)) & 15), BINS - 1)


def py_bin_lower(b):
    b = int(b)
    if b < 32:
        return b
    return min((16 + (b - 32) % 16) << (1 + (b - 32) // 16), (1 << 64) - 1)


def np_bins(d):
    d = np.asarray(d, dtype=np.uint64)
    out = d.astype(np.int64)
    big = d >= 32
    if big.any():
        v = d[big]
        o = np.zeros(v.size, dtype=np.int64)
        for s in (32, 16, 8, 4, 2, 1):                  # floor(log2 v), integers only
            m = (v >> (o + s).astype(np.uint64)) != 0
            o[m] += s
        out[big] = 32 + 16 * (o - 5) + ((v >> (o - 4).astype(np.uint64)) & np.uint64(15)).astype(np.int64)
    return np.minimum(out, BINS - 1)


def hist_of(edges, n_out):
    """the contract: closed run i = e[i+1] - e[i], level 1 for even i; the open runs aside"""
    e = np.asarray(edges, dtype=np.uint64)
    E = int(e.size)
    count = np.zeros((2, BINS), dtype=np.uint64)
    total = np.zeros((2, BINS), dtype=np.uint64)
    if E > 1:
        d = e[1:] - e[:-1]
        assert (e[1:] > e[:-1]).all(), "an edge list is strictly increasing"
        b = np_bins(d)
        lv = 1 - (np.arange(E - 1) & 1)
        for level in (0, 1):
            m = lv == level
            count[level] = np.bincount(b[m], minlength=BINS).astype(np.uint64)
            # (sums stay far below 2^53 here: float64 weights are exact)
            total[level] = np.bincount(b[m], weights=d[m].astype(np.float64), minlength=BINS).astype(np.uint64)
    return dict(num_edges=E, samples=int(n_out), runs=count.sum(axis=1), count=count, sum=total,
                open_head=int(e[0]) if E else int(n_out), open_tail=int(n_out) - int(e[-1]) if E else 0,
                tail_level=E & 1)


def assert_same_hist(got, want, what=""):
    for key in ("num_edges", "samples", "open_head", "open_tail", "tail_level"):
        assert got[key] == want[key], (what, key, got[key], want[key])
    for key in ("runs", "count", "sum"):
        g, w = np.asarray(got[key]), np.asarray(want[key])
        assert g.shape == w.shape and g.dtype == np.uint64, (what, key)
        diff = np.argwhere(g != w)
        assert diff.size == 0, (what, key, diff[:6].tolist(), g[g != w][:6], w[g != w][:6])


def runs_of(hist, level):
    """{bin: (count, sum)} of the occupied bins"""
    c, s = hist["count"][level], hist["sum"][level]
    return {int(b): (int(c[b]), int(s[b])) for b in np.nonzero(c)[0]}


def py_suggest(hist, rate):
    """the header's class rule"""
    out = dict(found=1, dropped_runs=[0, 0], classes=[[], []])
    for lv in (0, 1):
        c = [int(x) for x in hist["count"][lv]]
        s = [int(x) for x in hist["sum"][lv]]
        classes, last = [], None
        for b in range(BINS):
            if not c[b]:
                continue
            if last is None or not b - last < CLASS_GAP:
                classes.append(dict(first_bin=b, last_bin=b, runs=0, total=0))
            k = classes[-1]
            k["last_bin"] = b
            k["runs"] += c[b]
            k["total"] += s[b]
            last = b
        if len(classes) > MAX_CLASSES:
            order = sorted(range(len(classes)), key=lambda i: (-classes[i]["runs"], i))
            out["dropped_runs"][lv] = sum(classes[i]["runs"] for i in order[MAX_CLASSES:])
            classes = [classes[i] for i in sorted(order[:MAX_CLASSES])]
        us = (lambda x: x / rate * 1e6) if rate > 0 else (lambda x: 0.0)
        for k in classes:
            k["mean"] = k["total"] / k["runs"]
            k["lower"] = py_bin_lower(k["first_bin"])
            k["upper"] = py_bin_lower(k["last_bin"] + 1) - 1
            k["mean_us"], k["lower_us"], k["upper_us"] = us(k["mean"]), us(k["lower"]), us(k["upper"])
            del k["total"]
        out["classes"][lv] = classes
        if not any(k["runs"] >= 2 for k in classes):
            out["found"] = 0
    return out


def assert_same_suggestion(got, want):
    import pytest
    assert got["found"] == want["found"] and got["dropped_runs"] == want["dropped_runs"], (got, want)
    for lv in (0, 1):
        assert len(got["classes"][lv]) == len(want["classes"][lv]), (lv, got["classes"][lv], want["classes"][lv])
        for g, w in zip(got["classes"][lv], want["classes"][lv]):
            for key in ("first_bin", "last_bin", "runs", "lower", "upper"):
                assert g[key] == w[key], (lv, key, g, w)
            for key in ("mean", "mean_us", "lower_us", "upper_us"):
                assert g[key] == pytest.approx(w[key], rel=1e-12, abs=0), (lv, key, g, w)


def golden_iq(vectors, name, noise_seed=None, noise=40):
    """golden capture G1 / G2 as int16 I,Q, clean or with +-noise LSB of uniform noise on both rails"""
    from tests.helpers import iq_from_rle
    g = vectors[name]
    iq = iq_from_rle(g["i_rle"], g["num_samples"]).astype(np.int32)
    if noise_seed is not None:
        iq = iq + np.random.default_rng(noise_seed).integers(-noise, noise + 1, size=iq.size)
    return np.clip(iq, -32768, 32767).astype(np.int16)


def oracle_edges(oracle, iq, filter_name, thr=THR, spb=SPB):
    """(edges, n_out) of the reference path's bit stream"""
    from tests.helpers import edges_of, golden_path
    fir = oracle.load_filter_json(golden_path("filters", filter_name)) if filter_name else None
    r = oracle.rx(iq, fir, thr, None, spb, want_bits=True)
    return edges_of(r.bits).astype(np.uint64), r.decimated
