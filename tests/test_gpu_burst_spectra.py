"""Burst spectra on the GPU (ookd_rx_burst_spectra and its getters; burst_spectra.hip).  Every comparison is against the
numpy float64 restatement (tests/burst_spectra_contract.py) of the capture and the burst table the library returned --
the table itself is pinned by tests/test_gpu_bursts.py.  Per burst the 1024 doubles of `burst_spectrum` are within the
spectrum section's bound B of the float64 spectrum of the burst's whole frames (worst |err| / B is printed and must be
below 1), and the summary has the exact relations of the contract against those doubles.

Of the issue's designed cases one cannot be made on a context without a filter: a burst wholly in the padding
(num_samples = 0) needs a rise in the padding, which holds zeros (tests/test_gpu_bursts.py says the same of its table
tests).  The kernels' handling of such an entry (no frames, nothing read) is the same branch as that of a burst of
1 .. 1023 samples, which is tested.  The demonstration's capture is the issue's -- 2^20 silent samples, G1, G2 --
and so has 2.8 million samples, more than the 2^21 the other captures stay below."""
import subprocess

import numpy as np
import pytest

from tests.burst_spectra_contract import (FIELDS, N, assert_summary_of, bound, np_burst_spectrum, np_summary, peak_is_decided,
                                          py_suggest_burst_carriers, span_rule, spans_of, worst_over_bound)
from tests.bursts_contract import RATE, SPB, THR
from tests.helpers import golden_path
from tests.spectrum_contract import DC, NOISE
from tests.tuned_contract import golden_capture, moved, to_8bit

pytestmark = pytest.mark.gpu

GUARD_BIN = 37                          # the full-scale tone around a capture that must never show


@pytest.fixture(scope="module")
def ok():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from ookiedokie_amd import build as okbuild
    okbuild.build()
    import ookiedokie_amd as okm
    okm.lib()
    return okm


def keyed_tones(n, runs, seed=0, amp=900.0):
    """n samples [n, 2] int16: +-40 LSB of noise and a small DC term everywhere, and in every run (first, length, bin) a
    tone of `amp` LSB a quarter bin off the centre of `bin`.  At threshold 0.1 (204.8 LSB) the capture is on exactly in
    the runs: the off samples stay below 40 sqrt(2) + 45, the on samples above amp - that."""
    rng = np.random.default_rng(seed)
    z = rng.integers(-NOISE, NOISE + 1, size=n) + 1j * rng.integers(-NOISE, NOISE + 1, size=n) + (30 + 15j)
    for first, length, k in runs:
        t = np.arange(first, first + length, dtype=np.float64)
        z[first:first + length] += amp * np.exp(2j * np.pi * (((k + 0.25) / N * t) % 1.0))
    return np.stack([np.rint(z.real), np.rint(z.imag)], axis=1).astype(np.int16)


def guard_tone(count):
    t = np.arange(count, dtype=np.float64)
    z = 32000.0 * np.exp(2j * np.pi * ((GUARD_BIN / N * t) % 1.0))
    return np.stack([np.rint(z.real), np.rint(z.imag)], axis=1).astype(np.int16)


def on_device(cap, front=1027, behind=4096):
    """the capture in device memory between two guard regions of a full-scale tone on GUARD_BIN: the capture ends where
    the rear guard begins, and begins `front` samples (not a multiple of four: no 16-byte alignment) into the buffer
    -> (the tensor that owns the memory, the capture's pointer)"""
    import torch
    cap = np.ascontiguousarray(cap).reshape(-1, 2)
    if cap.dtype == np.int16:
        g0, g1 = guard_tone(front), guard_tone(behind)
    else:
        hi = 127 if cap.dtype == np.int8 else 255
        g0, g1 = np.full((front, 2), hi, cap.dtype), np.full((behind, 2), hi, cap.dtype)
    t = torch.from_numpy(np.concatenate([g0, cap, g1])).cuda()
    return t, t.data_ptr() + front * 2 * cap.dtype.itemsize


def check(ok, rx, iq16, c, table, span=0, what="", every=1):
    """capture (or carrier) c's burst spectra against numpy over the SC16Q11 capture iq16 and the library's table
    -> (the spectra dict, [(F_b, S_b)], worst |err| / B over the bursts looked at and the keyed spectrum)"""
    sp = rx.burst_spectra(c, span)
    nb = int(table["num_bursts"])
    assert sp["num_bursts"] == nb and all(sp[k].shape == (nb,) for k in FIELDS), what
    want = [np_burst_spectrum(iq16, table["first_sample"][b], table["num_samples"][b]) for b in range(nb)]
    assert sp["frames"].tolist() == [F for F, _ in want] == [int(x) // N for x in table["num_samples"]], what
    assert sp["total_frames"] == sum(F for F, _ in want), what
    total = int(table["total_samples"])
    used = span_rule(total, span)
    assert sp["span_frames"] == used and sp["spans"] == (spans_of(total, used) if nb else 0), (what, sp["span_frames"], sp["spans"])
    assert sp["partial_rows"] == 2 * sp["spans"] and sp["flags"] == table["flags"], what
    worst = 0.0
    for b in range(0, nb, every):
        F, S = want[b]
        power = rx.burst_spectrum(b, c)
        assert power.shape == (N,) and power.dtype == np.float64 and np.isfinite(power).all()
        w = worst_over_bound(power, S)
        assert w < 1.0, (what, "burst", b, F, w)
        worst = max(worst, w)
        entry = dict((k, sp[k][b]) for k in FIELDS)
        assert_summary_of(entry, power, F, (what, b))
        if F and peak_is_decided(S):
            assert int(entry["peak_bin"]) == np_summary(S, F)["peak_bin"], (what, b)
    keyed = rx.keyed_spectrum(c)
    S_all = np.sum([S for _, S in want], axis=0) if nb else np.zeros(N)
    power = np.frombuffer(bytes(keyed.power), dtype=np.float64)
    assert int(keyed.frames) == sp["total_frames"], what
    w = worst_over_bound(power, S_all)
    assert w < 1.0, (what, "keyed", w)
    worst = max(worst, w)
    print("worst |power - S| / B", what, "span", sp["span_frames"], worst)
    return sp, want, worst


# ------------------------------------------------------------------- 1. designed bursts, no span is crossed ----

def test_designed_bursts(ok, record_property):
    n = 1 << 18
    runs = [(4096, 1024, 100), (8193, 1025, 200), (12290, 2047, 300), (16387, 3000, -150 % N), (24000, 1, 50),
            (24100, 500, 60), (26001, 1023, 70), (30003, 5000, 400), (40000, 2048, 500), (n - 4097, 4097, -300 % N)]
    cap = keyed_tones(n, runs, seed=1)
    keep, ptr = on_device(cap)
    rx = ok.Receiver(None, None, max_samples=n, threshold=THR)
    rx.rx_device(ptr, n)
    assert rx.burst_spectra_kernel_ms == 0.0                    # nobody has asked about this run yet
    t = rx.bursts(0, 0, 0)[0]                                   # no margins: a burst is a run
    assert t["first_sample"].tolist() == [r[0] for r in runs] and t["num_samples"].tolist() == [r[1] for r in runs]
    assert sorted(set(int(x) % 4 for x in t["first_sample"])) == [0, 1, 2, 3]
    assert int(t["first_sample"][-1] + t["num_samples"][-1]) == n   # the last burst ends at the capture's last sample
    sp, want, worst = check(ok, rx, cap, 0, t, what="designed")
    record_property("worst_over_bound", worst)
    assert rx.burst_spectra_kernel_ms > 0.0
    assert sp["frames"].tolist() == [1, 1, 1, 2, 0, 0, 0, 4, 2, 4] and sp["spans"] == 1
    for b, (first, length, k) in enumerate(runs):
        if length >= N:
            assert int(sp["peak_bin"][b]) in (k, (k + 1) % N), (b, k)       # a quarter bin off the centre
            # the guards' tone does not show: its bin holds what the float64 spectrum of the burst alone says
            power = rx.burst_spectrum(b)
            S = want[b][1]
            assert abs(power[GUARD_BIN] - S[GUARD_BIN]) <= bound(S)[GUARD_BIN] and S[GUARD_BIN] < 1e-3 * S.max(), b
        else:
            assert all(float(sp[f][b]) == 0.0 for f in FIELDS)
    # the keyed spectrum is a spectrum: the carrier suggestion takes it and finds the strongest tones
    carriers, floor = ok.suggest_carriers(rx.keyed_spectrum(0))
    assert floor > 0.0 and carriers and carriers[0].bin in (400, 401, -300, -299)
    rx.close()
    del keep


# ----------------------------------------------------------------------------------------------- 2. spans ----

def _span_layout():
    """runs whose bursts (no margins) cross the spans of 32 frames as the issue lists them -> (runs, n)"""
    lengths = [32 * N,              # exactly one span, from a span boundary (the cut begins with it)
               33 * N,              # from a boundary, one frame into the next span
               100 * N + 300,       # crosses three boundaries
               N, N + 6, N + 476,   # three bursts of one frame, between two bursts that cross spans, in one span
               70 * N + 5,          # ... and runs on over two boundaries
               31 * N + 1000, 65 * N + 17, 700]
    runs, pos = [], 2051
    for k, length in enumerate(lengths):
        runs.append((pos, length, (90 + 83 * k) % (N - 4) + 2))
        pos += length + 150 + k     # first_sample mod 4 varies
    return runs, 1 << 19


def test_spans(ok, record_property):
    runs, n = _span_layout()
    assert runs[-1][0] + runs[-1][1] < n
    cap = keyed_tones(n, runs, seed=2)
    rx = ok.Receiver(None, None, max_samples=n, threshold=THR)
    rx.rx(np.ascontiguousarray(cap).reshape(-1))
    t = rx.bursts(0, 0, 0)[0]
    assert t["num_samples"].tolist() == [r[1] for r in runs]
    off = [int(x) for x in t["offset"]]
    W = 32 * N
    span_of = lambda b, f: (off[b] + N * f) // W
    frames = [r[1] // N for r in runs]
    # the layout is what the comments of _span_layout say it is
    assert off[0] == 0 and off[1] == W and span_of(1, 32) == 2 and span_of(2, 99) - span_of(2, 0) == 3
    assert span_of(2, 99) == span_of(3, 0) == span_of(4, 0) == span_of(5, 0) == span_of(6, 0) < span_of(6, 69)
    results = {}
    for span in (32, 64, 128):
        sp, want, worst = check(ok, rx, cap, 0, t, span=span, what="spans")
        record_property("worst_over_bound_%d" % span, worst)
        assert sp["frames"].tolist() == frames and sp["span_frames"] == span
        assert sp["spans"] == -(-int(t["total_samples"]) // (span * N)) and sp["partial_rows"] == 2 * sp["spans"]
        results[span] = [rx.burst_spectrum(b) for b in range(len(runs))]
    assert results[32][2].tolist() != results[128][2].tolist()      # another order of the same sums ...
    for b, (F, S) in enumerate(want):                               # ... within the bound of each other
        B = bound(S)
        for x, y in ((32, 64), (64, 128), (32, 128)):
            assert (np.abs(results[x][b] - results[y][b]) <= 2.0 * B).all(), (b, x, y)
    # 0 takes 32 for this cut, and launches nothing when 32 was the last one asked for
    rx.burst_spectra(0, 32)
    ms = rx.burst_spectra_kernel_ms
    assert rx.burst_spectra(0, 0)["span_frames"] == 32 and rx.burst_spectra_kernel_ms == ms
    for bad in (31, 48, 16, 1):
        with pytest.raises(ok.OokdError) as err:
            rx.burst_spectra(0, bad)
        assert err.value.code == -1 and "power of two" in str(err.value)
    assert rx.burst_spectra(0, 0)["span_frames"] == 32 and rx.burst_spectra_kernel_ms == ms     # a refusal changes nothing
    rx.close()


def test_the_fold_inside_one_span(ok, record_property):
    """one burst of 200 frames: at a span of 256 frames a wave sums 50 frames of it, beyond the 32 it may hold in fp32"""
    n = 1 << 18
    runs = [(101, 200 * N + 77, 333)]
    cap = keyed_tones(n, runs, seed=3)
    rx = ok.Receiver(None, None, max_samples=n, threshold=THR)
    rx.rx(np.ascontiguousarray(cap).reshape(-1))
    t = rx.bursts(0, 0, 0)[0]
    assert t["num_samples"].tolist() == [200 * N + 77]
    for span in (256, 128, 32):
        sp, want, worst = check(ok, rx, cap, 0, t, span=span, what="fold")
        record_property("worst_over_bound_%d" % span, worst)
        assert sp["spans"] == -(-(200 * N + 77) // (span * N)) and sp["frames"].tolist() == [200]
    rx.close()


# ------------------------------------------------------------------------------ 4. formats and contexts ----

@pytest.mark.parametrize("fmt", ["cs8", "cu8"])
def test_8bit_formats_in_place(ok, record_property, fmt):
    n = 1 << 17
    runs = [(1001, 3 * N + 9, 120), (6002, 40 * N + 3, 700), (50003, 2 * N, 250), (60000, 900, 10), (n - 2 * N - 2, 2 * N + 2, 900)]
    raw, wide = to_8bit(keyed_tones(n, runs, seed=4, amp=1800.0).reshape(-1), fmt)      # (1/20: on 90, off below 5)
    keep, ptr = on_device(raw.reshape(-1, 2))
    rx = ok.Receiver(None, None, max_samples=n, threshold=0.4, sample_format=fmt)
    rx.rx_device(ptr, n)
    t = rx.bursts(0, 0, 0)[0]
    assert t["first_sample"].tolist() == [r[0] for r in runs] and t["num_samples"].tolist() == [r[1] for r in runs]
    assert t["sample_bytes"] == 2
    sp, want, worst = check(ok, rx, wide, 0, t, what=fmt)
    record_property("worst_over_bound", worst)
    assert sp["frames"].tolist() == [3, 40, 2, 0, 2] and sp["spans"] == 2
    rx.close()
    del keep


def test_batch_of_three_middle_empty(ok):
    import torch
    n, stride = 40000, 41003
    runs = [[(1000, 5000, 100), (9001, 2500, 300), (20002, 1024, 500)], [], [(3, 2048, 50), (n - 3001, 3001, 800)]]
    caps = [keyed_tones(n, r, seed=10 + c) for c, r in enumerate(runs)]
    host = np.stack([np.concatenate([caps[c], guard_tone(stride - n)]) for c in range(3)])
    dev_t = torch.from_numpy(host).cuda()
    rx = ok.Receiver(None, None, max_samples=n, max_captures=3, threshold=THR)
    rx.rx_device(dev_t.data_ptr(), n, num_captures=3, stride=stride)
    tables = rx.bursts(0, 0, 0)
    assert [t["num_bursts"] for t in tables] == [3, 0, 2]
    for c in (2, 0, 1):
        sp, want, worst = check(ok, rx, caps[c], c, tables[c], what="capture %d" % c)
    empty = rx.burst_spectra(1)                                 # no edges: a valid result of no bursts
    assert empty["num_bursts"] == 0 and empty["total_frames"] == 0 and empty["spans"] == 0
    keyed = rx.keyed_spectrum(1)
    assert keyed.frames == 0 and not np.frombuffer(bytes(keyed.power), dtype=np.float64).any()
    assert rx.burst_spectra(0)["frames"].tolist() == [4, 2, 1] and rx.burst_spectra(2)["frames"].tolist() == [2, 2]
    with pytest.raises(ok.OokdError) as err:
        rx.burst_spectra(3)
    assert err.value.code == -1 and "capture 3 of 3" in str(err.value)
    with pytest.raises(ok.OokdError) as err:
        rx.burst_spectrum(3, 0)
    assert err.value.code == -1 and "burst 3 of 3" in str(err.value)
    rx.close()


def test_clean_table(ok):
    from tests.test_gpu_run_levels import _glitched
    iq = _glitched()
    n = iq.size // 2
    rx = ok.Receiver(None, None, max_samples=n, threshold=THR)
    rx.rx(iq)
    rx.clean_edges(0, 2000)
    t = rx.bursts(100, 500, 600, clean=True)[0]
    assert t["flags"] == 1 and t["num_samples"].tolist() == [4700, 1300]
    sp, want, worst = check(ok, rx, iq, 0, t, what="clean table")
    assert sp["flags"] == 1 and sp["frames"].tolist() == [4, 1]
    ms = rx.burst_spectra_kernel_ms
    # the raw form of the same run: another table, another result; each form keeps its own
    raw = rx.bursts(100, 500, 600)[0]
    assert raw["flags"] == 0 and raw["num_bursts"] != t["num_bursts"]
    with pytest.raises(ok.OokdError) as err:
        rx.keyed_spectrum(0)                                    # the raw table has no spectra yet
    assert err.value.code == -1 and "ookd_rx_burst_spectra first" in str(err.value)
    check(ok, rx, iq, 0, raw, what="raw table")
    rx.bursts(100, 500, 600, clean=True)
    assert rx.burst_spectra(0)["frames"].tolist() == [4, 1] and rx.burst_spectra_kernel_ms == ms
    rx.close()


# --------------------------------------------------------------------------------- 5. by-product rules ----

def test_by_product_rules(ok):
    n = 1 << 16
    runs = [(500, 3 * N, 100), (5001, 40 * N + 1, 300), (60000, 1500, 600)]
    cap = keyed_tones(n, runs, seed=6)
    iq = np.ascontiguousarray(cap).reshape(-1)
    rx = ok.Receiver(None, None, max_samples=n, threshold=THR)
    rx.rx(iq)
    assert rx.burst_spectra_kernel_ms == 0.0
    before = (rx.edges(0), rx.stats(), rx.bits(0))
    # no table yet
    with pytest.raises(ok.OokdError) as err:
        rx.burst_spectra(0)
    assert err.value.code == -1 and "ookd_rx_bursts first" in str(err.value)
    t = rx.bursts(0, 0, 0)[0]
    with pytest.raises(ok.OokdError) as err:
        rx.burst_spectrum(0)
    assert err.value.code == -1 and "ookd_rx_burst_spectra first" in str(err.value)
    first = rx.burst_spectra(0)
    ms = rx.burst_spectra_kernel_ms
    assert ms > 0.0 and first["frames"].tolist() == [3, 40, 1] and 0.0 < first["reduce_kernel_ms"] < ms
    keyed = bytes(rx.keyed_spectrum(0).power)
    one = rx.burst_spectrum(1)
    assert rx.burst_spectra_kernel_ms == ms                     # the single burst's pass is not the summaries'
    rx.bursts(0, 0, 0)                                          # the same table again
    again = rx.burst_spectra(0)
    assert rx.burst_spectra_kernel_ms == ms                     # the same float: no second pass was timed
    for k in FIELDS:
        assert again[k].tobytes() == first[k].tobytes()
    assert bytes(rx.keyed_spectrum(0).power) == keyed and rx.burst_spectrum(1).tobytes() == one.tobytes()
    # another span is another result, and bitwise the same when it is made a second time
    other = rx.burst_spectra(0, 64)
    assert other["span_frames"] == 64 and other["spans"] == 1 and first["spans"] == 2
    back = rx.burst_spectra(0, 32)
    for k in FIELDS:
        assert back[k].tobytes() == first[k].tobytes()
    assert bytes(rx.keyed_spectrum(0).power) == keyed and rx.burst_spectrum(1).tobytes() == one.tobytes()
    # new margins: a new table, and the old spectra are not its
    t2 = rx.bursts(10, 20, 30)[0]
    with pytest.raises(ok.OokdError) as err:
        rx.keyed_spectrum(0)
    assert err.value.code == -1
    check(ok, rx, cap, 0, t2, what="new margins")
    after = (rx.edges(0), rx.stats(), rx.bits(0))
    assert after[0].tolist() == before[0].tolist() and after[1] == before[1] and np.array_equal(after[2], before[2])
    # a new run: nothing of the last one holds, and a run nobody asks about costs nothing
    rx.rx(iq)
    assert rx.burst_spectra_kernel_ms == 0.0
    for call in (lambda: rx.burst_spectra(0), lambda: rx.keyed_spectrum(0), lambda: rx.burst_spectrum(0)):
        with pytest.raises(ok.OokdError) as err:
            call()
        assert err.value.code == -1
    rx.close()


def test_refusals(ok, vectors):
    import torch
    from tests.pulse_contract import golden_iq
    n = 1 << 14
    cap = keyed_tones(n, [(100, 3000, 100), (8000, 2000, 200)], seed=7)
    iq = np.ascontiguousarray(cap).reshape(-1)
    rx = ok.Receiver(None, None, max_samples=n, threshold=THR)
    with pytest.raises(ok.OokdError) as err:                    # no run yet
        rx.burst_spectra(0)
    assert err.value.code == -1 and "no finished run" in str(err.value)
    dev_t = torch.from_numpy(iq).cuda()
    rx.submit_device(dev_t.data_ptr(), n)                       # a run in flight
    with pytest.raises(ok.OokdError) as err:
        rx.burst_spectra(0)
    assert err.value.code == -1 and "ookd_rx_wait first" in str(err.value)
    rx.wait()
    rx.shard_begin(dev_t.data_ptr(), n, None, True, None)       # a shard run
    with pytest.raises(ok.OokdError) as err:
        rx.burst_spectra(0)
    assert err.value.code == -1 and "shard" in str(err.value)
    rx.rx(iq)                                                   # a whole run on the same context is answered again
    rx.bursts(0, 0, 0)
    assert rx.burst_spectra(0)["frames"].tolist() == [2, 1]
    rx.close()
    # an edge list that overflowed
    busy = np.zeros(2 * n, dtype=np.int16)
    busy[20::12] = 1000                                         # a pulse of one sample in every six
    rx = ok.Receiver(None, None, max_samples=n, threshold=THR, edge_capacity=256)
    with pytest.raises(ok.OokdError) as err:
        rx.rx(busy)
    assert err.value.code == -5
    with pytest.raises(ok.OokdError) as err:
        rx.burst_spectra(0)
    assert err.value.code == -5 and "overflow" in str(err.value)
    assert rx.burst_spectra_kernel_ms == 0.0
    rx.close()
    # a pipelined run (needs a state machine behind the front end)
    g = vectors["G1"]
    giq = golden_iq(vectors, "G1")
    f = ok.Filter.load(golden_path("filters", g["filter"]))
    d = ok.Device.load(golden_path("devices", g["device"]), RATE // f.total_decimation)
    rx = ok.Receiver(f, d, max_samples=giq.size // 2, pipeline_chunk_samples=4 * SPB)
    res = rx.rx(giq)
    assert res.stats["pipeline_chunks"] >= 2
    with pytest.raises(ok.OokdError) as err:
        rx.burst_spectra(0)
    assert err.value.code == -1 and "pipelined" in str(err.value)
    rx.close()


# ------------------------------------------------------------------------------------ 6. demonstration ----

DEMO_THR = 0.57
TIGHT, DEVICE_MARGINS = (600, 600, 1200), (600, 54000, 54600)
SILENCE, GAP = 1 << 20, 1 << 16


@pytest.fixture(scope="module")
def demo():
    """2^20 silent samples, G1 moved to +600 kHz, silence, G2 moved to -900 kHz, silence, at nominal level, with the
    spectrum tests' DC term and +-40 LSB of noise -> (capture, [(name, first sample, golden)], n)"""
    g1, _ = golden_capture("G1")
    g2, _ = golden_capture("G2")
    quiet = lambda count: np.zeros(2 * count, np.int16)
    parts = [quiet(SILENCE), moved(g1, 600e3 / RATE), quiet(GAP), moved(g2, -900e3 / RATE), quiet(GAP)]
    at1 = SILENCE
    at2 = at1 + g1.size // 2 + GAP
    iq = moved(np.concatenate(parts), 0.0, DC, NOISE, seed=21)
    return iq, [("G1", at1, g1), ("G2", at2, g2)], iq.size // 2


def test_demonstration(ok, oracle, demo, record_property):
    iq, stretches, n = demo
    rx = ok.Receiver(None, None, max_samples=n, threshold=DEMO_THR)
    rx.rx(iq)
    print("edges", rx.edges(0).size)
    # tight margins: about one burst per pulse train
    t = rx.bursts(*TIGHT)[0]
    sp, want, worst = check(ok, rx, iq, 0, t, what="demonstration, tight margins", every=7)
    record_property("worst_over_bound", worst)
    nb = t["num_bursts"]
    assert nb > 100 and (sp["frames"] >= 1).all()
    share = sp["peak_power"] / (sp["total_power"] - sp["dc_power"])
    print("bursts", nb, "share", share.min(), share.max())
    assert (share >= ok.BURST_MIN_SHARE).all()                  # every burst qualifies at the default share
    carriers, of = ok.suggest_burst_carriers(sp)
    want_c, want_of = py_suggest_burst_carriers(sp)
    assert [(c.bin, c.bursts, c.frames, c.power) for c in carriers] == want_c and of.tolist() == want_of
    assert sorted(c.bin for c in carriers) == [-307, 205]
    index = {c.bin: k for k, c in enumerate(carriers)}
    first = t["first_sample"].astype(np.int64)
    (_, at1, g1), (_, at2, g2) = stretches
    in1 = (first >= at1 - 1000) & (first < at1 + g1.size // 2)
    in2 = (first >= at2 - 1000) & (first < at2 + g2.size // 2)
    assert (in1 | in2).all() and in1.any() and in2.any()
    assert (of[in1] == index[205]).all() and (of[in2] == index[-307]).all()
    print("bursts at +205:", int(in1.sum()), "at -307:", int(in2.sum()))
    # the device's margins: one burst per transmitter
    t = rx.bursts(*DEVICE_MARGINS)[0]
    sp, want, worst = check(ok, rx, iq, 0, t, what="demonstration, device margins")
    assert t["num_bursts"] == 2 and sp["peak_bin"].tolist() == [205, N - 307]
    carriers, of = ok.suggest_burst_carriers(sp)
    assert sorted(c.bin for c in carriers) == [-307, 205] and sorted(of.tolist()) == [0, 1]
    assert [c.bursts for c in carriers] == [1, 1]
    rx.close()
    # those carriers decode: each golden's own device finds its messages where the unmoved golden has them
    nus = [c.nu for c in sorted(carriers, key=lambda c: -c.bin)]            # +205 first
    f = ok.Filter.load(golden_path("filters", "fs32_fs4"))
    of_ = oracle.load_filter_json(golden_path("filters", "fs32_fs4"))
    for k, (name, at, g) in enumerate(stretches):
        _, entry = golden_capture(name)
        d = ok.Device.load(golden_path("devices", entry["device"]), RATE)
        od = oracle.load_device_json(golden_path("devices", entry["device"]), RATE)[0]
        base = np.zeros(2 * n, np.int16)
        base[2 * at:2 * at + g.size] = g
        expect = oracle.rx(base, of_, THR, od, SPB)
        assert len(expect.msg_samples) == len(entry["survey"]["msg_samples"])
        crx = ok.Receiver(f, d, max_samples=n, carriers=nus)
        got = crx.rx(iq).for_capture(k)
        assert list(got.msg_samples) == list(expect.msg_samples), name
        assert (got.payloads == expect.payloads).all(), name
        crx.close()


def test_carrier_context_reads_the_one_capture(ok, demo):
    iq, stretches, n = demo
    f = ok.Filter.load(golden_path("filters", "fs32_fs4"))
    rx = ok.Receiver(f, None, max_samples=n, carriers=[205 / N, -307 / N])
    rx.rx(iq)
    tables = rx.bursts(*DEVICE_MARGINS)
    assert len(tables) == 2
    for k, (want_bin, (name, at, g)) in enumerate(zip((205, N - 307), stretches)):
        sp, want, worst = check(ok, rx, iq, k, tables[k], what="carrier %d" % k)
        # (the other transmitter's keying splatters into this list too: the burst that holds this one's first message)
        msg = at + golden_capture(name)[1]["survey"]["msg_samples"][0]
        first = tables[k]["first_sample"].astype(np.int64)
        own = np.nonzero((first <= msg) & (msg < first + tables[k]["num_samples"].astype(np.int64)))[0]
        assert own.size == 1 and sp["frames"][own[0]] > 100 and sp["peak_bin"][own[0]] == want_bin, (k, own)
    rx.close()


# ------------------------------------------------------------------------------------------ 7. example ----

def test_c_example_burst_carriers(ok, demo, tmp_path):
    """examples/ookd_rx.c --bursts F --burst-carriers on the demonstration's capture: the two carriers and a line per
    burst on stderr; stdout, the cut and its index are what they are without the option"""
    from tests.test_host import _build_c_example
    exe = _build_c_example(tmp_path)
    iq, stretches, n = demo
    cap = tmp_path / "demo.sc16q11"
    iq.tofile(str(cap))
    tail = [str(cap), golden_path("devices", "p3l-nexa2012"), "none", str(RATE), "csv"]
    us = [str(x * 1000000 // RATE) for x in DEVICE_MARGINS]
    opts = ["--threshold", str(DEMO_THR), "--burst-pre-us", us[0], "--burst-post-us", us[1], "--burst-gap-us", us[2]]
    plain = subprocess.run([exe, "--bursts", str(tmp_path / "a.sc16q11")] + opts + tail, capture_output=True, text=True, timeout=120)
    both = subprocess.run([exe, "--bursts", str(tmp_path / "b.sc16q11"), "--burst-carriers"] + opts + tail, capture_output=True,
                          text=True, timeout=120)
    assert plain.returncode == 0 and both.returncode == 0, (plain.stderr, both.stderr)
    print(both.stderr)
    fields = lambda text: [ln.split(",", 1)[1:] for ln in text.split("\n")]         # (the first is the wall clock)
    assert fields(both.stdout) == fields(plain.stdout)
    assert (tmp_path / "a.sc16q11").read_bytes() == (tmp_path / "b.sc16q11").read_bytes()
    assert (tmp_path / "a.sc16q11.idx").read_text() == (tmp_path / "b.sc16q11.idx").read_text()
    assert "burst carrier" not in plain.stderr
    lines = both.stderr.split("\n")
    found = sorted(ln.split(": ", 1)[1] for ln in lines if ln.startswith("burst carrier "))
    assert len(found) == 2 and found[0].startswith("-899414 Hz, 1 bursts, ") and found[1].startswith("600586 Hz, 1 bursts, ")
    idx = [ln.split() for ln in (tmp_path / "b.sc16q11.idx").read_text().strip().split("\n")]
    per = [ln.split() for ln in lines if ln.startswith("burst ") and not ln.startswith("burst carrier") and not ln.startswith("burst spectra")]
    assert [p[1:3] for p in per] == [i[0:2] for i in idx] and [p[3] for p in per] == ["600586", "-899414"]
    assert all(0.5 < float(p[4]) < 0.6 for p in per)
    # the option alone is refused
    alone = subprocess.run([exe, "--burst-carriers"] + tail, capture_output=True, text=True, timeout=120)
    assert alone.returncode != 0 and "--burst-carriers needs --bursts" in alone.stderr
