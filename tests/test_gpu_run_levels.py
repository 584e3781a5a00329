"""The pulse levels on the GPU (ookd_rx_run_levels; run_levels_kernel in run_levels.hip).  A peak is the maximum of
float bit patterns, exact and independent of any order, so every comparison is equality of uint32 patterns against the
numpy restatement of the contract (tests/run_levels_contract.py) over `rx.edges(c)` and the reference's power of the
capture zero padded to whole buffers."""
import os
import subprocess

import numpy as np
import pytest

from tests.helpers import golden_path
from tests.run_levels_contract import (RATE, SPB, THR, assert_same_bits, message_levels_of, nominal_power, padded,
                                       peaks_of, runs_of, tiles_filtered_of, two_level_capture)
from tests.test_survey_host import np_hist, oracle_power
from tests.tuned_contract import golden_capture, lib_stages, moved
from tests.tuned_survey_contract import contract_power

pytestmark = pytest.mark.gpu

ON = 2047
BLOCK = 4096
LENGTHS = (100003, 4097, 1025, 31, 1, 0)
# an isolated pulse (input samples, amplitude) that is on for exactly one output of the shape at threshold 0.1
ONE_PULSE = {"none": (1, ON), "fs32_fs4": (2, 412), "fs128_fs16_dec4": (2, 1650), "three": (6, 1825)}
# what the edge list of the 100003-sample capture has to hold, by shape: output 0 is below the threshold behind the
# two golden filters' first taps, and the three-stage filter leaves 3549 outputs -- less than one block
EVERYTHING = {"one", "at0", "pad", "tile", "block", "span3", "block_on", "block_off"}
WANT = {"none": EVERYTHING, "fs32_fs4": EVERYTHING - {"at0"}, "fs128_fs16_dec4": EVERYTHING - {"at0"},
        "three": {"one", "at0", "pad", "tile"}}


@pytest.fixture(scope="module")
def ok():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from ookiedokie_amd import build as okbuild
    okbuild.build()
    import ookiedokie_amd as okm
    okm.lib()
    return okm


def three_stages():
    def win(T):
        h = np.hanning(T + 2)[1:-1]
        return (h / h.sum()).astype(np.float32)
    return [(3, win(7)), (2, win(5)), (5, win(11))]


def shape_filters(ok, oracle, shape):
    """(library filter, oracle filter, total decimation) of a shape"""
    if shape == "none":
        return None, None, 1
    if shape == "three":
        st = three_stages()
        return ok.Filter.from_stages(st), oracle.make_fir(st), 30
    of = oracle.load_filter_json(golden_path("filters", shape))
    return ok.Filter.load(golden_path("filters", shape)), of, of.total_decimation


def designed(n, D, one, on=ON):
    """n samples laid out in outputs (x D input samples): a run from output 0, the one-output pulse, runs across a
    tile and a block boundary, one over more than four tiles, one that covers block 3 whole (block 5 is empty and
    off), a long silence, and a last run up to the capture's end -- which falls in the padding.  What does not fit in
    front of the last run is left out."""
    i = np.zeros(n, dtype=np.int16)
    if n <= 600:
        i[n // 3:] = on
    else:
        for a, f in ((0, 40), (1000, 1100), (4000, 4200), (5000, 9500), (12000, 20000)):
            if f * D < n - 600:
                i[a * D:f * D] = on
        if (100 + 8) * D < n - 600:
            i[100 * D:100 * D + one[0]] = one[1]
        i[n - 500:] = on
    iq = np.zeros(2 * n, dtype=np.int16)
    iq[0::2] = i
    return iq


def properties(edges, n_out, tile, n, D):
    runs = runs_of(edges, n_out)
    e = [int(x) for x in edges]
    out = set()
    if any(f - a == 1 for a, f in runs):
        out.add("one")
    if e and e[0] == 0:
        out.add("at0")
    if e and len(e) % 2 == 0 and e[-1] * D >= n and n % SPB:
        out.add("pad")
    if any(a // tile != (f - 1) // tile for a, f in runs):
        out.add("tile")
    if any(a // BLOCK != (f - 1) // BLOCK for a, f in runs):
        out.add("block")
    if any(f - a > 3 * tile for a, f in runs):
        out.add("span3")
    for b in range(n_out // BLOCK):
        if not any(b * BLOCK <= x < (b + 1) * BLOCK for x in e):
            out.add("block_on" if sum(x < b * BLOCK for x in e) % 2 else "block_off")
    return out


def check(rx, capture, power, clean=False, what=""):
    """one capture's answer against the restatement over its own edge list; -> (the answer, the edges)"""
    n_out = rx.stats()["decimated_samples"]
    e = rx.edges(capture, clean)
    lv = rx.run_levels(capture, clean)
    assert power.size == n_out, (what, power.size, n_out)
    want = peaks_of(power, e, n_out)
    assert lv["peaks"].dtype == np.float32
    assert_same_bits(lv["peaks"], want, what)
    assert lv["hist"].dtype == np.uint64 and lv["hist"].tolist() == np_hist(want).tolist(), what
    assert lv["num_runs"] == (e.size + 1) // 2 == lv["peaks"].size, what
    tile = lv["tile_outputs"]
    assert tile >= 1 and tile & (tile - 1) == 0 and tile <= 1024, what
    assert lv["tiles_total"] == -(-n_out // tile), what
    assert lv["tiles_filtered"] == tiles_filtered_of(e, n_out, tile), what
    return lv, e


# ----------------------------------------------------------------- 1. peaks against the restatement ----

@pytest.mark.parametrize("shape", ["none", "fs32_fs4", "fs128_fs16_dec4", "three"])
def test_peaks_shapes_and_lengths(ok, oracle, shape):
    f, of, D = shape_filters(ok, oracle, shape)
    rx = ok.Receiver(f, None, max_samples=max(LENGTHS), threshold=THR)
    assert rx.levels_kernel_ms == 0.0
    for n in LENGTHS:
        iq = designed(n, D, ONE_PULSE[shape])
        rx.rx(iq)
        assert rx.levels_kernel_ms == 0.0                       # nobody has asked about this run yet
        power = oracle_power(oracle, of, padded(iq))
        lv, e = check(rx, 0, power, what="%s n=%d" % (shape, n))
        n_out = rx.stats()["decimated_samples"]
        assert n_out == -(-n // SPB) * SPB // D
        if n == 0:
            assert lv["num_runs"] == 0 and lv["tiles_total"] == 0 and rx.levels_kernel_ms == 0.0
            continue
        assert rx.levels_kernel_ms > 0.0
        if shape in ("none", "fs32_fs4"):
            assert lv["num_runs"] >= 1, (shape, n)
        if n == LENGTHS[0]:
            have = properties(e, n_out, lv["tile_outputs"], n, D)
            assert WANT[shape] <= have, (shape, sorted(WANT[shape] - have), e.tolist())
            assert 0 < lv["tiles_filtered"] < lv["tiles_total"], (shape, lv["tiles_filtered"], lv["tiles_total"])
    rx.close()


THREE_LONG = 30 * 26000 + 7     # the three-stage filter's own length: 26214 outputs, six whole blocks


def test_three_stages_over_whole_blocks(ok, oracle):
    """the designed capture through decimations 3, 2, 5 at a length that leaves whole blocks: every property at once,
    the block without an edge that starts on among them"""
    f, of, D = shape_filters(ok, oracle, "three")
    n = THREE_LONG
    rx = ok.Receiver(f, None, max_samples=n, threshold=THR)
    iq = designed(n, D, ONE_PULSE["three"])
    rx.rx(iq)
    lv, e = check(rx, 0, oracle_power(oracle, of, padded(iq)), what="three n=%d" % n)
    n_out = rx.stats()["decimated_samples"]
    assert n_out == -(-n // SPB) * SPB // D and n_out >= 6 * BLOCK
    have = properties(e, n_out, lv["tile_outputs"], n, D)
    assert EVERYTHING <= have, (sorted(EVERYTHING - have), e.tolist())
    assert 0 < lv["tiles_filtered"] < lv["tiles_total"]
    rx.close()


@pytest.mark.parametrize("fmt", ["cs8", "cu8"])
@pytest.mark.parametrize("shape", ["none", "fs32_fs4", "fs128_fs16_dec4", "three"])
def test_8bit_captures_equal_the_widened_capture(ok, oracle, shape, fmt):
    f, of, D = shape_filters(ok, oracle, shape)
    for n in (100003, 1025):
        v = (designed(n, D, ONE_PULSE[shape]) >> 4).astype(np.int16)                 # on = 127
        raw = v.astype(np.int8) if fmt == "cs8" else (v + 128).astype(np.uint8)
        wide = (v * 16).astype(np.int16)
        rx8 = ok.Receiver(f, None, max_samples=n, threshold=THR, sample_format=fmt)
        rx8.rx(raw)
        power = oracle_power(oracle, of, padded(wide))
        lv8, e8 = check(rx8, 0, power, what="%s %s n=%d" % (shape, fmt, n))
        rx16 = ok.Receiver(f, None, max_samples=n, threshold=THR)
        rx16.rx(wide)
        lv16, e16 = check(rx16, 0, power)
        assert e8.tolist() == e16.tolist() and e8.size >= 2
        assert_same_bits(lv8["peaks"], lv16["peaks"])
        for key in ("num_runs", "tiles_total", "tiles_filtered", "tile_outputs"):
            assert lv8[key] == lv16[key], key
        assert lv8["hist"].tolist() == lv16["hist"].tolist()
        rx8.close()
        rx16.close()


@pytest.mark.parametrize("shape", ["none", "fs32_fs4"])
def test_no_edge_and_on_throughout(ok, oracle, shape):
    f, of, D = shape_filters(ok, oracle, shape)
    n = 3 * SPB
    rx = ok.Receiver(f, None, max_samples=n, threshold=THR)
    quiet = np.zeros(2 * n, dtype=np.int16)
    rx.rx(quiet)
    lv, e = check(rx, 0, oracle_power(oracle, of, quiet), what="quiet")
    assert e.size == 0 and lv["num_runs"] == 0 and lv["tiles_filtered"] == 0 and lv["tiles_total"] > 0
    assert not lv["hist"].any()
    on = np.zeros(2 * n, dtype=np.int16)
    on[0::2] = ON
    rx.rx(on)
    lv, e = check(rx, 0, oracle_power(oracle, of, on), what="on throughout")
    assert e.size == 1 and lv["num_runs"] == 1 and lv["tiles_filtered"] == lv["tiles_total"] == n // lv["tile_outputs"]
    rx.close()


# ----------------------------------------------------------------------------- 2. tuned contexts ----

def _two_carriers():
    nu1, nu2 = 600e3 / RATE, -900e3 / RATE
    g1, _ = golden_capture("G1")
    g2, _ = golden_capture("G2")
    ext = np.zeros_like(g1)
    ext[:g2.size] = g2
    # (both transmitters at half level: tests/test_gpu_pulses.py, test_carrier_histograms_are_the_tuned_contexts)
    z = moved(g1, nu1, scale=0.5).astype(np.int32) + moved(ext, nu2, 400.0 * (1 + 0.5j), 40, seed=11, scale=0.5).astype(np.int32)
    return np.clip(z, -32768, 32767).astype(np.int16), [(nu1, 0.1), (nu2, 0.12)]


@pytest.mark.parametrize("filt,fir2", [("fs32_fs4", False), ("fs128_fs16_dec4", False), ("fs128_fs16_dec4", True)],
                         ids=["fs32_fs4", "fs128-generic", "fs128-tuned_fir2"])
def test_tuned_and_carrier_contexts(ok, filt, fir2):
    iq, carriers = _two_carriers()
    n = iq.size // 2
    f = ok.Filter.load(golden_path("filters", filt))
    rx = ok.Receiver(f, None, max_samples=n, carriers=[carriers[0][0], carriers[1]], threshold=carriers[0][1], tuned_fir2=fir2)
    rx.rx(iq)
    for k, (nu, thr) in enumerate(carriers):
        power = contract_power(padded(iq), lib_stages(f, nu))
        lv, e = check(rx, k, power, what="carrier %d" % k)
        one = ok.Receiver(f, None, max_samples=n, threshold=thr, tune=nu, tuned_fir2=fir2)
        one.rx(iq)
        lv1, e1 = check(one, 0, power, what="tuned to carrier %d" % k)
        assert e1.tolist() == e.tolist() and e.size > 100
        if filt == "fs32_fs4":
            assert e.size == (228, 136)[k]
        assert_same_bits(lv1["peaks"], lv["peaks"])
        assert lv1["hist"].tolist() == lv["hist"].tolist() and lv1["tiles_filtered"] == lv["tiles_filtered"]
        one.close()
    with pytest.raises(ok.OokdError) as err:
        rx.run_levels(2)
    assert err.value.code == -1
    rx.close()


def test_message_levels_in_a_carrier_context(ok):
    """G1 at +600 kHz at half level and G1 again, 77000 samples later, at -900 kHz at 0.3 of nominal: a carrier context
    with the device decodes three messages on carrier 0 and two on carrier 1 (the reference does, on the contract's
    bits), and every message's level comes from its own carrier's list"""
    nu1, nu2 = 600e3 / RATE, -900e3 / RATE
    g1, meta = golden_capture("G1")
    late = np.zeros_like(g1)
    late[2 * 77000:] = g1[:-2 * 77000]
    z = moved(g1, nu1, scale=0.5).astype(np.int32) + moved(late, nu2, scale=0.3).astype(np.int32)
    iq = np.clip(z, -32768, 32767).astype(np.int16)
    n = iq.size // 2
    f = ok.Filter.load(golden_path("filters", "fs32_fs4"))
    d = ok.Device.load(golden_path("devices", meta["device"]), RATE // f.total_decimation)
    rx = ok.Receiver(f, d, max_samples=n, carriers=[nu1, nu2], threshold=THR)
    res = rx.rx(iq)
    assert sorted(res.captures.tolist()) == [0, 0, 0, 1, 1]
    assert res.stats["num_errors"] == 0
    levels = rx.message_levels(res)
    assert levels.dtype == np.float32 and levels.size == 5
    for k, (nu, scale) in enumerate(((nu1, 0.5), (nu2, 0.3))):
        lv, e = check(rx, k, contract_power(padded(iq), lib_stages(f, nu)), what="carrier %d" % k)
        m = res.captures == k
        want = message_levels_of(e, lv["peaks"], res.msg_samples[m], d.num_bits + 2)
        assert levels[m].tolist() == want.tolist(), k
        # within 1.5 of the own transmitter's nominal on power, as on the reference; the other's is 2.8 times away
        ratio = levels[m].astype(np.float64) / nominal_power(scale)
        assert (ratio > 1 / 1.5).all() and (ratio < 1.5).all(), (k, ratio)
    rx.close()


# ---------------------------------------------------------------------------------- 3. batched run ----

def _random_runs(n, rng, lo=3, hi=400):
    i = np.zeros(n, dtype=np.int16)
    pos = int(rng.integers(0, 50))
    while pos < n:
        d = int(rng.integers(lo, hi))
        i[pos:pos + d] = int(rng.integers(600, 2048))
        pos += d + int(rng.integers(lo, 4 * hi))
    iq = np.zeros(2 * n, dtype=np.int16)
    iq[0::2] = i
    return iq


def test_batch_with_loud_gaps_then_a_shorter_run(ok, oracle):
    import torch
    f, of, D = shape_filters(ok, oracle, "fs32_fs4")
    rng = np.random.default_rng(31)
    caps, n, stride = 5, 20001, 24000
    host = np.zeros((caps, 2 * stride), dtype=np.int16)
    host[:, 0::2] = 30000                                       # the gaps are loud
    iqs = [_random_runs(n, rng) for _ in range(caps)]
    iqs[2][:] = 0                                               # one capture without an edge
    for c in range(caps):
        host[c, :2 * n] = iqs[c]
    rx = ok.Receiver(f, None, max_samples=n, max_captures=caps, threshold=THR)
    dev_t = torch.from_numpy(host).cuda()
    rx.rx_device(dev_t.data_ptr(), n, num_captures=caps, stride=stride)
    assert rx.levels_kernel_ms == 0.0
    runs = []
    for c in (3, 0, 1, 2, 4):
        lv, e = check(rx, c, oracle_power(oracle, of, padded(iqs[c])), what="capture %d" % c)
        runs.append(lv["num_runs"])
        if c == 3:
            ms = rx.levels_kernel_ms
            assert ms > 0.0
        assert rx.levels_kernel_ms == ms                        # one pass answered all captures: nothing more was launched
    assert runs[3] == 0 and min(runs[:3] + runs[4:]) > 10
    with pytest.raises(ok.OokdError) as err:
        rx.run_levels(caps)
    assert err.value.code == -1
    # a shorter run with fewer captures on the same context: nothing of the first is left
    m = 9000
    rx.rx_device(dev_t.data_ptr(), m, num_captures=2, stride=stride)
    assert rx.levels_kernel_ms == 0.0
    for c in range(2):
        short = iqs[c][:2 * m]
        check(rx, c, oracle_power(oracle, of, padded(short)), what="short capture %d" % c)
    with pytest.raises(ok.OokdError):
        rx.run_levels(2)
    rx.close()


# ------------------------------------------------------------------------------------ 4. clean lists ----

def _glitched():
    """no filter: a pulse of two amplitudes with a dropout of 3 samples between them (the louder half second), some
    ordinary pulses, and a pulse with a dropout in its first half whose louder half comes first"""
    i = np.zeros(3 * SPB - 100, dtype=np.int16)
    i[1000:1050] = 1000
    i[1053:1100] = 2000
    i[3000:3400] = 1500
    i[5000:5040] = 1900
    i[5043:5100] = 900
    i[9000:9700] = 1200
    iq = np.zeros(2 * i.size, dtype=np.int16)
    iq[0::2] = i
    return iq


@pytest.mark.parametrize("debounced", [False, True], ids=["clean_edges", "debounced-context"])
def test_clean_list(ok, oracle, debounced):
    iq = _glitched()
    n = iq.size // 2
    power = oracle_power(oracle, None, padded(iq))
    rx = ok.Receiver(None, None, max_samples=n, threshold=THR, min_off=5 if debounced else 0)
    rx.rx(iq)
    if not debounced:
        with pytest.raises(ok.OokdError) as err:
            rx.run_levels(0, clean=True)
        assert err.value.code == -1 and "cleaned list" in str(err.value)
        assert rx.clean_edges(0, 5)[0]["deleted"] == [2, 0]
    raw, e_raw = check(rx, 0, power, what="raw list")
    lv, e = check(rx, 0, power, clean=True, what="cleaned list")
    assert e_raw.size == 12 and e.tolist() == [1000, 1100, 3000, 3400, 5000, 5100, 9000, 9700]
    s = np.float32(1.0 / 2048.0)
    amp = lambda a: (np.float32(a) * s) * (np.float32(a) * s)
    # the swallowed dropouts: each cleaned run reports the louder of its two halves
    assert lv["peaks"].tolist() == [amp(2000), amp(1500), amp(1900), amp(1200)]
    assert raw["peaks"].tolist() == [amp(1000), amp(2000), amp(1500), amp(1900), amp(900), amp(1200)]
    # other minimums on the same run: another cleaned list, and the answer is about that one
    ms = rx.levels_kernel_ms
    rx.clean_edges(0, 2000)
    lv2, e2 = check(rx, 0, power, clean=True, what="cleaned again")
    assert e2.tolist() == [1000, 5100, 9000, 9700] and lv2["num_runs"] == 2
    assert lv2["peaks"].tolist() == [amp(2000), amp(1200)]
    at = ok.RxResult(np.zeros(2, np.uint32), np.array([6000, 9500], np.uint64), np.zeros((2, 0), np.uint8), {})
    assert rx.message_levels(at, pulses=3, clean=True).tolist() == [amp(2000), amp(1200)]
    # ... and back: the first list's answer again, the raw list's pass untouched throughout
    rx.clean_edges(0, 5)
    lv3, e3 = check(rx, 0, power, clean=True, what="cleaned a third time")
    assert e3.tolist() == e.tolist() and lv3["peaks"].tolist() == lv["peaks"].tolist()
    assert rx.levels_kernel_ms == ms
    check(rx, 0, power, what="raw list afterwards")
    rx.close()


# -------------------------------------------------------------------------------------- 5. refusals ----

def test_refusals(ok, vectors):
    import torch
    from tests.pulse_contract import golden_iq
    n = 1 << 15
    i = np.zeros(n // 2, dtype=np.int16)
    i[10::6] = ON
    i[11::6] = ON
    i[12::6] = ON
    iq = np.zeros(n, dtype=np.int16)
    iq[0::2] = i
    # no run yet
    rx = ok.Receiver(None, None, max_samples=n, threshold=THR, edge_capacity=256)
    with pytest.raises(ok.OokdError) as e:
        rx.run_levels(0)
    assert e.value.code == -1 and "no finished run" in str(e.value)
    # an overflowed edge list
    with pytest.raises(ok.OokdError) as e:
        rx.rx(iq)
    assert e.value.code == -5
    with pytest.raises(ok.OokdError) as e:
        rx.run_levels(0)
    assert e.value.code == -5 and "overflow" in str(e.value)
    assert rx.levels_kernel_ms == 0.0
    rx.close()
    # a run in flight, a capture out of range, a shard run
    rx = ok.Receiver(None, None, max_samples=n, threshold=THR, edge_capacity=n)
    dev_t = torch.from_numpy(iq).cuda()
    rx.submit_device(dev_t.data_ptr(), iq.size // 2)
    with pytest.raises(ok.OokdError) as e:
        rx.run_levels(0)
    assert e.value.code == -1 and "ookd_rx_wait first" in str(e.value)
    rx.wait()
    assert rx.run_levels(0)["num_runs"] > 100
    with pytest.raises(ok.OokdError) as e:
        rx.run_levels(1)
    assert e.value.code == -1 and "capture 1 of 1" in str(e.value)
    rx.shard_begin(dev_t.data_ptr(), iq.size // 2, None, True, None)
    with pytest.raises(ok.OokdError) as e:
        rx.run_levels(0)
    assert e.value.code == -1 and "shard" in str(e.value)
    rx.rx(iq)                                                   # a whole run on the same context is answered again
    assert rx.run_levels(0)["num_runs"] > 100
    rx.close()
    # a pipelined run (needs a state machine behind the front end)
    g = vectors["G1"]
    giq = golden_iq(vectors, "G1")
    f = ok.Filter.load(golden_path("filters", g["filter"]))
    d = ok.Device.load(golden_path("devices", g["device"]), RATE // f.total_decimation)
    rx = ok.Receiver(f, d, max_samples=giq.size // 2, pipeline_chunk_samples=4 * SPB)
    res = rx.rx(giq)
    assert res.stats["pipeline_chunks"] >= 2
    with pytest.raises(ok.OokdError) as e:
        rx.run_levels(0)
    assert e.value.code == -1 and "pipelined" in str(e.value)
    rx.close()
    # a filter whose history the pass's LDS window cannot hold: the survey's refusal, at the first call
    long_taps = np.full(11000, 1.0 / 11000.0, dtype=np.float32)
    f = ok.Filter.from_stages([(1, long_taps)])
    with pytest.raises(ok.OokdError) as e:
        ok.Survey(f)
    assert "does not fit the kernel's LDS window" in str(e.value)
    rx = ok.Receiver(f, None, max_samples=SPB, threshold=THR)
    rx.rx(np.zeros(2 * SPB, dtype=np.int16))
    with pytest.raises(ok.OokdError) as e:
        rx.run_levels(0)
    assert e.value.code == -1 and "does not fit the kernel's LDS window" in str(e.value)
    assert rx.levels_kernel_ms == 0.0
    rx.close()


# ------------------------------------------------------------------------- 6. the two transmitters ----

@pytest.mark.parametrize("filt", ["fs32_fs4", "fs128_fs16_dec4"])
def test_two_transmitters_end_to_end(ok, oracle, vectors, filt):
    g, iq, half = two_level_capture(vectors)
    f = ok.Filter.load(golden_path("filters", filt))
    dec = f.total_decimation
    d = ok.Device.load(golden_path("devices", g["device"]), RATE // dec)
    rx = ok.Receiver(f, d, max_samples=iq.size // 2, threshold=THR, pipeline=False)
    res = rx.rx(iq)
    assert len(res.msg_samples) == 6 and res.stats["num_errors"] == 0
    of = oracle.load_filter_json(golden_path("filters", filt))
    lv, e = check(rx, 0, oracle_power(oracle, of, padded(iq)), what=filt)
    assert lv["num_runs"] == 228
    levels = rx.message_levels(res)
    assert levels.dtype == np.float32
    assert levels.tolist() == message_levels_of(e, lv["peaks"], res.msg_samples, d.num_bits + 2).tolist()
    strong, weak = nominal_power(1.0), nominal_power(0.25)
    own = np.where(e[0::2] < half // dec, strong, weak)
    ratio = lv["peaks"].astype(np.float64) / own
    assert (ratio > 1 / 1.5).all() and (ratio < 1.5).all(), (ratio.min(), ratio.max())
    for m, x in enumerate(levels.astype(np.float64)):
        mine, other = (strong, weak) if m < 3 else (weak, strong)
        assert mine / 1.5 < x < mine * 1.5, (m, x)
        assert x >= 8 * other or x <= other / 8, (m, x)
    rx.close()


# ---------------------------------------------------------------------------------- 7. the example ----

def test_c_example_levels(ok, vectors, tmp_path):
    """examples/ookd_rx.c --levels: stdout is what it is without the option (but for the wall clock in the first
    column), and the levels on stderr are Python's to the printed digits"""
    from tests.test_host import _build_c_example
    exe = _build_c_example(tmp_path)
    g, iq, _ = two_level_capture(vectors)
    cap = tmp_path / "two.sc16q11"
    iq.tofile(str(cap))
    args = [str(cap), golden_path("devices", g["device"]), golden_path("filters", "fs32_fs4"), str(RATE), "csv"]
    plain = subprocess.run([exe] + args, capture_output=True, text=True, timeout=120)
    with_levels = subprocess.run([exe, "--levels"] + args, capture_output=True, text=True, timeout=120)
    assert plain.returncode == 0 and with_levels.returncode == 0, (plain.stderr, with_levels.stderr)
    fields = lambda text: [ln.split(",", 1)[1:] for ln in text.split("\n")]         # (the first is the wall clock)
    assert fields(with_levels.stdout) == fields(plain.stdout) and len(plain.stdout.strip().split("\n")) == 7
    assert "level" not in plain.stderr
    f = ok.Filter.load(golden_path("filters", "fs32_fs4"))
    d = ok.Device.load(golden_path("devices", g["device"]), RATE // f.total_decimation)
    rx = ok.Receiver(f, d, max_samples=iq.size // 2, threshold=THR)
    res = rx.rx(iq)
    levels = rx.message_levels(res)
    rx.close()
    want = ["level 0 %d %.2f" % (s, 10.0 * np.log10(np.float64(x))) for s, x in zip(res.msg_samples, levels)]
    got = [ln for ln in with_levels.stderr.split("\n") if ln.startswith("level ")]
    assert got == want and len(got) == 6
    # stderr without the level lines is the plain run's but for its timing figure
    rest = [ln for ln in with_levels.stderr.split("\n") if not ln.startswith("level ")]
    assert len(rest) == len(plain.stderr.split("\n"))


# ------------------------------------------------------------------------ 8. nothing else changes ----

def test_the_run_is_what_it_was(ok, vectors):
    from tests.pulse_contract import golden_iq
    g = vectors["G1"]
    iq = golden_iq(vectors, "G1", noise_seed=5)
    f = ok.Filter.load(golden_path("filters", g["filter"]))
    d = ok.Device.load(golden_path("devices", g["device"]), RATE // f.total_decimation)
    rx = ok.Receiver(f, d, max_samples=iq.size // 2, threshold=THR, pipeline=False)
    rx.rx(iq)
    before = (rx.result(), rx.edges(0), rx.pulse_hist(0), rx.stats(), rx.bits(0))
    lv = rx.run_levels(0)
    assert lv["num_runs"] == 114 and rx.levels_kernel_ms > 0.0
    after = (rx.result(), rx.edges(0), rx.pulse_hist(0), rx.stats(), rx.bits(0))
    assert len(before[0].msg_samples) == 3
    assert (after[0].msg_samples == before[0].msg_samples).all() and (after[0].payloads == before[0].payloads).all()
    assert (after[0].captures == before[0].captures).all() and after[0].stats == before[0].stats
    assert after[1].tolist() == before[1].tolist()
    for key in before[2]:
        assert np.array_equal(after[2][key], before[2][key]), key
    assert after[3] == before[3] and np.array_equal(after[4], before[4])
    rx.close()
