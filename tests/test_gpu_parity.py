"""Parity tests proper: the HIP path, called through the C ABI, against the
CPU oracle on the same inputs (bit-exact for bits / edges / messages /
payloads / error positions; FIR floats bit-exact in EXACT mode and within
1e-5 of full scale in the default fused mode -- tolerance stated below),
against the committed golden vectors, and -- at BASELINE.json sizes --
through size-independent properties."""
import ctypes as C
import json
import os

import contextlib
import math

import numpy as np
import pytest

from tests.helpers import edges_of, golden_path, iq_from_rle, stream_from_runs

pytestmark = pytest.mark.gpu

RATE = 3000000
# FIR float tolerance (BASELINE.json north_star: "within 1e-5 relative"),
# made well-defined as SURVEY.md hard part 2 prescribes:
#   |y - y_ref| <= 1e-5 * max(|y_ref|, sum|h| * max|x|)
FIR_RTOL = 1e-5


@pytest.fixture(scope="module")
def ok():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from ookiedokie_amd import build as okbuild
    okbuild.build()
    import ookiedokie_amd as okm
    okm.lib()
    return okm


def _flt(ok, name):
    return ok.Filter.load(golden_path("filters", name)) if name else None


def _ofir(oracle, name):
    return oracle.load_filter_json(golden_path("filters", name)) if name else None


def _dev(ok, name, rate=RATE):
    return ok.Device.load(golden_path("devices", name), rate)


def _odev(oracle, name, rate=RATE):
    return oracle.load_device_json(golden_path("devices", name), rate)[0]


@contextlib.contextmanager
def _sync_walk_forced(on=True):
    """Receivers created inside try the scan's walk from synchronising spans whatever the expected edge count
    (by default an edge list under 20 000 goes through the composing kernels)."""
    keys = ("OOKD_DEVELOPER", "OOKD_SYNC_MIN_EDGES")
    old = {k: os.environ.get(k) for k in keys}
    if on:
        os.environ["OOKD_DEVELOPER"] = "1"
        os.environ["OOKD_SYNC_MIN_EDGES"] = "0"
    try:
        yield
    finally:
        for k in keys:
            if old[k] is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = old[k]


def _form_for(ok, of, exact=False, valu=False):
    """the front-end kernel launch_front runs for a filter (the rules of kernels.hip front_form and front_plan.cpp
    plan_real_form; thresholds within [2^-50, 2^50] and taps near unit gain: the matrix cores never refuse)"""
    if of is None:
        return ok.FRONT_NO_FILTER
    n = [int(of.stage_taps(s).size) for s in range(of.num_stages)]
    d = [int(of.decimation[s]) for s in range(of.num_stages)]
    if d == [1] and -(-n[0] // 32) * 32 <= 256:
        return ok.FRONT_FIR1_VALU_EXACT if exact else ok.FRONT_FIR1_VALU if valu else ok.FRONT_FIR1_MFMA
    if d == [2, 2] and n[0] <= 16 and n[1] <= 32:
        return ok.FRONT_FIR2_VALU_EXACT if exact else ok.FRONT_FIR2_VALU if valu else ok.FRONT_FIR2_MFMA
    return ok.FRONT_GENERIC


def _compare(ok, oracle, iq, filt, devname, spb=8192, thr=0.1, exact=False, check_fir=False,
             segment_buffers=0, rate=RATE, expect_scan=True):
    """Runs the capture through every form of the state machine (scan of
    per-edge transition functions, with span tables and with per-span
    simulation; segment rounds) and checks each against the oracle."""
    f = _flt(ok, filt)
    of = _ofir(oracle, filt)
    dec = of.total_decimation if of else 1
    d = _dev(ok, devname, rate // dec)
    od = _odev(oracle, devname, rate // dec)
    n = iq.size // 2
    want = oracle.rx(iq, of, thr, od, spb, want_bits=True, want_fir=check_fir)
    got = None
    # state machine forms: scan with span tables, scan simulating every span, rounds; then the scan
    # again with the capture pipelined in small chunks (front end of chunk c+1 beside the state
    # machine of chunk c, state carried on the device) and with the packed-VALU form of the 1-stage
    # front end instead of the matrix-core one (the default wherever it applies); and the scan with its entry
    # states from composed block tables only (the default first tries the walk from synchronising spans)
    # (tables: None = the default -- composed for an edge list as short as a test's --, True = OOKD_RX_SCAN_TABLES,
    #  False = the walk from synchronising spans whatever the length)
    for fsm_rounds, scan_sims, chunk, valu, tables in (
            (False, False, 0, False, None), (False, True, 0, False, None), (True, False, 0, False, None),
            (False, False, 4 * spb, False, None), (False, False, 0, True, None), (False, False, 0, False, True),
            (False, False, 0, False, False), (False, False, 4 * spb, False, False)):
        with _sync_walk_forced(tables is False):
            rx = ok.Receiver(f, d, max_samples=max(n, 1), threshold=thr, samples_per_buffer=spb,
                             exact_fir=exact, keep_fir=check_fir, segment_buffers=segment_buffers,
                             fsm_rounds=fsm_rounds, quiet_skip=not fsm_rounds, scan_sims=scan_sims,
                             pipeline_chunk_samples=chunk, fir_valu=valu, scan_tables=bool(tables))
        got = rx.rx(iq)
        assert got.stats["decimated_samples"] == want.decimated
        assert got.stats["front_form"] == _form_for(ok, of, exact, valu)
        if tables and got.stats["fsm_path"] == 1:
            assert got.stats["scan_entry_form"] == 2
        if chunk and expect_scan and spb % 4096 == 0 and n >= 16 * spb and got.stats["fsm_fallback_reason"] == 0:
            assert got.stats["pipeline_chunks"] >= 2, "the capture was not pipelined"
        assert got.stats["num_edges"] == len(edges_of(want.bits))
        if want.decimated:
            assert got.stats["fsm_path"] == (2 if fsm_rounds else (1 if expect_scan else got.stats["fsm_path"]))
        bits = rx.bits()
        assert bits.size == want.bits.size
        diff = np.nonzero(bits != want.bits)[0]
        assert diff.size == 0, "first differing bit at %s" % diff[:5]
        assert list(rx.edges()) == list(edges_of(want.bits))
        assert list(got.msg_samples) == list(want.msg_samples), "fsm_rounds=%s" % fsm_rounds
        assert (got.payloads == want.payloads).all(), "fsm_rounds=%s" % fsm_rounds
        errs, nerr = rx.errors(len(want.err_samples) + 8)
        assert nerr == len(want.err_samples), "fsm_rounds=%s" % fsm_rounds
        assert list(errs) == list(want.err_samples), "fsm_rounds=%s" % fsm_rounds
        if check_fir and not fsm_rounds:
            y = rx.fir_output()
            if exact or of is None:
                assert (y.view(np.uint32) == want.fir.view(np.uint32)).all(), "FIR floats not bit-identical"
            else:
                # fused multiply-add kernels (bits are protected by the guard band)
                gain = 1.0
                for st in range(of.num_stages):
                    gain *= max(1.0, float(np.abs(of.stage_taps(st)).sum()))
                scale = gain * float(np.abs(iq).max()) / 2048.0
                tol = FIR_RTOL * np.maximum(np.abs(want.fir), scale)
                assert (np.abs(y - want.fir) <= tol).all()
        rx.close()
    return got, want


def _g1(vectors, noise_seed=None):
    g = vectors["G1"]
    iq = iq_from_rle(g["i_rle"], g["num_samples"])
    if noise_seed is not None:
        rng = np.random.default_rng(noise_seed)
        iq = (iq + rng.integers(-40, 41, size=iq.size)).astype(np.int16)
    return g, iq


# ----------------------------------------------------------------- golden ----

@pytest.mark.parametrize("exact", [False, True])
def test_g1_golden(ok, oracle, vectors, exact):
    g, iq = _g1(vectors)
    got, want = _compare(ok, oracle, iq, "fs32_fs4", "p3l-nexa2012", exact=exact, check_fir=True)
    s = g["survey"]
    assert list(got.msg_samples) == s["msg_samples"]
    assert all(got.payload_bits(i, 36) == s["payload_bits"] for i in range(3))
    assert got.stats["num_edges"] == s["num_edges"]


def test_g1_printed_text(ok, vectors):
    """End to end to the text the real binary printed for G1:
    three CSV records 0x27,0xd5,2,21.500,70.700,0x00 (plus the wall-clock
    "Decode Timestamp" column p3l-nexa2012 asks for)."""
    g, iq = _g1(vectors)
    f = _flt(ok, "fs32_fs4")
    d = _dev(ok, "p3l-nexa2012", RATE)
    rx = ok.Receiver(f, d, max_samples=iq.size // 2, threshold=0.1, samples_per_buffer=8192)
    res = rx.rx(iq)
    fmt = ok.Formatter(d)
    lines = fmt.print_messages(res, 8192, 1, ok.RX_FMT_CSV).split("\n")
    assert lines[0] == "Decode Timestamp,Preamble,Unknown-1,Channel,Temperature (C),Temperature (F),Unknown-2"
    assert [ln.split(",", 1)[1] for ln in lines[1:4]] == ["0x27,0xd5,2,21.500,70.700,0x00"] * 3
    assert lines[4:] == [""]
    pretty = ok.Formatter(d).print_messages(res, 8192, 1, ok.RX_FMT_PRETTY)
    assert pretty.count("     Temperature (C) : 21.500\n") == 3 and pretty.endswith("0x00\n\n")
    rx.close()


def test_c_host_example(ok, vectors, tmp_path):
    """The C99 host of examples/ookd_rx.c (gcc, header + .so only): backend
    handle -> HBM capture -> fused demod -> printed text, plus --rx-rec-dig."""
    import subprocess
    from tests.test_host import _build_c_example
    exe = _build_c_example(tmp_path)
    g, iq = _g1(vectors)
    cap = tmp_path / "g1.sc16q11"
    iq.tofile(str(cap))
    dig = tmp_path / "dig.csv"
    r = subprocess.run([exe, str(cap), golden_path("devices", "p3l-nexa2012"), golden_path("filters", "fs32_fs4"),
                        str(RATE), "csv", str(dig)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.split("\n")
    assert lines[0] == "Decode Timestamp,Preamble,Unknown-1,Channel,Temperature (C),Temperature (F),Unknown-2"
    assert [ln.split(",", 1)[1] for ln in lines[1:4]] == ["0x27,0xd5,2,21.500,70.700,0x00"] * 3
    rx = ok.Receiver(_flt(ok, "fs32_fs4"), None, max_samples=iq.size // 2)
    rx.rx(iq)
    assert dig.read_text() == rx.dig_text()
    rx.close()


@pytest.mark.parametrize("spb", [1000, 4096, 65536])
def test_g1_other_buffer_sizes(ok, oracle, vectors, spb):
    g, iq = _g1(vectors)
    got, _ = _compare(ok, oracle, iq, "fs32_fs4", "p3l-nexa2012", spb=spb)
    assert list(got.msg_samples) == g["survey"]["msg_samples"]


def test_g2_golden(ok, oracle, vectors):
    g = vectors["G2"]
    iq = iq_from_rle(g["i_rle"], g["num_samples"])
    got, _ = _compare(ok, oracle, iq, "fs32_fs4", "unknown-remote1", check_fir=True)
    assert list(got.msg_samples) == g["survey"]["msg_samples"]
    assert all(got.payload_bits(i, 32) == g["survey"]["payload_bits"] for i in range(2))


@pytest.mark.parametrize("spb", [1000, 4096, 8192, 65536])
def test_g3_error_drops_rest_of_buffer(ok, oracle, vectors, spb):
    g, iq = _g1(vectors)
    a, b, v = vectors["G3"]["glitch"]
    iq[2 * a:2 * b:2] = v
    got, want = _compare(ok, oracle, iq, "fs32_fs4", "p3l-nexa2012", spb=spb)
    assert len(got.msg_samples) == vectors["G3"]["survey_num_msgs"][str(spb)]


@pytest.mark.parametrize("thr", [0.02, 0.1, 0.5])
def test_quiet_shortcut_boundary(ok, oracle, thr):
    """Blocks of noise whose amplitude straddles the level below which a
    wavefront may skip the filter: bits must not depend on the shortcut."""
    of = _ofir(oracle, "fs32_fs4")
    S = float(np.abs(of.taps.astype(np.float64)).sum())
    lvl = thr * 0.999 / (np.sqrt(2.0) * S) * 2048.0      # in LSB
    rng = np.random.default_rng(77)
    blocks = []
    for i in range(600):
        amp = max(1, int(lvl * rng.choice([0.5, 0.9, 0.99, 1.0, 1.01, 1.1, 1.5, 3.0])))
        m = int(rng.integers(300, 3000))
        b = rng.integers(-amp, amp + 1, size=(m, 2)).astype(np.int16)
        if rng.random() < 0.3:
            b[:, 0] = amp            # constant: the filter's DC gain, not sum|h|, decides
            b[:, 1] = -amp
        blocks.append(b)
    iq = np.concatenate(blocks).reshape(-1)
    _compare(ok, oracle, iq, "fs32_fs4", "p3l-nexa2012", thr=thr)


# ----------------------------------------------------------------- recorders ----

def test_rx_rec_dig_text(ok, oracle, vectors, tmp_path):
    """--rx-rec-dig (ookiedokie.c:146-169): text identical to record_dig run
    over the oracle's bit stream; first edges as the real binary wrote them
    for G1."""
    g, iq = _g1(vectors)
    f = _flt(ok, "fs32_fs4")
    rx = ok.Receiver(f, None, max_samples=iq.size // 2, threshold=0.1, samples_per_buffer=8192)
    rx.rx(iq)
    want = oracle.rx(iq, _ofir(oracle, "fs32_fs4"), 0.1, None, 8192, want_bits=True)
    text = rx.dig_text()
    assert text == oracle.dig_text(want.bits, 8192)
    assert text.startswith("0, 0\n12013, 0\n12014, 1\n13516, 1\n13517, 0\n39613, 0\n39614, 1\n")
    assert text.count("\n") == 1 + 2 * 228
    p = tmp_path / "dig.csv"
    rx.record_dig(str(p))
    assert p.read_text() == text
    rx.close()
    # a capture that starts high: first line carries the level, no pair for sample 0
    iq2 = np.zeros(2 * 5000, dtype=np.int16)
    iq2[0:2 * 1200:2] = 1945
    iq2[2 * 3000:2 * 3100:2] = 1945
    rx = ok.Receiver(None, None, max_samples=5000, threshold=0.1, samples_per_buffer=1000)
    rx.rx(iq2)
    want = oracle.rx(iq2, None, 0.1, None, 1000, want_bits=True)
    assert rx.dig_text() == oracle.dig_text(want.bits, 1000) == (
        "0, 1\n1199, 1\n1200, 0\n2999, 0\n3000, 1\n3099, 1\n3100, 0\n")
    rx.rx(np.zeros(0, dtype=np.int16))
    assert rx.dig_text() == ""                 # no buffer, no first line
    rx.close()


@pytest.mark.parametrize("filt", ["fs32_fs4", "fs128_fs16_dec4"])
def test_rx_rec_post_filter_sc16q11(ok, oracle, vectors, tmp_path, filt):
    """--rx-rec (post-filter, ookiedokie.c:265-270): complexf_to_sc16q11 of the
    filter output, checked against the oracle's pack and the reference's own
    complexf.h through oracle/_ref."""
    g, iq = _g1(vectors, noise_seed=21)
    iq = iq[:2 * 300000]
    f = _flt(ok, filt)
    rx = ok.Receiver(f, None, max_samples=iq.size // 2, threshold=0.1, samples_per_buffer=8192,
                     exact_fir=True, keep_fir=True)
    rx.rx(iq)
    want = oracle.rx(iq, _ofir(oracle, filt), 0.1, None, 8192, want_fir=True)
    got = rx.fir_sc16q11()
    assert (got == oracle.pack(want.fir)).all()
    p = tmp_path / "post.sc16q11"
    rx.record_fir(str(p))
    assert (np.fromfile(str(p), dtype=np.int16) == got).all()
    rx.close()


# ----------------------------------------------- other filters / no filter ----

@pytest.mark.parametrize("exact", [False, True])
@pytest.mark.parametrize("filt", ["fs128_fs16_dec4", "unity16", "unity1", None])
def test_other_filters_noisy(ok, oracle, vectors, filt, exact):
    g, iq = _g1(vectors, noise_seed=11)
    _compare(ok, oracle, iq, filt, "p3l-nexa2012", check_fir=True, exact=exact)


def test_dec4_with_buffer_not_multiple_of_decimation(ok, oracle, vectors):
    g, iq = _g1(vectors, noise_seed=12)
    for spb in (1001, 4098, 8191):
        _compare(ok, oracle, iq[:2 * 600000], "fs128_fs16_dec4", "p3l-nexa2012", spb=spb)


def test_255_tap_filter(ok, oracle, vectors, tmp_path):
    # BASELINE config 3 shape: 255 real taps = hamming-windowed sinc, cutoff Fs/64
    n = np.arange(255) - 127
    h = np.sinc(n / 32.0) * np.hamming(255)
    h = (h / h.sum()).astype(np.float64)
    p = tmp_path / "sinc255.json"
    p.write_text(json.dumps({"filter": {"stages": [{"decimation": 1, "taps": list(h)}]}}))
    g = vectors["G2"]
    iq = iq_from_rle(g["i_rle"], g["num_samples"])
    rng = np.random.default_rng(2)
    iq = (iq + rng.integers(-40, 41, size=iq.size)).astype(np.int16)
    f = ok.Filter.load(str(p))
    of = oracle.load_filter_json(str(p))
    for exact in (False, True):
        d = _dev(ok, "unknown-remote1")
        od = _odev(oracle, "unknown-remote1")
        rx = ok.Receiver(f, d, max_samples=iq.size // 2, exact_fir=exact, keep_fir=True)
        got = rx.rx(iq)
        want = oracle.rx(iq, of, 0.1, od, 8192, want_bits=True, want_fir=True)
        assert (rx.bits() == want.bits).all()
        assert list(got.msg_samples) == list(want.msg_samples) and len(want.msg_samples) == 2
        assert (got.payloads == want.payloads).all()
        y = rx.fir_output()
        if exact:
            assert (y.view(np.uint32) == want.fir.view(np.uint32)).all()
        else:
            scale = float(np.abs(of.taps).sum()) * float(np.abs(iq).max()) / 2048.0
            assert (np.abs(y - want.fir) <= FIR_RTOL * np.maximum(np.abs(want.fir), scale)).all()


# ------------------------------------------------- dense edges / tile info ----

@pytest.mark.parametrize("filt", [None, "fs32_fs4", "fs128_fs16_dec4", "unity16"])
@pytest.mark.parametrize("n", [1000, 4096 + 1024, 3 * 4096 + 257, 70000])
def test_dense_random_levels(ok, oracle, filt, n):
    """Samples that cross the threshold at random, every few samples: the edge
    list (built from the per-tile change counts of the front-end kernels) must
    be the oracle's, whatever the position of tile / block / capture ends."""
    rng = np.random.default_rng(n + (0 if filt is None else len(filt)))
    # runs of 1..12 samples, alternately far below and far above the threshold
    runs = rng.integers(1, 13, size=2 * n)
    lvl = np.repeat(np.arange(runs.size) & 1, runs)[:n]
    iq = np.zeros(2 * n, dtype=np.int16)
    iq[0::2] = np.where(lvl == 1, 1500, 20) + rng.integers(-15, 16, size=n)
    iq[1::2] = rng.integers(-15, 16, size=n)
    f = _flt(ok, filt)
    of = _ofir(oracle, filt)
    for spb in (512, 8192):
        rx = ok.Receiver(f, None, max_samples=n, threshold=0.1, samples_per_buffer=spb, edge_capacity=n + 64)
        got = rx.rx(iq)
        want = oracle.rx(iq, of, 0.1, None, spb, want_bits=True)
        assert (rx.bits() == want.bits).all()
        assert list(rx.edges()) == list(edges_of(want.bits))
        assert got.stats["num_edges"] == len(edges_of(want.bits))
        assert rx.dig_text() == oracle.dig_text(want.bits, max(1, spb // (of.total_decimation if of else 1)))
        rx.close()


# ------------------------------------------ matrix-core form of the 1-stage front end ----

def _write_filter(tmp_path, taps, name):
    p = tmp_path / (name + ".json")
    p.write_text(json.dumps({"filter": {"stages": [{"decimation": 1, "taps": [float(t) for t in taps]}]}}))
    return str(p)


def _loud_capture(n, rng, wide):
    """every window loud, the filtered magnitude crossing the threshold all the time; `wide`: samples over
    the whole int16 range (the matrix-core form splits those into two fp16 pieces)"""
    t = np.arange(n)
    env = 205.0 * (1.0 + 0.8 * np.sin(2 * np.pi * t / 3000.0)) * (12.0 if wide else 1.0)
    ph = rng.uniform(0, 2 * np.pi)
    amp = 2500 if wide else 250
    i = env * np.cos(ph) + rng.integers(-amp, amp + 1, size=n)
    q = env * np.sin(ph) + rng.integers(-amp, amp + 1, size=n)
    if wide:
        idx = rng.integers(0, n, size=n // 40)
        i[idx] = rng.choice([-32768, 32767, -2049, 2048, -2048, 2047], size=idx.size)
        q[idx[::2]] = rng.choice([-32768, 32767], size=idx[::2].size)
    lim = 32767 if wide else 2047
    iq = np.empty(2 * n, dtype=np.int16)
    iq[0::2] = np.clip(np.round(i), -lim - 1, lim).astype(np.int16)
    iq[1::2] = np.clip(np.round(q), -lim - 1, lim).astype(np.int16)
    return iq


@pytest.mark.parametrize("ntaps", [1, 2, 31, 32, 33, 64, 65, 128, 129, 255, 256, 257])
def test_mfma_fir_tap_counts(ok, oracle, tmp_path, ntaps):
    """Single-stage filters of every compiled window length (and one beyond, which stays on the packed-VALU
    kernel): bits of the matrix-core form == oracle == packed-VALU form; floats within the stated tolerance;
    nominal and wide sample ranges; capture lengths that end inside a tile."""
    rng = np.random.default_rng(1000 + ntaps)
    taps = rng.normal(0, 1, ntaps) * np.hamming(ntaps + 2)[1:-1]
    taps = (taps / np.abs(taps).sum() * 1.7).astype(np.float32)
    path = _write_filter(tmp_path, taps, "t%d" % ntaps)
    f = ok.Filter.load(path)
    of = oracle.load_filter_json(path)
    for wide, n in ((False, 70000 + ntaps), (True, 33000)):
        iq = _loud_capture(n, rng, wide)
        y0 = oracle.rx(iq, of, 0.0, None, 8192, want_bits=True, want_fir=True).fir.astype(np.float64)
        thr = float(np.float32(np.median(np.sqrt(y0[:, 0] ** 2 + y0[:, 1] ** 2))))        # in the middle of the output range
        want = oracle.rx(iq, of, thr, None, 8192, want_bits=True, want_fir=True)
        assert 0.2 < want.bits.mean() < 0.8
        scale = float(np.abs(taps).sum()) * float(np.abs(iq.astype(np.int32)).max()) / 2048.0
        for valu in (False, True):
            rx = ok.Receiver(f, None, max_samples=n, threshold=thr, edge_capacity=n + 64, keep_fir=True, fir_valu=valu)
            got = rx.rx(iq)
            form = ok.FRONT_GENERIC if ntaps > 256 else ok.FRONT_FIR1_VALU if valu else ok.FRONT_FIR1_MFMA
            assert got.stats["front_form"] == form, (ntaps, wide, valu)
            assert (rx.bits() == want.bits).all(), (ntaps, wide, valu)
            assert list(rx.edges()) == list(edges_of(want.bits))
            y = rx.fir_output()
            assert (np.abs(y - want.fir) <= FIR_RTOL * np.maximum(np.abs(want.fir), scale)).all(), (ntaps, wide, valu)
            rx.close()
            # and without the float output (quiet shortcut armed, sparse words)
            rx = ok.Receiver(f, None, max_samples=n, threshold=thr, edge_capacity=n + 64, fir_valu=valu)
            got = rx.rx(iq)
            assert got.stats["front_form"] == form, (ntaps, wide, valu)
            assert (rx.bits() == want.bits).all(), (ntaps, wide, valu)
            rx.close()


@pytest.mark.parametrize("scale", [1e-15, 1e-6, 1e-3, 1.0, 37.5, 1e6, 1e15])
def test_mfma_fir_tap_magnitudes(ok, oracle, tmp_path, scale):
    """Taps of any magnitude and dynamic range (a tap 2^-30 of the largest still counts; filters the
    matrix-core form refuses fall back to the packed-VALU loop): bits == oracle with a threshold placed
    in the middle of the output range."""
    rng = np.random.default_rng(77)
    ntaps = 48
    taps = rng.normal(0, 1, ntaps)
    taps[5] *= 2.0 ** -30
    taps[17] = 0.0
    taps = (taps / np.abs(taps).sum() * scale).astype(np.float32)
    path = _write_filter(tmp_path, taps, "m")
    f = ok.Filter.load(path)
    of = oracle.load_filter_json(path)
    n = 50000
    iq = _loud_capture(n, rng, False)
    y = oracle.rx(iq, of, 0.0, None, 8192, want_bits=True, want_fir=True).fir
    mag = np.sqrt(y[:, 0].astype(np.float64) ** 2 + y[:, 1].astype(np.float64) ** 2)
    thr = float(np.float32(np.median(mag)))
    if not np.isfinite(thr) or thr <= 0.0:
        pytest.skip("degenerate output range")
    want = oracle.rx(iq, of, thr, None, 8192, want_bits=True)
    assert 0.2 < want.bits.mean() < 0.8
    rx = ok.Receiver(f, None, max_samples=n, threshold=thr, edge_capacity=n + 64)
    got = rx.rx(iq)
    # the matrix-core form unless plan_real_form refuses: tap scaling beyond 2^+-100 (mfma_prepare_taps), p_star
    # outside [2^-100, 2^100], band edges that do not scale into normal floats in accumulator units (mfma_scale_band)
    _, e = math.frexp(float(np.abs(taps.astype(np.float64)).max()))
    sh = 15 - e
    p = float(np.float32(thr)) ** 2
    lc = math.log2(p) + 2 * (11 + sh)
    refused = abs(sh) > 100 or not (2.0 ** -100 <= p <= 2.0 ** 100) or not (-125 < lc < 127)
    assert got.stats["front_form"] == (ok.FRONT_FIR1_VALU if refused else ok.FRONT_FIR1_MFMA), (scale, refused)
    assert (rx.bits() == want.bits).all()
    rx.close()


def test_mfma_guard_band_forces_exact_recompute_255_taps(ok, oracle, tmp_path):
    """the 255-tap filter with the filtered magnitude hovering around the threshold: every borderline output
    goes through the reference-order recompute (from the capture itself) and the bits are the oracle's"""
    k = np.arange(255) - 127
    h = np.sinc(k / 32.0) * np.hamming(255)
    h = (h / h.sum()).astype(np.float32)
    path = _write_filter(tmp_path, h, "sinc255")
    f = ok.Filter.load(path)
    of = oracle.load_filter_json(path)
    rng = np.random.default_rng(19)
    n = 300000
    base = 204.7 + 0.6 * np.sin(np.arange(n) / 7000.0)
    iq = np.empty(2 * n, np.int16)
    iq[0::2] = np.round(base + rng.normal(0, 3.0, n)).astype(np.int16)
    iq[1::2] = rng.integers(-2, 3, n).astype(np.int16)
    rx = ok.Receiver(f, None, max_samples=n, edge_capacity=n + 1024)
    got = rx.rx(iq)
    want = oracle.rx(iq, of, 0.1, None, 8192, want_bits=True)
    assert got.stats["front_form"] == ok.FRONT_FIR1_MFMA
    assert (rx.bits() == want.bits).all()
    assert got.stats["guard_recomputes"] > 20
    assert 0.05 < want.bits.mean() < 0.95
    rx.close()


# ------------------------------------------------------------- guard band ----

@pytest.mark.parametrize("filt", ["fs32_fs4", "fs128_fs16_dec4"])
def test_guard_band_forces_exact_recompute(ok, oracle, filt):
    """A signal whose filtered magnitude hovers around the threshold: the
    fused path must hand every borderline sample to the exact recompute and
    still produce the oracle's bits."""
    rng = np.random.default_rng(9)
    n = 400000
    of = _ofir(oracle, filt)
    dc = 1.0
    for st in range(of.num_stages):
        dc *= float(of.stage_taps(st).astype(np.float64).sum())
    # amplitude * DC gain ~ 0.1 FS = 204.8 LSB, tiny ramp + noise
    base = 204.6 / dc + 0.8 * np.sin(np.arange(n) / 5000.0)
    i = np.round(base + rng.normal(0, 0.6, n)).astype(np.int16)
    q = rng.integers(-2, 3, n).astype(np.int16)
    iq = np.empty(2 * n, np.int16)
    iq[0::2], iq[1::2] = i, q
    f = _flt(ok, filt)
    rx = ok.Receiver(f, None, max_samples=n, edge_capacity=n + 1024)
    got = rx.rx(iq)
    want = oracle.rx(iq, of, 0.1, None, 8192, want_bits=True)
    assert got.stats["front_form"] == (ok.FRONT_FIR2_MFMA if of.num_stages == 2 else ok.FRONT_FIR1_MFMA)
    assert (rx.bits() == want.bits).all()
    assert got.stats["guard_recomputes"] > 20
    assert list(rx.edges()) == list(edges_of(want.bits))
    assert 0.05 < want.bits.mean() < 0.95


@pytest.mark.parametrize("thr", [0.0, -1.0, 1e-6, 0.5, 0.999, 16.0, 30.0, float("nan")])
def test_threshold_edge_values(ok, oracle, vectors, thr):
    g, iq = _g1(vectors, noise_seed=4)
    iq = iq[:2 * 200000]
    f = _flt(ok, "fs32_fs4")
    of = _ofir(oracle, "fs32_fs4")
    for exact in (False, True):
        rx = ok.Receiver(f, None, max_samples=iq.size // 2, threshold=thr, exact_fir=exact,
                         edge_capacity=iq.size)
        rx.rx(iq)
        want = oracle.rx(iq, of, thr, None, 8192, want_bits=True)
        assert (rx.bits() == want.bits).all(), (thr, exact)


# ---------------------------------------------------------- ragged / empty ----

@pytest.mark.parametrize("n", [0, 1, 3, 31, 64, 4095, 4096, 4097, 8191, 8192, 8193, 20000])
def test_ragged_lengths(ok, oracle, vectors, n):
    g, iq = _g1(vectors, noise_seed=6)
    iq = iq[2 * 11000:2 * (11000 + n)].copy()      # starts inside the idle gap before a pulse
    for filt in ("fs32_fs4", "fs128_fs16_dec4", None):
        _compare(ok, oracle, iq, filt, "p3l-nexa2012", spb=4096)


# ---------------------------------------------------------- state machine ----

def _iq_from_stream(stream, amp=1945):
    iq = np.zeros(2 * stream.size, dtype=np.int16)
    iq[0::2] = stream.astype(np.int16) * amp
    return iq


def test_g7_tolerance_boundaries(ok, oracle, vectors):
    g = vectors["G7"]
    from tests.golden import make_golden as mg
    d = _dev(ok, g["device"])
    for c in g["cases"]:
        runs = mg.p3l_runs(g["payload_bits"], **{c["param"]: c["value"]})
        iq = _iq_from_stream(stream_from_runs(runs))
        for fsm_rounds in (False, True):
            rx = ok.Receiver(None, d, max_samples=iq.size // 2, samples_per_buffer=g["spb"],
                             fsm_rounds=fsm_rounds)
            got = rx.rx(iq)
            assert list(got.msg_samples) == c["msg_samples"], (c, fsm_rounds)
            rx.close()


def _glitchy_message_runs(devname, nmsg, seed):
    """Run lengths of nmsg messages with 1-3 short pulses inside bit gaps each (placed
    before any bit window opens, so the messages still decode)."""
    sh = {"p3l-nexa2012": dict(bits=36, start=500, first=8700, pulse=500, gap0=2000, gap1=4000),
          "unknown-remote1": dict(bits=32, start=8900, first=4400, pulse=550, gap0=550, gap1=1700)}[devname]
    rng = np.random.default_rng(seed)
    us = RATE // 1000000
    runs = [5000]
    for m in range(nmsg):
        runs += [sh["start"] * us, sh["first"] * us]
        bits = rng.integers(0, 2, size=sh["bits"])
        hit = {int(x) for x in rng.choice(sh["bits"], size=1 + m % 3, replace=False)}
        for i, bit in enumerate(bits):
            gap = (sh["gap1"] if bit else sh["gap0"]) * us
            runs.append(sh["pulse"] * us)
            if i in hit and gap > 900:
                a = int(rng.integers(100, min(gap - 700, 900)))     # ends before any bit window opens
                g = int(rng.integers(20, 400))
                runs += [a, g, gap - a - g]          # gap = a + glitch + rest: the rising edge still sees `gap`
            else:
                runs.append(gap)
        runs += [sh["pulse"] * us, int(rng.integers(12000, 40000))]
    return runs


@pytest.mark.parametrize("devname", ["p3l-nexa2012", "unknown-remote1"])
def test_glitches_inside_bit_gaps_stay_in_the_scan(ok, oracle, devname):
    """A short pulse inside a bit gap: no trigger fires on its two edges (bit_off_time
    has no window for them), the counter runs on and the next real edge is judged by the
    whole gap -- the reference decodes the message as if nothing had happened.  The scan
    form holds such stretches as "stuck" codes; with 70 messages and the glitch at a
    different bit each time the stretches cross chunk (16 leaves), block (64) and group
    (1024) boundaries.  Must not fall back, must equal the oracle."""
    runs = _glitchy_message_runs(devname, 70, seed=77)
    iq = _iq_from_stream(stream_from_runs(runs))
    d = _dev(ok, devname)
    od = _odev(oracle, devname)
    want = oracle.rx(iq, None, 0.1, od, 8192)
    assert len(want.msg_samples) >= 60          # the glitches do not break the messages
    for spb in (8192, 1000):
        want = oracle.rx(iq, None, 0.1, od, spb)
        rx = ok.Receiver(None, d, max_samples=iq.size // 2, samples_per_buffer=spb)
        got = rx.rx(iq)
        assert got.stats["fsm_path"] == 1, got.stats["fsm_fallback_reason"]
        assert list(got.msg_samples) == list(want.msg_samples)
        assert (got.payloads == want.payloads).all()
        assert got.stats["num_errors"] == len(want.err_samples)
        rx.close()


def test_short_randomised_differential_run():
    """200 captures of tools/fuzz_gpu.py (fixed seed): jittered and glitched message
    streams on the shipped devices, a third of them on random state machines; scan with
    tables, scan with simulation and rounds, each against the oracle."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "fuzz_gpu.py"), "--cases", "200", "--seed", "5",
                        "--random-devices", "0.3"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["cases"] >= 200 and out["mismatches"] == []


@pytest.mark.parametrize("segment_buffers", [1, 3, 0, -1])
def test_reference_fsm_fixtures_random_streams(ok, oracle, vectors, segment_buffers):
    # segment_buffers >= 0: the round path with that segment size; -1: the scan path
    fsm_rounds = segment_buffers >= 0
    segment_buffers = max(segment_buffers, 0)
    for case in vectors["random_streams"]:
        d = _dev(ok, case["device"], case["rate"])
        iq = _iq_from_stream(stream_from_runs(case["runs"]))
        for buf, want in case["ref_fsm"].items():
            rx = ok.Receiver(None, d, max_samples=iq.size // 2, samples_per_buffer=int(buf),
                             segment_buffers=segment_buffers, fsm_rounds=fsm_rounds)
            got = rx.rx(iq)
            # the file backend pads the capture to whole buffers; the fixtures
            # were cut at the end of the stream: ignore anything in the padding
            keep = got.msg_samples < len(iq) // 2
            assert list(got.msg_samples[keep]) == want["msg_samples"], (case["device"], buf)
            assert [bytes(p).hex() for p in got.payloads[keep]] == want["payloads"]
            rx.close()


def test_random_devices_match_oracle(ok, oracle):
    from tests.test_oracle import _random_fsm
    rng = np.random.default_rng(123)
    for it in range(40):
        rate = int(rng.choice([3000000, 1000000, 750000, 48000]))
        od = _random_fsm(oracle, rng, rate)
        d = ok.Device.from_tables(
            max_bits=od.max_bits, sample_rate=rate, state_duration_us=od.state_duration_us,
            state_timeout_us=od.state_timeout_us, trig_begin=od.trig_begin, trig_cond=od.trig_cond,
            trig_action=od.trig_action, trig_next=od.trig_next, trig_duration_us=od.trig_duration_us)
        scale = rate / 1e6
        runs = [max(1, int(rng.choice([30, 60, 100, 200, 250, 400, 1000, 5000]) * scale
                       * rng.uniform(0.8, 1.2))) for _ in range(int(rng.integers(20, 300)))]
        stream = stream_from_runs(runs)
        iq = _iq_from_stream(stream)
        for spb, segb, fsm_rounds in ((97, 1, True), (512, 2, False), (4096, 3, True), (4096, 3, False)):
            # a random device may emit a message on every sample: one slot per sample.
            # fsm_rounds False: the scan runs where it can and hands over to the
            # rounds where the device leaves its model -- either way the oracle's result.
            rx = ok.Receiver(None, d, max_samples=iq.size // 2, samples_per_buffer=spb,
                             segment_buffers=segb, message_slots=2 * spb * segb + 2,
                             message_capacity=1 << 20, edge_capacity=iq.size, fsm_rounds=fsm_rounds)
            got = rx.rx(iq)
            want = oracle.rx(iq, None, 0.1, od, spb, msg_cap=1 << 20)
            assert list(got.msg_samples) == list(want.msg_samples), (it, spb)
            assert (got.payloads == want.payloads).all(), (it, spb)
            assert got.stats["num_errors"] == len(want.err_samples), (it, spb)
            errs, nerr = rx.errors(len(want.err_samples) + 8)
            assert nerr == len(want.err_samples) and list(errs) == list(want.err_samples), (it, spb)
            rx.close()


def test_devices_beyond_64_states_run_through_the_round_form(ok, oracle):
    """The reference allocates states and triggers dynamically (state_machine.c:135-235).  Devices with more
    than 64 of either decode through the round form with their tables in LDS: a 100-state / ~250-trigger
    random machine and one state with 70 triggers (more than one lane group), over a thousand segments."""
    from tests.test_oracle import _random_fsm
    rng = np.random.default_rng(4242)
    for it, (ns, mt) in enumerate(((100, 4), (100, 5), (3, 72), (130, 3))):
        rate = int(rng.choice([3000000, 1000000]))
        od = _random_fsm(oracle, rng, rate, ns=ns, max_triggers=mt)
        assert len(od.state_duration_us) > 64 or len(od.trig_cond) > 64
        d = ok.Device.from_tables(
            max_bits=od.max_bits, sample_rate=rate, state_duration_us=od.state_duration_us,
            state_timeout_us=od.state_timeout_us, trig_begin=od.trig_begin, trig_cond=od.trig_cond,
            trig_action=od.trig_action, trig_next=od.trig_next, trig_duration_us=od.trig_duration_us)
        scale = rate / 1e6
        runs = [max(1, int(rng.choice([30, 60, 100, 200, 250, 400, 1000, 5000]) * scale
                       * rng.uniform(0.8, 1.2))) for _ in range(6000)]
        stream = stream_from_runs(runs)
        iq = _iq_from_stream(stream)
        n = iq.size // 2
        spb = 1024
        segb = max(1, n // spb // 1100)         # > 1 000 segments
        rx = ok.Receiver(None, d, max_samples=n, samples_per_buffer=spb, segment_buffers=segb,
                         message_slots=2 * spb * segb + 2, message_capacity=1 << 22, edge_capacity=n)
        got = rx.rx(iq)
        want = oracle.rx(iq, None, 0.1, od, spb, msg_cap=1 << 22)
        assert got.stats["fsm_path"] == 2 and got.stats["num_segments"] >= 1000, got.stats
        assert list(got.msg_samples) == list(want.msg_samples), it
        assert (got.payloads == want.payloads).all(), it
        assert got.stats["num_errors"] == len(want.err_samples), it
        errs, nerr = rx.errors(len(want.err_samples) + 8)
        assert nerr == len(want.err_samples) and list(errs) == list(want.err_samples), it
        rx.close()


# ------------------------------------------------------- batched / sharded ----

@pytest.mark.parametrize("walk", [False, True])
def test_batched_captures_are_independent(ok, oracle, vectors, walk):
    import torch
    g, iq = _g1(vectors)
    n = 300000
    caps = []
    for c in range(5):
        rng = np.random.default_rng(100 + c)
        off = int(rng.integers(0, 600000))
        x = iq[2 * off:2 * (off + n)].copy()
        x = (x + rng.integers(-40, 41, size=x.size)).astype(np.int16)
        caps.append(x)
    stride = n + 12          # padded stride, multiple of 4 samples
    host = np.zeros((5, 2 * stride), dtype=np.int16)
    for c in range(5):
        host[c, :2 * n] = caps[c]
    dev_t = torch.from_numpy(host).cuda()
    f = _flt(ok, "fs32_fs4")
    d = _dev(ok, "p3l-nexa2012")
    with _sync_walk_forced(walk):          # (the scan's walk from synchronising spans: whatever the edge count)
        rx = ok.Receiver(f, d, max_samples=n, max_captures=5)
    got = rx.rx_device(dev_t.data_ptr(), n, num_captures=5, stride=stride)
    of = _ofir(oracle, "fs32_fs4")
    od = _odev(oracle, "p3l-nexa2012")
    total = 0
    for c in range(5):
        want = oracle.rx(caps[c], of, 0.1, od, 8192, want_bits=True)
        assert (rx.bits(c) == want.bits).all(), c
        gc = got.for_capture(c)
        assert list(gc.msg_samples) == list(want.msg_samples)
        assert (gc.payloads == want.payloads).all()
        total += len(want.msg_samples)
    assert total == len(got.msg_samples)


@pytest.mark.parametrize("walk", [False, True])
def test_batched_captures_with_glitches_inside_bit_gaps(ok, oracle, walk):
    """Six independent captures in one call, each with stuck stretches (and the first edges of
    a capture right behind one): per capture the oracle's messages, all in the scan form."""
    import torch
    caps = [_iq_from_stream(stream_from_runs(_glitchy_message_runs("p3l-nexa2012", 6 + c, seed=300 + c)))
            for c in range(6)]
    n = max(x.size // 2 for x in caps)
    n += (-n) % 4
    stride = n + 8
    host = np.zeros((len(caps), 2 * stride), dtype=np.int16)
    for c, x in enumerate(caps):
        host[c, :x.size] = x
    dev_t = torch.from_numpy(host).cuda()
    d = _dev(ok, "p3l-nexa2012")
    od = _odev(oracle, "p3l-nexa2012")
    with _sync_walk_forced(walk):
        rx = ok.Receiver(None, d, max_samples=n, max_captures=len(caps))
    got = rx.rx_device(dev_t.data_ptr(), n, num_captures=len(caps), stride=stride)
    assert got.stats["fsm_path"] == 1, got.stats["fsm_fallback_reason"]
    total = 0
    for c in range(len(caps)):
        want = oracle.rx(host[c, :2 * n], None, 0.1, od, 8192)
        gc = got.for_capture(c)
        assert list(gc.msg_samples) == list(want.msg_samples), c
        assert (gc.payloads == want.payloads).all(), c
        assert len(want.msg_samples) >= 5 + c
        total += len(want.msg_samples)
    assert total == len(got.msg_samples)
    rx.close()


@pytest.mark.parametrize("walk", [False, True])
def test_batch_with_one_refused_capture_redoes_only_that_one(ok, oracle, walk):
    """A stretch of inert edges deeper than the scan's stuck codes hold (six short pulses inside ONE bit
    gap of p3l-nexa2012: twelve edges on which nothing fires) makes the scan refuse that capture.  In a
    batch the other captures keep the scan's results; the refused one is redone alone in the round form
    and merged in, in capture order -- messages, payloads and error counts per capture as the oracle's."""
    import torch
    from tests.in_flight_inputs import p3l_message_captures
    plain0, deep, plain1 = p3l_message_captures((False, True, False))      # (the builder lives beside the in-flight captures)
    caps = [plain0, deep, _iq_from_stream(stream_from_runs(_glitchy_message_runs("p3l-nexa2012", 5, seed=5))), plain1]
    n = max(c.size // 2 for c in caps)
    stride = n + 8
    host = np.zeros((len(caps), 2 * stride), dtype=np.int16)
    for c, x in enumerate(caps):
        host[c, :x.size] = x
    dev_t = torch.from_numpy(host).cuda()
    d = _dev(ok, "p3l-nexa2012")
    od = _odev(oracle, "p3l-nexa2012")
    # alone, the deep capture leaves the scan (otherwise this test tests nothing)
    solo = ok.Receiver(None, d, max_samples=n)
    r1 = solo.rx(host[1, :2 * n])
    assert r1.stats["fsm_path"] == 3 and r1.stats["fsm_fallback_reason"] != 0
    solo.close()
    with _sync_walk_forced(walk):
        rx = ok.Receiver(None, d, max_samples=n, max_captures=len(caps))
    for order in ((0, 1, 2, 3), (0, 2, 3)):                 # with the refused capture, then a clean batch on the same context
        sub = torch.from_numpy(host[list(order)].copy()).cuda()
        got = rx.rx_device(sub.data_ptr(), n, num_captures=len(order), stride=stride)
        assert got.stats["fsm_path"] == (3 if 1 in order else 1), got.stats
        total = nerr = 0
        kept, redone = [], []           # error positions (capture-local) of the captures the scan kept / refused
        for i, c in enumerate(order):
            want = oracle.rx(host[c, :2 * n], None, 0.1, od, 8192)
            gc = got.for_capture(i)
            assert list(gc.msg_samples) == list(want.msg_samples), c
            assert (gc.payloads == want.payloads).all(), c
            total += len(want.msg_samples)
            nerr += len(want.err_samples)
            (redone if c == 1 else kept).extend(int(x) for x in want.err_samples)
        assert total == len(got.msg_samples) and total >= 15
        assert got.stats["num_errors"] == nerr
        errs, ne = rx.errors()
        assert ne == nerr and len(errs) == nerr
        # capture-major; with fsm_path 3 the refused capture's errors follow those of all the others (ookiedokie_amd.h)
        assert [int(x) for x in errs] == kept + redone
    rx.close()


def _check_sharded(ok, oracle, iq, filt, devname, shard_buffers, walk=False):
    """One capture cut into shards (as 8 GPUs would hold it): halo + carried
    FSM state reproduce the single-pass result."""
    import torch
    of = _ofir(oracle, filt)
    dec = of.total_decimation if of else 1
    f = _flt(ok, filt)
    d = _dev(ok, devname, RATE // dec)
    od = _odev(oracle, devname, RATE // dec)
    spb = 8192
    n = iq.size // 2
    want = oracle.rx(iq, of, 0.1, od, spb, want_bits=True)
    shard = shard_buffers * spb
    bounds = list(range(0, n, shard)) + [n]
    nsh = len(bounds) - 1
    rxs, outs, bits = [], [None] * nsh, [None] * nsh
    dev_t = torch.from_numpy(iq.copy()).cuda()
    ins = [None] * nsh
    H = None
    for r in range(nsh):
        with _sync_walk_forced(walk):      # (shards begun and refined through the scan's walk from synchronising spans)
            rx = ok.Receiver(f, d, max_samples=shard, samples_per_buffer=spb)
        H = rx.halo_samples
        lo, hi = bounds[r], bounds[r + 1]
        halo = iq[2 * (lo - H):2 * lo] if r > 0 and H else None
        _, out = rx.shard_begin(dev_t.data_ptr() + 4 * lo, hi - lo, halo, r == nsh - 1, None)
        rxs.append(rx)
        outs[r] = out
    # propagate the carried state until nothing changes (what ranks do over RCCL)
    for _round in range(nsh + 1):
        changed = False
        for r in range(1, nsh):
            if ins[r] is None or ins[r].key() != outs[r - 1].key():
                ins[r] = outs[r - 1]
                _, o = rxs[r].shard_refine(ins[r])
                if o.key() != outs[r].key():
                    changed = True
                outs[r] = o
        if not changed:
            break
    msgs, pays = [], []
    off = 0
    for r in range(nsh):
        res = rxs[r]._result()
        msgs += [int(s) + off for s in res.msg_samples]
        pays += [bytes(p) for p in res.payloads]
        b = rxs[r].bits()
        assert (b == want.bits[off:off + b.size]).all(), r
        off += b.size
        rxs[r].close()
    assert off == want.decimated
    assert msgs == list(want.msg_samples)
    assert pays == [bytes(p) for p in want.payloads]
    return len(msgs)


@pytest.mark.parametrize("filt", ["fs32_fs4", "fs128_fs16_dec4"])
def test_sharded_capture_equals_whole(ok, oracle, vectors, filt):
    g, iq = _g1(vectors, noise_seed=21)
    assert _check_sharded(ok, oracle, iq, filt, "p3l-nexa2012", 40) == 3


@pytest.mark.parametrize("walk", [False, True])
def test_sharded_capture_with_glitches_inside_bit_gaps(ok, oracle, walk):
    """Shard boundaries that fall into messages whose bit gaps hold glitch pulses: a shard
    may begin inside a stretch in which no trigger fires (carried counter != 0)."""
    iq = _iq_from_stream(stream_from_runs(_glitchy_message_runs("p3l-nexa2012", 24, seed=5)))
    assert _check_sharded(ok, oracle, iq, None, "p3l-nexa2012", 7, walk=walk) >= 20


# ------------------------------------------------------- fine-grained APIs ----

@pytest.mark.parametrize("filt", ["fs32_fs4", "fs128_fs16_dec4", "unity16"])
@pytest.mark.parametrize("chunk", [7, 33, 1000, 8192])
def test_stream_fir_matches_oracle_for_any_chunking(ok, oracle, vectors, filt, chunk):
    g, iq = _g1(vectors, noise_seed=31)
    x = oracle.unpack(iq[:2 * 30000])
    sf = ok.StreamFir(_flt(ok, filt), 8192)
    outs = [sf.filter_and_decimate(x[o:o + chunk]) for o in range(0, x.shape[0], chunk)]
    y = np.concatenate(outs)
    want = oracle.fir_run(_ofir(oracle, filt), x, chunk)
    assert y.shape == want.shape
    assert (y.view(np.uint32) == want.view(np.uint32)).all()
    sf.reset()
    y2 = sf.filter_and_decimate(x[:100])
    assert (y2.view(np.uint32) == want[:y2.shape[0]].view(np.uint32)).all()


def test_fir_impulse_known_answers(ok, oracle):
    x = np.zeros((100, 2), np.float32)
    x[49, 0] = 1.0
    f = _flt(ok, "fs32_fs4")
    y = ok.StreamFir(f, 4096).filter_and_decimate(x)
    _, taps = f.stage(0)
    assert (y[49:81, 0].view(np.uint32) == taps.view(np.uint32)).all() and not y[:, 1].any()
    y = ok.StreamFir(_flt(ok, "unity16"), 4096).filter_and_decimate(x)
    assert list(np.nonzero(y[:, 0])[0]) == list(range(49, 65))


@pytest.mark.parametrize("name", ["fs32_fs4", "fs128_fs16_dec4"])
@pytest.mark.parametrize("period", [4.0, 32.0])
def test_fir_harness_tones_steady_state(ok, name, period):
    """src/matlab/gen_samples.m:19-34 on the GPU FIR: behind the start-up the output is H(w) * tone, a
    known answer independent of any restatement of the filter loop (1e-5 of sum|h|)."""
    from tests.helpers import harness_tone, steady_state_response
    f = _flt(ok, name)
    x = harness_tone(400000, period)
    fir = ok.StreamFir(f, 65536)             # fed like the reference feeds fir_filter_and_decimate: max_input at a time
    y = np.concatenate([fir.filter_and_decimate(x[i:i + 65536]) for i in range(0, x.shape[0], 65536)])
    taps = [f.stage(s)[1] for s in range(f.num_stages)]
    decs = [f.stage(s)[0] for s in range(f.num_stages)]
    want, first = steady_state_response(taps, decs, x.shape[0], period)
    assert y.shape[0] == want.size
    got = y[:, 0].astype(np.float64) + 1j * y[:, 1].astype(np.float64)
    tol = 1e-5 * float(np.prod([np.abs(t).sum() for t in taps]))
    assert np.abs(got[first + 64:] - want[first + 64:]).max() <= tol


def test_fir_harness_long_impulse(ok):
    # gen_samples.m:13-16: 10^6 samples, impulse at sample 1000
    x = np.zeros((1000000, 2), np.float32)
    x[999, 0] = 1.0
    f = _flt(ok, "fs32_fs4")
    fir = ok.StreamFir(f, 65536)
    y = np.concatenate([fir.filter_and_decimate(x[i:i + 65536]) for i in range(0, x.shape[0], 65536)])
    _, taps = f.stage(0)
    assert (y[999:1031, 0].view(np.uint32) == taps.view(np.uint32)).all()
    assert not y[:999].any() and not y[1031:].any()


def test_backend_rx_matches_file_backend_semantics(ok, oracle, vectors, tmp_path):
    g, iq = _g1(vectors, noise_seed=41)
    iq = iq[:2 * 20000].copy()
    path = tmp_path / "cap.sc16q11"
    iq.tofile(path)
    be = ok.HipFileBackend(str(path), samples_per_buffer=8192)
    chunks, status = [], 0
    while status == 0:
        status, x = be.rx(8192)
        if status == 0:
            chunks.append(x)
    assert status == ok.FILE_EOF
    y = np.concatenate(chunks)
    assert y.shape[0] == 3 * 8192                   # short final read zero padded
    want = oracle.unpack(iq)
    assert (y[:20000].view(np.uint32) == want.view(np.uint32)).all()
    assert not y[20000:].any()
    ptr, n = be.capture()
    assert n == 20000 and ptr
    f = _flt(ok, "fs32_fs4")
    rx = ok.Receiver(f, None, max_samples=n)
    rx.rx_device(ptr, n)
    assert (rx.bits() == oracle.rx(iq, _ofir(oracle, "fs32_fs4"), 0.1, None, 8192,
                                   want_bits=True).bits).all()


def test_synth_device_fill_equals_host_fill(ok):
    import torch
    d = _dev(ok, "p3l-nexa2012")
    n = 3_000_001
    syn = ok.Synth(d, n, seed=77)
    t = torch.empty(2 * n, dtype=torch.int16, device="cuda")
    syn.fill_device(t.data_ptr())
    torch.cuda.synchronize()
    assert (t.cpu().numpy() == syn.fill_host()).all()
    t2 = torch.empty(2 * 1000, dtype=torch.int16, device="cuda")
    syn.fill_device(t2.data_ptr(), first=1234567, count=1000)
    torch.cuda.synchronize()
    assert (t2.cpu().numpy() == syn.fill_host(1234567, 1000)).all()


# ------------------------------------------------------------ bench shape ----

def test_synthetic_capture_matches_oracle_16M(ok, oracle):
    """BASELINE config-2 recipe at a size the oracle finishes in seconds."""
    import torch
    d = _dev(ok, "p3l-nexa2012")
    od = _odev(oracle, "p3l-nexa2012")
    n = 1 << 24
    syn = ok.Synth(d, n, seed=0x00C0FFEE + 2)
    t = torch.empty(2 * n, dtype=torch.int16, device="cuda")
    syn.fill_device(t.data_ptr())
    torch.cuda.synchronize()
    f = _flt(ok, "fs32_fs4")
    rx = ok.Receiver(f, d, max_samples=n)
    got = rx.rx_device(t.data_ptr(), n)
    iq = t.cpu().numpy()
    want = oracle.rx(iq, _ofir(oracle, "fs32_fs4"), 0.1, od, 8192, want_bits=True)
    assert (rx.bits() == want.bits).all()
    assert list(got.msg_samples) == list(want.msg_samples)
    assert (got.payloads == want.payloads).all()
    assert got.stats["num_errors"] == len(want.err_samples)
    # decoded payloads are a subsequence of what was transmitted
    sent = [syn.message(i)[1] for i in range(syn.num_messages)]
    it = iter(sent)
    assert all(any(bytes(p) == s for s in it) for p in got.payloads)
    assert len(got.msg_samples) >= 0.8 * (syn.num_messages - 2)


def test_full_size_properties_1GiB(ok):
    """BASELINE config 2 at full size (268 435 456 samples): properties that
    do not need the oracle -- every decoded payload was transmitted, in
    order; OUTPUT_READY follows each decoded message's start by the known
    waveform length; the decode is idempotent; the edge list is sorted."""
    import torch
    d = _dev(ok, "p3l-nexa2012")
    n = 1 << 28
    syn = ok.Synth(d, n, seed=0x00C0FFEE + 2)
    t = torch.empty(2 * n + 2 * 8192, dtype=torch.int16, device="cuda")
    syn.fill_device(t.data_ptr())
    torch.cuda.synchronize()
    f = _flt(ok, "fs32_fs4")
    rx = ok.Receiver(f, d, max_samples=n)
    got = rx.rx_device(t.data_ptr(), n)
    again = rx.rx_device(t.data_ptr(), n)
    assert list(got.msg_samples) == list(again.msg_samples)
    assert (got.payloads == again.payloads).all()
    starts = np.array([syn.message(i)[0] for i in range(syn.num_messages)])
    sent = [syn.message(i)[1] for i in range(syn.num_messages)]
    assert len(got.msg_samples) >= 0.8 * (len(sent) - 2)
    j = 0
    for s, p in zip(got.msg_samples, got.payloads):
        while j < len(sent) and sent[j] != bytes(p):
            j += 1
        assert j < len(sent), "decoded a payload that was never sent"
        # OUTPUT_READY lands inside the transmitted waveform of that message
        assert starts[j] < int(s) < starts[j] + 500000
        j += 1
    # edge list is sorted and consistent with the bit stream's popcount of changes
    e = rx.edges()
    assert (np.diff(e.astype(np.int64)) > 0).all()
    assert got.stats["num_edges"] == e.size


# ------------------------------------------------------------------ hygiene ----

def test_contexts_release_their_memory(ok, vectors):
    """Create / run / destroy in a loop: device memory must come back (buffers,
    pinned staging, streams, events of rx contexts, formatters, backends)."""
    import torch
    g, iq = _g1(vectors)
    iq = iq[:2 * 300000]
    f = _flt(ok, "fs128_fs16_dec4")
    d = _dev(ok, "p3l-nexa2012", RATE // 4)

    def once():
        rx = ok.Receiver(f, d, max_samples=iq.size // 2, keep_fir=True)
        rx.rx(iq)                               # host path: pinned ingest buffers too
        rx.fir_sc16q11()
        rx.dig_text()
        fm = ok.Formatter(d)
        fm.print_messages(rx.result(), 8192, 4)
        fm.close()
        rx.close()

    once()
    torch.cuda.synchronize()
    free0, _ = torch.cuda.mem_get_info()
    for _ in range(12):
        once()
    torch.cuda.synchronize()
    free1, _ = torch.cuda.mem_get_info()
    assert free0 - free1 < 8 << 20, "device memory shrank by %d bytes over 12 create/destroy cycles" % (free0 - free1)


def test_context_is_reusable_across_sizes(ok, oracle, vectors):
    """One context, captures of different lengths back to back (state of the
    previous run must not leak into the next: header counters, tile info,
    stamped aggregates, edge lists)."""
    g, iq = _g1(vectors, noise_seed=31)
    f = _flt(ok, "fs32_fs4")
    of = _ofir(oracle, "fs32_fs4")
    d = _dev(ok, "p3l-nexa2012")
    od = _odev(oracle, "p3l-nexa2012")
    rx = ok.Receiver(f, d, max_samples=iq.size // 2)
    for n in (iq.size // 2, 5000, 0, 450000, 1, iq.size // 2, 820000):
        part = iq[:2 * n]
        got = rx.rx(part)
        want = oracle.rx(part, of, 0.1, od, 8192, want_bits=True)
        assert list(got.msg_samples) == list(want.msg_samples), n
        assert (got.payloads == want.payloads).all()
        assert list(rx.edges()) == list(edges_of(want.bits)), n
    rx.close()


@pytest.mark.parametrize("filt", ["fs32_fs4", "fs128_fs16_dec4"])
# (the ids keep the shape they had when a case also chose between two front-end forms)
@pytest.mark.parametrize("chunk,read_bits,stamp0", [pytest.param(0, True, None, id="0-False-True-None"),
                                                    pytest.param(32768, True, None, id="32768-False-True-None"),
                                                    pytest.param(0, False, None, id="0-False-False-None"),
                                                    pytest.param(32768, False, None, id="32768-False-False-None"),
                                                    pytest.param(0, False, 0xffff - 3, id="0-False-False-65532"),
                                                    pytest.param(0, True, 0xffff - 2, id="0-False-True-65533")])
def test_sparse_bit_words_do_not_leak_between_runs(ok, oracle, vectors, chunk, read_bits, stamp0, filt, monkeypatch):
    """The tuned front ends (1 stage; the two decimate-by-2 stages of the backend default) store nothing for quiet tiles: what earlier runs left in their words
    and tile infos carries those runs' stamps and must read as quiet (kernels.hpp: tile_live), for the
    edge stage, the state machine and -- after ookd_rx_get_bits has zeroed the stale tiles -- for the
    raw words.  Different captures of equal and of different lengths through one context, whole and
    pipelined in chunks, with the words read back after
    every run (which cleans up) and never (stale tiles of many runs pile up), and across the wrap of the
    16-bit stamp: bits, edges and messages of every run must be the oracle's."""
    if stamp0 is not None:
        monkeypatch.setenv("OOKD_DEVELOPER", "1")
        monkeypatch.setenv("OOKD_TILE_STAMP_START", str(stamp0))
    g, a = _g1(vectors, noise_seed=41)
    rng = np.random.default_rng(42)
    shift = 2 * 77000                       # the same waveform moved: pulses where A has silence
    b = np.concatenate([rng.integers(-40, 41, size=shift).astype(np.int16), a[:-shift]])
    c = rng.integers(-40, 41, size=a.size).astype(np.int16)         # silence: nothing may survive
    f = _flt(ok, filt)
    of = _ofir(oracle, filt)
    d = _dev(ok, "p3l-nexa2012", RATE // of.total_decimation)
    od = _odev(oracle, "p3l-nexa2012", RATE // of.total_decimation)
    rx = ok.Receiver(f, d, max_samples=a.size // 2, pipeline_chunk_samples=chunk)
    for name, iq in (("a", a), ("b", b), ("c", c), ("a", a), ("b half", b[:b.size // 2]), ("a", a), ("c third", c[:2 * 400000]),
                     ("b", b)):
        got = rx.rx(iq)
        want = oracle.rx(iq, of, 0.1, od, 8192, want_bits=True)
        if read_bits:
            bits = rx.bits()
            diff = np.nonzero(bits != want.bits)[0]
            assert diff.size == 0, "%s: first differing bit at %s" % (name, diff[:5])
        assert list(rx.edges()) == list(edges_of(want.bits)), name
        assert list(got.msg_samples) == list(want.msg_samples), name
        assert (got.payloads == want.payloads).all(), name
    rx.close()


def test_submit_wait_two_contexts(ok, oracle, vectors):
    """ookd_rx_submit_device / ookd_rx_wait with two contexts in flight give the
    results of the blocking call, whatever the interleaving."""
    import torch
    g, iq = _g1(vectors, noise_seed=41)
    f = _flt(ok, "fs32_fs4")
    d = _dev(ok, "p3l-nexa2012")
    want = oracle.rx(iq, _ofir(oracle, "fs32_fs4"), 0.1, _odev(oracle, "p3l-nexa2012"), 8192)
    n = iq.size // 2
    t = torch.from_numpy(iq.copy()).cuda()
    gate = ok.FrontGate()               # the two contexts take turns for their front ends
    a = ok.Receiver(f, d, max_samples=n, front_gate=gate)
    b = ok.Receiver(f, d, max_samples=n, front_gate=gate)
    with pytest.raises(ok.OokdError):
        a.wait()                            # nothing submitted
    for _ in range(3):
        a.submit_device(t.data_ptr(), n)
        b.submit_device(t.data_ptr(), n)
        with pytest.raises(ok.OokdError):
            a.submit_device(t.data_ptr(), n)    # one run in flight per context
        b.wait()
        a.wait()
        for r in (a.result(), b.result()):
            assert list(r.msg_samples) == list(want.msg_samples)
            assert (r.payloads == want.payloads).all()
    a.close()
    b.close()


@pytest.mark.parametrize("filt,leaf_form", [("fs128_fs16_dec4", None), ("fs32_fs4", None), ("fs128_fs16_dec4", "block")])
def test_fresh_contexts_and_shards_repeat_exactly(ok, oracle, vectors, filt, leaf_form, monkeypatch):
    """The same capture through a dozen freshly made contexts, whole and as two shards (halo, carried state,
    refine): every one of them must give the oracle's messages.  Fresh contexts get fresh (dirty) device
    memory and their kernels land wherever the chip has room, so anything read before it is written, or
    depending on which workgroup took which block, shows up here as a run that differs from its
    neighbours.  leaf_form "block": the scan's workgroup-per-block leaf kernel (what runs without span
    tables), otherwise the wave-per-block one."""
    from ookiedokie_amd.distributed import shard_bounds
    if leaf_form:
        monkeypatch.setenv("OOKD_DEVELOPER", "1")
        monkeypatch.setenv("OOKD_SCAN_LEAF", leaf_form)
    g, iq = _g1(vectors, noise_seed=21)
    n = iq.size // 2
    import torch
    f = _flt(ok, filt)
    rate = RATE // f.total_decimation
    d = ok.Device.load(golden_path("devices", "p3l-nexa2012"), rate)
    od = oracle.load_device_json(golden_path("devices", "p3l-nexa2012"), rate)[0]
    want = oracle.rx(iq, _ofir(oracle, filt), 0.1, od, 8192)
    want_msgs = [int(s) for s in want.msg_samples]
    assert len(want_msgs) == 3
    cap = torch.from_numpy(iq.copy()).cuda()
    b = shard_bounds(n, 2, 8192, f.total_decimation)
    for it in range(12):
        rxw = ok.Receiver(f, d, max_samples=n, samples_per_buffer=8192)
        whole = rxw.rx_device(cap.data_ptr(), n)
        assert [int(s) for s in whole.msg_samples] == want_msgs, (it, "whole")
        assert (whole.payloads == want.payloads).all()
        rxw.close()
        rx0 = ok.Receiver(f, d, max_samples=b[1], samples_per_buffer=8192)
        rx1 = ok.Receiver(f, d, max_samples=n - b[1], samples_per_buffer=8192)
        H = rx0.halo_samples
        r0, s0 = rx0.shard_begin(cap.data_ptr(), b[1], None, False, None)
        halo = cap[2 * (b[1] - H):2 * b[1]]
        r1, s1 = rx1.shard_begin(cap.data_ptr() + 4 * b[1], n - b[1], halo, True, None)
        if bytes(s0) != bytes(ok.FsmState()):
            r1, s1 = rx1.shard_refine(s0)
        got = [int(x) for x in r0.msg_samples] + [int(x) + b[1] // f.total_decimation for x in r1.msg_samples]
        assert got == want_msgs, (it, "sharded", r0.stats["fsm_path"], r1.stats["fsm_path"])
        rx0.close()
        rx1.close()


@pytest.mark.parametrize("short_by", [1, 9, 100])
def test_edge_list_overflow_with_a_state_machine_is_refused_cleanly(ok, oracle, vectors, short_by):
    """An edge list a few entries too small for the capture (round-1 advisor finding: the scan form sized its
    buffers by the capacity and never looked at the overflow flag): the call must fail with the capacity
    error -- not decode something, not touch what lies behind its buffers -- and a context made and run right
    after it, whose buffers are likely to be the neighbours in device memory, must still decode the capture
    exactly."""
    g, iq = _g1(vectors, noise_seed=41)
    n = iq.size // 2
    f = _flt(ok, "fs32_fs4")
    d = _dev(ok, "p3l-nexa2012")
    want = oracle.rx(iq, _ofir(oracle, "fs32_fs4"), 0.1, _odev(oracle, "p3l-nexa2012"), 8192, want_bits=True)
    nedges = len(edges_of(want.bits))
    assert nedges > 200
    small = ok.Receiver(f, d, max_samples=n, edge_capacity=nedges - short_by)
    good = ok.Receiver(f, d, max_samples=n)
    for _ in range(3):
        with pytest.raises(ok.OokdError):
            small.rx(iq)
        got = good.rx(iq)
        assert list(got.msg_samples) == list(want.msg_samples) and (got.payloads == want.payloads).all()
        assert list(good.edges()) == list(edges_of(want.bits))
    small.close()
    good.close()


# ------------------------------------------------- walk from synchronising spans ----

@pytest.mark.parametrize("devname,kw", [("p3l-nexa2012", {}), ("p3l-nexa2012", dict(glitch_every=5)),
                                        ("p3l-nexa2012", dict(gap_us=(17000, 30000))), ("unknown-remote1", {}),
                                        ("unknown-remote1", dict(glitch_every=7, noise=120))])
def test_scan_walk_from_synchronising_spans(ok, oracle, devname, kw):
    """Captures with silence between the messages: the scan finds every leaf's entry state by walking from one
    synchronising span to the next (stats.scan_entry_form 1) -- messages, payloads and errors are the oracle's, and
    those of the composing kernels (OOKD_RX_SCAN_TABLES)."""
    n = 1 << 24
    d = _dev(ok, devname)
    od = _odev(oracle, devname)
    iq = ok.Synth(d, n, seed=11, sample_rate=RATE, **kw).fill_host()
    want = oracle.rx(iq, _ofir(oracle, "fs32_fs4"), 0.1, od, 8192, want_bits=False)
    res = {}
    for tables in (False, True):
        with _sync_walk_forced(not tables):
            rx = ok.Receiver(_flt(ok, "fs32_fs4"), d, max_samples=n, scan_tables=tables)
        for _ in range(2):              # (the second run of a context: stamps, counters and tickets of the first behind it)
            got = rx.rx(iq)
        assert got.stats["fsm_path"] == 1 and got.stats["scan_entry_form"] == (2 if tables else 1), got.stats
        assert list(got.msg_samples) == list(want.msg_samples)
        assert (got.payloads == want.payloads).all()
        errs, nerr = rx.errors()
        assert nerr == len(want.err_samples) and list(errs[:32]) == list(want.err_samples[:32])
        res[tables] = got
        rx.close()
    assert len(want.msg_samples) >= 20


def test_scan_walk_gives_up_and_the_scan_composes(ok, oracle):
    """Gaps too short to synchronise anything (under the longest time-out): the walk gives up -- alone in its launch
    the first time, so the run is queued again with the composing kernels; then composed for a few runs; then one
    run carries both forms and the verdict stands.  Every run decodes what the oracle does."""
    n = 1 << 25
    d = _dev(ok, "p3l-nexa2012")
    od = _odev(oracle, "p3l-nexa2012")
    iq = ok.Synth(d, n, seed=12, sample_rate=RATE, gap_us=(4000, 5500), glitch_every=0).fill_host()
    want = oracle.rx(iq, _ofir(oracle, "fs32_fs4"), 0.1, od, 8192, want_bits=False)
    with _sync_walk_forced():
        rx = ok.Receiver(_flt(ok, "fs32_fs4"), d, max_samples=n)
    for run in range(11):
        got = rx.rx(iq)
        assert got.stats["fsm_path"] == 1 and got.stats["scan_entry_form"] == 2, (run, got.stats)
        assert list(got.msg_samples) == list(want.msg_samples), run
        assert (got.payloads == want.payloads).all(), run
        assert rx.errors()[1] == len(want.err_samples), run
    rx.close()
