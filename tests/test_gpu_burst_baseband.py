"""The burst basebands on the GPU (ookd_rx_burst_baseband_*; burst_baseband_kernel in burst_baseband.hip).  The cut is an
exact function of the burst table and the capture, so every comparison is equality -- CF32 as uint32 patterns, SC16Q11
as int16 -- against the numpy restatement of the contract (tests/burst_baseband_contract.py) over `rx.edges(c)` and
the reference's -- or the tuned contract's -- complex filter output of the capture zero padded to whole buffers.  Every
device buffer is longer than the cut and filled with a sentinel that must survive.

Without a filter the pass's tile is 1024 outputs and the bursts are laid against its seams; every on sample has an I
and a Q of its own (lay_hashed), so an element stored in the wrong place shows.  The burst rule keeps two bursts at
least one output apart (a gap splits only when it is longer than pre + post), so "bursts that touch" are laid as the
nearest the rule allows: one output between them, on either side of a seam.  Behind a filter the captures are the
moments' seam captures (moved_seam).  Captures are a few thousand to about a million samples: each test takes seconds."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from tests import run_level_seams_inputs as S
from tests import run_moment_seams_inputs as M
from tests.burst_baseband_contract import (FORMATS, assert_table, baseband_cut_of, baseband_table_of, same_bits,
                                           tiles_filtered_of, total_of, turn_of)
from tests.bursts_contract import RATE, SPB, THR, bursts_of, mapped_samples, margins
from tests.helpers import golden_path
from tests.run_levels_contract import SEAM_NU, oracle_fir, padded, seam_tuned
from tests.run_moments_contract import moved_seam, oracle_y
from tests.tuned_contract import contract_rx, lib_stages

pytestmark = pytest.mark.gpu

T = S.T
SENTINEL = 0xA5
ELEMENT = {"cf32": 8, "sc16q11": 4}
SMALL = (3, 4, 10)


@pytest.fixture(scope="module")
def ok():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from ookiedokie_amd import build as okbuild
    okbuild.build()
    import ookiedokie_amd as okm
    okm.lib()
    return okm


def lib_filter(ok, shape):
    if shape == "three":
        return ok.Filter.from_stages(S.three_stages())
    return ok.Filter.load(golden_path("filters", shape))


def device_cut(rx, capture, fmt, total, extra=5, offset=0):
    """the cut into a device buffer of total + extra elements filled with the sentinel -> (the cut's bytes, the rest)"""
    import torch
    size = ELEMENT[fmt]
    buf = torch.full(((total + extra) * size + offset,), SENTINEL, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    assert rx.burst_baseband_device(capture, buf.data_ptr() + offset, total + extra, fmt) == total
    out = buf.cpu().numpy()
    assert (out[:offset] == SENTINEL).all()
    return out[offset:offset + total * size], out[offset + total * size:]


def check(rx, capture, y, n, pre, post, max_gap, clean=False, what="", formats=FORMATS):
    """capture's table and cut, in both formats, through the host call and into device memory, against the restatement
    over its own edge list; n: the capture's samples -> (baseband_info, the restatement's table, the edges)"""
    rx.bursts(pre, post, max_gap, clean)
    n_out = rx.stats()["decimated_samples"]
    D = rx.total_decimation
    e = rx.edges(capture, clean)
    bursts = bursts_of(e, n_out, D, n, pre, post, max_gap)
    table = baseband_table_of(bursts, n_out, D, n)
    info = rx.baseband_info(capture)
    assert_table(info, table, what)
    tile = info["tile_outputs"]
    assert tile >= 1 and tile & (tile - 1) == 0 and tile <= 1024, what
    assert info["tiles_total"] == -(-n_out // tile) and info["decimation"] == D, what
    total = total_of(table)
    y = np.ascontiguousarray(y, dtype=np.float32).reshape(-1, 2)
    assert y.shape[0] == n_out, (what, y.shape, n_out)
    for fmt in formats:
        want = baseband_cut_of(y, table, fmt)
        got = rx.burst_baseband(capture, fmt)
        same_bits(got, want, fmt, what)
        cut, rest = device_cut(rx, capture, fmt, total)
        assert cut.tobytes() == want.tobytes(), (what, fmt, "device")
        assert (rest == SENTINEL).all(), (what, fmt, "beyond total_outputs")
        after = rx.baseband_info(capture)
        if total:
            assert after["tiles_filtered"] == tiles_filtered_of(table, n_out, tile), (what, fmt)
            assert rx.baseband_kernel_ms > 0.0, what
        else:
            assert after["tiles_filtered"] == 0 and rx.baseband_kernel_ms == 0.0, what
    return rx.baseband_info(capture), table, e


# ----------------------------------------------------------------------------------------- 1. no filter ----

def _case(name, n, spb, runs):
    return S.Case(name, n, spb, [(a, f, a) for a, f in runs], [], 0)


# name, capture, (pre, post, max_gap), what the table must look like
NO_FILTER = [
    ("ends on tile seams", _case("seams", 5 * T - 24, 1000, [(T + 3, 2 * T - 4), (3 * T + 3, 4 * T - 4)]), SMALL,
     [(T, T), (3 * T, T)]),
    ("from output 0, pre clipped", _case("zero", 3000, 1000, [(2, 50), (1500, 1600)]), (30, 4, 40), [(0, 54), (1470, 134)]),
    ("three in a tile, one across three", _case("three", 5 * T - 24, 1000, [(100, 120), (300, 330), (600, 650), (T + 476, 3 * T + 628)]),
     SMALL, [(97, 27), (297, 37), (597, 57), (T + 473, 2 * T + 159)]),
    ("one output apart on both sides of a seam", _case("near", 3 * T - 72, 1000, [(1000, T - 4), (T + 4, 1100), (2020, 2 * T - 5), (2 * T + 3, 2100)]),
     (3, 4, 7), [(997, 27), (T + 1, 79), (2017, 30), (2 * T, 56)]),
    ("a post clipped where the capture ends", _case("end", 2 * T + 100, 1000, [(500, 520), (2 * T + 40, 2 * T + 100)]), SMALL,
     [(497, 27), (2 * T + 37, 63)]),
    ("eight tiles, bursts in two", _case("eight", 8 * T, T, [(2 * T + 100, 2 * T + 300), (5 * T + 10, 5 * T + 11), (5 * T + 900, 6 * T - 4)]),
     SMALL, [(2 * T + 97, 207), (5 * T + 7, 8), (5 * T + 897, 127)]),
]


@pytest.mark.parametrize("name,case,m,layout", NO_FILTER, ids=[c[0] for c in NO_FILTER])
def test_no_filter(ok, oracle, name, case, m, layout):
    iq = M.lay_hashed(case)
    rx = ok.Receiver(None, None, max_samples=case.n, samples_per_buffer=case.spb, threshold=THR, edge_capacity=case.n + 64)
    rx.rx(iq)
    assert rx.baseband_kernel_ms == 0.0                         # nobody has asked about this run yet
    info, table, e = check(rx, 0, oracle_y(oracle, None, padded(iq, case.spb)), case.n, *m, what=name)
    assert info["tile_outputs"] == T, "the cases are laid for tiles of 1024 outputs"
    assert [(b["first_output"], b["num_outputs"]) for b in table] == layout, name
    assert info["nu"] == 0.0 and info["turn"] == 0.0
    if name == "eight tiles, bursts in two":
        assert info["tiles_total"] == 8 and info["tiles_filtered"] == 2
    if name == "ends on tile seams":
        assert info["tiles_filtered"] == 2
    if name == "three in a tile, one across three":
        assert info["tiles_filtered"] == 4
    if name == "a post clipped where the capture ends":         # n is no multiple of the buffer: the run falls at n,
        assert case.n % case.spb and int(e[-1]) == case.n       # and the burst ends there, not at n + post
    rx.close()


def test_no_edge_launches_nothing(ok):
    n = 3000
    rx = ok.Receiver(None, None, max_samples=n, samples_per_buffer=1000, threshold=THR)
    rx.rx(np.zeros(2 * n, dtype=np.int16))
    assert rx.bursts(*SMALL)[0]["num_bursts"] == 0
    info = rx.baseband_info(0)
    assert info["num_bursts"] == 0 and info["total_outputs"] == 0 and info["tiles_total"] == 3
    for fmt in FORMATS:
        got = rx.burst_baseband(0, fmt)
        assert got.shape[0] == 0
        cut, rest = device_cut(rx, 0, fmt, 0)
        assert (rest == SENTINEL).all()
    assert rx.baseband_kernel_ms == 0.0 and rx.baseband_info(0)["tiles_filtered"] == 0
    rx.close()


GLITCHED = _case("glitched", 3 * 500 * 8 - 100, 500, [(1000, 1050), (1053, 1100), (3000, 3400), (5000, 5040), (5043, 5100), (9000, 9700)])


def test_clean_table(ok, oracle):
    iq = M.lay_hashed(GLITCHED)
    y = oracle_y(oracle, None, padded(iq, GLITCHED.spb))
    rx = ok.Receiver(None, None, max_samples=GLITCHED.n, samples_per_buffer=GLITCHED.spb, threshold=THR)
    rx.rx(iq)
    rx.clean_edges(0, 5)
    info, table, e = check(rx, 0, y, GLITCHED.n, 0, 0, 0, clean=True, what="cleaned list")
    assert e.tolist() == [1000, 1100, 3000, 3400, 5000, 5100, 9000, 9700] and info["total_outputs"] == 1300
    ms = rx.baseband_kernel_ms
    raw, raw_table, e_raw = check(rx, 0, y, GLITCHED.n, 0, 0, 0, what="raw list")
    assert e_raw.size == 12 and raw["num_bursts"] == 6 and raw["total_outputs"] == 1294
    # the cut follows the form `bursts` was last called with, and each form keeps its own pass
    rx.bursts(0, 0, 0, clean=True)
    assert rx.burst_baseband(0).shape[0] == 1300
    rx.bursts(0, 0, 0)
    assert rx.burst_baseband(0).shape[0] == 1294 and ms > 0.0
    rx.clean_edges(0, 2000)                                     # another cleaned list of the same run: a new table
    again, _, e2 = check(rx, 0, y, GLITCHED.n, 0, 0, 0, clean=True, what="cleaned again")
    assert e2.tolist() == [1000, 5100, 9000, 9700] and again["total_outputs"] == 4800
    rx.close()


# ------------------------------------------------------------------------------------ 2. behind filters ----

@pytest.mark.parametrize("which", sorted(S.FILTERED_TARGETS))
@pytest.mark.parametrize("shape", sorted(S.SHAPE_D))
def test_filtered_seams(ok, oracle, shape, which):
    """an untuned context on fs32_fs4, the two-stage D = 4 filter and the three-stage shape, the edges on tile and
    block seams, at the last output and open to it; with small margins and with the round trip's"""
    iq, n, spb, targets = moved_seam(oracle, shape, which)
    D = S.SHAPE_D[shape]
    rx = ok.Receiver(lib_filter(ok, shape), None, max_samples=n, samples_per_buffer=spb, threshold=THR)
    rx.rx(iq)
    y = oracle_y(oracle, oracle_fir(oracle, shape), padded(iq, spb))
    info, table, e = check(rx, 0, y, n, *SMALL, what="%s %s small" % (shape, which))
    assert rx.stats()["decimated_samples"] == S.FILTERED_OUT and T % info["tile_outputs"] == 0
    assert len(table) == 4
    wide, wide_table, _ = check(rx, 0, y, n, *margins(D), what="%s %s margins(D)" % (shape, which))
    assert wide["total_outputs"] > info["total_outputs"]
    rx.close()


def test_run_open_through_the_padding(ok, oracle):
    """n is no multiple of the buffer and the last run is on up to n_out, PAD outputs into the zero padding: its burst
    is clipped at m = n, not at n_out"""
    iq, n, spb = M.open_pad_capture()
    rx = ok.Receiver(lib_filter(ok, "fs32_fs4"), None, max_samples=n, samples_per_buffer=spb, threshold=THR)
    rx.rx(iq)
    info, table, e = check(rx, 0, oracle_y(oracle, oracle_fir(oracle, "fs32_fs4"), padded(iq, spb)), n, *SMALL, what="open pad")
    n_out = rx.stats()["decimated_samples"]
    assert n_out == n + M.PAD and e.size == 3 and n % spb
    assert table[-1]["first_output"] + table[-1]["num_outputs"] == n < n_out
    rx.close()


def test_narrow_tiles_and_the_grid_stride_loop(ok, oracle):
    """a tile of 4 outputs (most lanes of a pass hold nothing) and at least twice as many chunks as workgroups can be
    launched: a workgroup walks a second chunk, and the bursts of the capture's end are cut there"""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    bound, n = S.grid_stride_samples(cus, 4, captures=1)
    stages = S.narrow_stages(4)
    iq = S.grid_stride_capture(n, 1)
    y = oracle_y(oracle, oracle.make_fir(stages), iq)
    rx = ok.Receiver(ok.Filter.from_stages(stages), None, max_samples=n, threshold=S.GRID_THR)
    rx.rx(iq)
    info, table, e = check(rx, 0, y, n, *SMALL, what="grid stride", formats=("cf32",))
    assert info["tile_outputs"] == 4
    chunks = -(-info["tiles_total"] // 64)
    assert chunks >= 2 * bound and bound == cus * 8, (chunks, bound, cus)       # (at most 8 workgroups of 256 lanes a CU)
    assert len(table) == 3 and table[0]["first_output"] < 256 and table[-1]["first_output"] + table[-1]["num_outputs"] == n
    rx.close()


# --------------------------------------------------------------------------------- 3. tuned and carriers ----

@pytest.mark.parametrize("which", sorted(S.FILTERED_TARGETS))
def test_tuned_single_stage(ok, which):
    f = lib_filter(ok, "fs32_fs4")
    iq, n, spb, targets, stages = seam_tuned(f, which)
    rx = ok.Receiver(f, None, max_samples=n, samples_per_buffer=spb, threshold=THR, tune=SEAM_NU)
    rx.rx(iq)
    info, table, e = check(rx, 0, contract_rx(iq, stages, THR, spb)[1], n, *SMALL, what="tuned %s" % which)
    assert info["nu"] == SEAM_NU and info["turn"] == pytest.approx(turn_of(SEAM_NU, 1), abs=1e-15) and len(table) == 4
    rx.close()


def _moved_g1():
    from tests.spectrum_contract import moved_golden
    iq, _, g = moved_golden("G1", 600e3, seed=12)
    return iq, g


@pytest.mark.parametrize("fir2", [False, True], ids=["generic", "tuned_fir2"])
def test_tuned_two_stages(ok, fir2):
    iq, g = _moved_g1()
    n = iq.size // 2
    nu = 600e3 / RATE
    f = lib_filter(ok, "fs128_fs16_dec4")
    rx = ok.Receiver(f, None, max_samples=n, threshold=THR, tune=nu, tuned_fir2=fir2)
    rx.rx(iq)
    y = contract_rx(iq, lib_stages(f, nu), THR)[1]
    info, table, e = check(rx, 0, y, n, *margins(4), what="tuned two stages")
    assert info["decimation"] == 4 and info["nu"] == nu and info["turn"] == pytest.approx(-0.2, abs=1e-12)
    assert 1 <= len(table) and 0 < info["total_outputs"] < rx.stats()["decimated_samples"]
    rx.close()


def test_carrier_context_with_two_carriers(ok):
    """list k's cut is the cut of a context tuned to carrier k alone, byte for byte: transmitter k alone"""
    from tests.test_gpu_run_levels import _two_carriers
    iq, carriers = _two_carriers()
    n = iq.size // 2
    f = lib_filter(ok, "fs32_fs4")
    rx = ok.Receiver(f, None, max_samples=n, carriers=[carriers[0][0], carriers[1]], threshold=carriers[0][1])
    rx.rx(iq)
    m = margins(1)
    tables = []
    for k, (nu, thr) in enumerate(carriers):
        y = contract_rx(iq, lib_stages(f, nu), thr)[1]
        info, table, e = check(rx, k, y, n, *m, what="carrier %d" % k)
        assert info["nu"] == nu and info["num_bursts"] >= 1
        tables.append(table)
        one = ok.Receiver(f, None, max_samples=n, threshold=thr, tune=nu)
        one.rx(iq)
        one.bursts(*m)
        rx.bursts(*m)
        assert one.baseband_info(0)["first_output"].tolist() == info["first_output"].tolist()
        for fmt in FORMATS:
            assert one.burst_baseband(0, fmt).tobytes() == rx.burst_baseband(k, fmt).tobytes()
        one.close()
    assert tables[0] != tables[1]                               # two lists, two cuts, one capture
    with pytest.raises(ok.OokdError) as err:
        rx.burst_baseband(2)
    assert err.value.code == -1
    rx.close()


# ------------------------------------------------------------------------------------------ 4. cs8 / cu8 ----

@pytest.mark.parametrize("fmt", ["cs8", "cu8"])
def test_8bit_equals_the_widened_capture(ok, oracle, fmt):
    name, case, m, layout = NO_FILTER[2]
    v = M.lay_hashed(case, M.MIN_RAIL8, M.SPAN8)
    raw = v.astype(np.int8) if fmt == "cs8" else (v + 128).astype(np.uint8)
    wide = (v * 16).astype(np.int16)
    rx = ok.Receiver(None, None, max_samples=case.n, samples_per_buffer=case.spb, threshold=THR, sample_format=fmt)
    rx.rx(raw)
    info, table, e = check(rx, 0, oracle_y(oracle, None, padded(wide, case.spb)), case.n, *m, what=fmt)
    assert [(b["first_output"], b["num_outputs"]) for b in table] == layout
    rx.close()
    iq, n, spb, targets = moved_seam(oracle, "fs128_fs16_dec4", "a")
    v = np.clip(np.rint(iq.astype(np.float64) / 16.0), -128, 127).astype(np.int16)
    wide = (v * 16).astype(np.int16)
    raw = v.astype(np.int8) if fmt == "cs8" else (v + 128).astype(np.uint8)
    rx = ok.Receiver(lib_filter(ok, "fs128_fs16_dec4"), None, max_samples=n, samples_per_buffer=spb, threshold=THR, sample_format=fmt)
    rx.rx(raw)
    info, table, e = check(rx, 0, oracle_y(oracle, oracle_fir(oracle, "fs128_fs16_dec4"), padded(wide, spb)), n, *SMALL,
                           what="%s behind a filter" % fmt)
    assert info["num_bursts"] >= 3
    rx.close()


# -------------------------------------------------------------------------------------- 5. demonstration ----

def test_the_cut_is_transmitter_k_alone_at_a_quarter_of_the_rate(ok, tmp_path):
    """golden G1 at +600 kHz beside a DC term, through a context tuned there on fs128_fs16_dec4: the SC16Q11 cut decodes,
    without a filter at fs / 4, to the whole capture's payloads at the mapped samples; its carrier sits at `turn`; and
    examples/ookd_rx.c --baseband writes the same bytes"""
    from tests.test_host import _build_c_example
    iq, g = _moved_g1()
    n = iq.size // 2
    nu = 600e3 / RATE
    f = lib_filter(ok, "fs128_fs16_dec4")
    D = f.total_decimation
    d = ok.Device.load(golden_path("devices", g["device"]), RATE // D)
    rx = ok.Receiver(f, d, max_samples=n, threshold=THR, tune=nu, pipeline=False)
    whole = rx.rx(iq)
    assert len(whole.msg_samples) == 3 and whole.stats["num_errors"] == 0
    pre, post, max_gap = margins(D)
    rx.bursts(pre, post, max_gap)
    n_out = rx.stats()["decimated_samples"]
    bursts = bursts_of(rx.edges(0), n_out, D, n, pre, post, max_gap)
    info = rx.baseband_info(0)
    assert_table(info, baseband_table_of(bursts, n_out, D, n))
    cut = rx.burst_baseband(0, "sc16q11")
    assert 0 < cut.shape[0] == info["total_outputs"] < n_out and cut.shape[0] * 4 < n      # under a quarter of the raw bytes
    # ... decodes like the whole capture
    again_rx = ok.Receiver(None, d, max_samples=cut.shape[0], threshold=THR, pipeline=False)
    again = again_rx.rx(cut.reshape(-1))
    assert again.payloads.tolist() == whole.payloads.tolist()
    assert again.msg_samples.tolist() == mapped_samples(whole.msg_samples, bursts, D)[0]
    assert again.stats["num_errors"] == whole.stats["num_errors"]
    again_rx.close()
    # ... holds the carrier at turn = nu D - rint(nu D) = -0.2 cycles per output: bin -205 of 1024
    assert info["turn"] == pytest.approx(-0.2, abs=1e-12)
    sp = ok.Spectrum()
    frames, power = sp.spectrum(cut.reshape(-1))
    sp.close()
    assert frames >= 8
    power = np.array(power, dtype=np.float64)
    power[[0, 1, 1023]] = 0.0
    peak = int(np.argmax(power))
    want = int(np.rint(1024 * info["turn"])) % 1024
    assert want == 1024 - 205 and min((peak - want) % 1024, (want - peak) % 1024) <= 1, (peak, want)
    # ... and is what the example writes
    exe = _build_c_example(tmp_path)
    cap = tmp_path / "g1_600k.sc16q11"
    iq.tofile(str(cap))
    for fmt in FORMATS:
        path = tmp_path / ("cut." + fmt)
        r = subprocess.run([exe, "--tune", "600000", "--baseband", str(path), "--burst-pre-us", "200.5", "--burst-post-us", "18400.5",
                            "--burst-gap-us", "18601", str(cap), golden_path("devices", g["device"]),
                            golden_path("filters", "fs128_fs16_dec4"), str(RATE), "csv"], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        assert "baseband: %d outputs in %d bursts at 750000 Hz, carrier at -150000 Hz" % (info["total_outputs"], info["num_bursts"]) in r.stderr
        assert open(str(path), "rb").read() == rx.burst_baseband(0, fmt).tobytes()
        idx = [[int(x) for x in ln.split()] for ln in open(str(path) + ".idx").read().strip().split("\n")]
        assert idx == [[int(info[k][b]) for k in ("first_output", "num_outputs", "offset")] for b in range(info["num_bursts"])]
    rx.close()


# ------------------------------------------------------------------------------ 6. by-product behaviour ----

def test_by_product_behaviour(ok, oracle):
    import torch
    name, case, m, layout = NO_FILTER[2]
    iq = M.lay_hashed(case)
    rx = ok.Receiver(None, None, max_samples=case.n, samples_per_buffer=case.spb, threshold=THR)
    assert ok.lib().ookd_rx_burst_baseband_host(rx._h, 0, 0, None, 0) == -1 and "no finished run" in ok.last_error()
    with pytest.raises(ok.OokdError) as err:
        rx.burst_baseband(0)
    assert err.value.code == -1
    rx.rx(iq)
    with pytest.raises(ok.OokdError) as err:                    # the cut before the table
        rx.burst_baseband(0)
    assert err.value.code == -1 and "ookd_rx_bursts first" in str(err.value)
    with pytest.raises(ok.OokdError) as err:
        rx.baseband_info(0)
    assert err.value.code == -1 and "ookd_rx_bursts first" in str(err.value)
    before = (rx.result(), rx.edges(0), rx.stats(), rx.bits(0), rx.run_levels(0), rx.run_moments(0))
    rx.bursts(*m)
    raw_cut = rx.burst_samples(0)
    info = rx.baseband_info(0)
    assert rx.baseband_kernel_ms == 0.0 and info["tiles_filtered"] == 0        # the table alone launches nothing
    total = info["total_outputs"]
    first = rx.burst_baseband(0)
    ms = rx.baseband_kernel_ms
    assert ms > 0.0 and rx.baseband_info(0)["tiles_filtered"] == 4
    assert rx.burst_baseband(0).tobytes() == first.tobytes()    # the same call twice: the same bytes
    with pytest.raises(ok.OokdError) as err:
        rx.burst_baseband(1)
    assert err.value.code == -1 and "capture 1 of 1" in str(err.value)
    # one output short: refused, and nothing is written; so are an unknown format and a pointer off its element
    for fmt in FORMATS:
        buf = torch.full((total * ELEMENT[fmt] + 16,), SENTINEL, dtype=torch.uint8, device="cuda")
        with pytest.raises(ok.OokdError) as err:
            rx.burst_baseband_device(0, buf.data_ptr(), total - 1, fmt)
        assert err.value.code == -5 and "capacity" in str(err.value)
        with pytest.raises(ok.OokdError) as err:
            rx.burst_baseband_device(0, buf.data_ptr() + ELEMENT[fmt] // 2, total, fmt)
        assert err.value.code == -1 and "aligned" in str(err.value)
        assert ok.lib().ookd_rx_burst_baseband_device(rx._h, 0, 2, C.c_void_p(buf.data_ptr()), total) == -1 and "format" in ok.last_error()
        torch.cuda.synchronize()
        assert (buf.cpu().numpy() == SENTINEL).all()
        cut, rest = device_cut(rx, 0, fmt, total, offset=ELEMENT[fmt])      # aligned to the element and no further
        assert cut.tobytes() == rx.burst_baseband(0, fmt).tobytes() and (rest == SENTINEL).all()
    # the run, the raw cut and the other by-products are what they were
    after = (rx.result(), rx.edges(0), rx.stats(), rx.bits(0), rx.run_levels(0), rx.run_moments(0))
    assert after[1].tolist() == before[1].tolist() and after[2] == before[2] and np.array_equal(after[3], before[3])
    assert after[0].msg_samples.tolist() == before[0].msg_samples.tolist()
    assert after[4]["peaks"].tolist() == before[4]["peaks"].tolist() and after[5]["power"].tolist() == before[5]["power"].tolist()
    assert rx.burst_samples(0).tobytes() == raw_cut.tobytes()
    # a new run nobody has made a table of is refused, and costs nothing
    rx.rx(iq)
    assert rx.baseband_kernel_ms == 0.0
    with pytest.raises(ok.OokdError) as err:
        rx.burst_baseband(0)
    assert err.value.code == -1 and "ookd_rx_bursts first" in str(err.value)
    rx.bursts(*m)
    assert rx.burst_baseband(0).tobytes() == first.tobytes()
    rx.close()


def test_refusals_of_the_run_and_of_the_filter(ok):
    import torch
    n = 2 * SPB
    iq = np.zeros(2 * n, dtype=np.int16)
    iq[0::2] = 2000
    rx = ok.Receiver(None, None, max_samples=n, threshold=THR)
    dev_t = torch.from_numpy(iq).cuda()
    rx.rx_device(dev_t.data_ptr(), n)
    rx.bursts(*SMALL)
    assert rx.burst_baseband(0).shape[0] == n                    # on throughout: one open run, the whole capture
    rx.shard_begin(dev_t.data_ptr(), n, None, True, None)       # a shard run has no table, and could not make one
    with pytest.raises(ok.OokdError) as err:
        rx.burst_baseband(0)
    assert err.value.code == -1
    rx.close()
    long_taps = np.full(11000, 1.0 / 11000.0, dtype=np.float32)   # a filter the pass's LDS window cannot hold
    rx = ok.Receiver(ok.Filter.from_stages([(1, long_taps)]), None, max_samples=n, threshold=THR)
    rx.rx(iq)
    assert rx.bursts(*SMALL)[0]["num_bursts"] == 1
    with pytest.raises(ok.OokdError) as err:
        rx.burst_baseband(0)
    assert err.value.code == -1 and "does not fit the kernel's LDS window" in str(err.value)
    with pytest.raises(ok.OokdError) as err:
        rx.baseband_info(0)
    assert err.value.code == -1 and "does not fit the kernel's LDS window" in str(err.value)
    assert rx.baseband_kernel_ms == 0.0
    rx.close()
