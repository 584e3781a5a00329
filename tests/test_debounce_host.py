"""The debounced decode without a GPU: the restatement (tests/debounce_contract.py) on the synthetic capture whose
glitches cost messages, the interface, the header and the example.  The reference everywhere is the CPU oracle's state
machine on the bit stream painted from the cleaned edge list."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests.debounce_contract import cleaned, decode_cleaned, paint
from tests.debounce_inputs import FULL, GRID, PART, glitched_burst_runs
from tests import dense_devices as dd
from tests.helpers import edges_of, golden_path, stream_from_runs
from tests.pulse_contract import RATE, SPB, THR

import ookiedokie_amd as ok
from ookiedokie_amd import build as okbuild

INCLUDE = os.path.dirname(ok.HEADER_PATH)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="session", autouse=True)
def built_lib():
    okbuild.build()
    return ok.lib()


# ---- the restatement itself -------------------------------------------------------------------------------

def test_paint_inverts_edges_of():
    rng = np.random.default_rng(2)
    for n in (0, 1, 2, 63, 64, 65, 1000):
        bits = (rng.random(n) < 0.3).astype(np.uint8)
        e = edges_of(bits)
        assert paint(e, n).tolist() == bits.tolist()
    assert paint([], 5).tolist() == [0] * 5
    assert paint([0], 3).tolist() == [1, 1, 1]
    assert paint([2, 4], 6).tolist() == [0, 0, 1, 1, 0, 0]
    assert paint([2, 9], 6).tolist() == [0, 0, 1, 1, 1, 1]            # an edge at or beyond n_out paints nothing


def test_minimums_up_to_one_keep_the_list():
    e = np.array([3, 4, 5, 9, 10, 40], dtype=np.uint64)
    for mins in ((0, 0), (1, 0), (0, 1), (1, 1)):
        assert cleaned(e, mins).tolist() == e.tolist()
    assert cleaned(e, (2, 0)).tolist() == [5, 9, 10, 40]                # the pulse 3..4 goes with its two edges
    assert cleaned(e, (2, 2)).tolist() == [5, 40]                       # ... and so does the gap 9..10
    assert paint(cleaned(e, (2, 2)), 12).tolist() == [0] * 5 + [1] * 7


# ---- the designed stream ----------------------------------------------------------------------------------

def test_designed_stream_is_what_it_says(oracle):
    runs, plain = glitched_burst_runs()
    s, p = stream_from_runs(runs), stream_from_runs(plain)
    e, ep = edges_of(s).astype(np.uint64), edges_of(p).astype(np.uint64)
    assert s.size == p.size and e.size > ep.size + 100
    assert cleaned(e, FULL).tolist() == ep.tolist()
    kept = cleaned(e, PART)
    assert ep.size < kept.size < e.size
    length = np.diff(e.astype(np.int64))
    assert {1, 2, 7} <= set(length[0::2].tolist()) and {1, 2} <= set(length[1::2].tolist())
    # the two stretches on the segment grid
    on7 = [int(a) for a, b in zip(e[0::2], e[1::2]) if b - a == 7 and a % GRID == GRID - 3]
    off2 = [int(a) for a, b in zip(e[1::2], e[2::2]) if b - a == 2 and a % GRID == GRID - 1]
    assert len(on7) >= 6 and len(off2) >= 6
    painted = paint(cleaned(e, FULL), s.size)
    assert all(s[a + 2] == 1 and painted[a + 2] == 0 for a in on7[-6:])            # the sample in front of a segment
    assert all(s[a] == 0 and painted[a] == 1 for a in off2[-6:])
    # the decodes differ: at FULL the unglitched stream's, at PART and raw the glitches cost messages or errors
    fsm = dd.fsm_desc(oracle, dd.burst(8))
    want = oracle.rx(dd.iq_of(plain), None, dd.THR, fsm, GRID)
    seen = {}
    for mins in (FULL, PART, (0, 0)):
        m, pay, errs = decode_cleaned(fsm, e, s.size, mins, GRID)
        seen[mins] = (m.tolist(), errs.tolist())
        print("designed stream", mins, len(m), "messages", len(errs), "errors")
    assert seen[FULL] == (want.msg_samples.tolist(), want.err_samples.tolist()) and len(seen[FULL][0]) == 40
    assert seen[PART] != seen[FULL] and seen[(0, 0)] != seen[PART]


# ---- the synthetic capture --------------------------------------------------------------------------------

@pytest.mark.parametrize("filt", ["fs32_fs4", "fs128_fs16_dec4"])
def test_synthetic_capture_keeps_its_messages(oracle, filt):
    """2^24 samples at 3 Msps, seed 5, p3l-nexa2012 with pauses of 4 .. 20 ms, a 100 us pulse 1 ms ahead of every
    eighth message.  Raw, the reference decodes 34 messages and reports 60 errors (the pulse raises an error and the
    rest of that buffer is dropped); on the cleaned list (min_on = 250 us) it decodes what it decodes on the capture
    without glitches: 37 messages at the same samples with the same payloads, no error."""
    fir = oracle.load_filter_json(golden_path("filters", filt))
    rate = RATE // fir.total_decimation
    buf_len = SPB // fir.total_decimation
    min_on = int(250e-6 * rate)
    fsm = oracle.load_device_json(golden_path("devices", "p3l-nexa2012"), rate)[0]
    d = ok.Device.load(golden_path("devices", "p3l-nexa2012"), RATE)
    seen = {}
    for glitch_every in (0, 8):
        syn = ok.Synth(d, 1 << 24, seed=5, sample_rate=RATE, gap_us=(4000, 20000), glitch_every=glitch_every)
        iq = syn.fill_host()
        syn.close()
        seen[glitch_every] = oracle.rx(iq, fir, THR, fsm, SPB, want_bits=True)
    d.close()
    plain, raw = seen[0], seen[8]
    print(filt, "plain", len(plain.msg_samples), len(plain.err_samples), "raw", len(raw.msg_samples), len(raw.err_samples))
    assert (len(plain.msg_samples), len(plain.err_samples)) == (37, 0)
    assert (len(raw.msg_samples), len(raw.err_samples)) == (34, 60)
    e, n_out = edges_of(raw.bits).astype(np.uint64), raw.decimated
    for mins in ((min_on, 0), (min_on, min_on)):
        m, p, errs = decode_cleaned(fsm, e, n_out, mins, buf_len)
        assert (len(m), len(errs)) == (37, 0), mins
        assert m.tolist() == plain.msg_samples.tolist() and (p == plain.payloads).all(), mins
    # minimums <= 1: the raw decode, and the restatement agrees with the whole reference path on it
    for mins in ((0, 0), (1, 1)):
        m, p, errs = decode_cleaned(fsm, e, n_out, mins, buf_len)
        assert m.tolist() == raw.msg_samples.tolist() and (p == raw.payloads).all(), mins
        assert errs.tolist() == raw.err_samples.tolist(), mins


# ---- interface --------------------------------------------------------------------------------------------

def test_new_symbols_are_exported(built_lib):
    for name in ("ookd_rx_set_debounce", "ookd_rx_get_debounce"):
        assert hasattr(built_lib, name), name
    for name in ("set_debounce", "debounce"):
        assert hasattr(ok.Receiver, name), name
    assert built_lib.ookd_api_version() == 1


def test_null_arguments_need_no_gpu(built_lib):
    a, b = C.c_uint64(7), C.c_uint64(7)
    assert built_lib.ookd_rx_set_debounce(None, 750, 0) == -1 and "ookd_rx_set_debounce" in ok.last_error()
    assert "NULL" in ok.last_error()
    assert built_lib.ookd_rx_set_debounce(None, 0, 0) == -1
    assert built_lib.ookd_rx_get_debounce(None, C.byref(a), C.byref(b)) == -1 and "ookd_rx_get_debounce" in ok.last_error()
    assert (a.value, b.value) == (7, 7)


def test_header_is_c99(tmp_path):
    src = tmp_path / "db.c"
    src.write_text('#include <stdio.h>\n#include "ookiedokie_amd.h"\n'
                   'int main(void) {\n'
                   '  uint64_t on = 5, off = 6;\n'
                   '  if (ookd_rx_set_debounce(NULL, 750, 0) != OOKD_ERR_ARG) return 1;\n'
                   '  if (ookd_rx_get_debounce(NULL, &on, &off) != OOKD_ERR_ARG || on != 5 || off != 6) return 2;\n'
                   '  printf("%d %zu %zu", ookd_api_version(), sizeof(ookd_rx_config), sizeof(ookd_rx_stats));\n'
                   '  return 0; }\n')
    exe = tmp_path / "db"
    libdir = os.path.dirname(ok.LIB_PATH)
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", INCLUDE, str(src), "-o", str(exe),
                        "-L", libdir, "-lookiedokie_amd", "-Wl,-rpath," + libdir], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr)
    # the configuration and the statistics are what they were: the debounce is a call, not a field
    assert [int(x) for x in r.stdout.split()] == [1, C.sizeof(ok.RxConfig), C.sizeof(ok.RxStats)] == [1, 80, 104]


def test_the_example_takes_the_minimums(tmp_path):
    exe = tmp_path / "ookd_rx"
    libdir = os.path.dirname(ok.LIB_PATH)
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", INCLUDE, os.path.join(ROOT, "examples", "ookd_rx.c"),
                        "-o", str(exe), "-L", libdir, "-lookiedokie_amd", "-Wl,-rpath," + libdir],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode != 0 and "--min-on-us" in r.stderr and "--min-off-us" in r.stderr
    for bad in (["--min-on-us"], ["--min-off-us", "x"], ["--min-on-us", "-3"]):
        r = subprocess.run([str(exe), "x.sc16q11", "d.json", "none", "3000000"] + bad, capture_output=True, text=True)
        assert r.returncode != 0 and "usage" in r.stderr, bad
