"""The edge cleaning rule on the host (ookd_clean_edges; include/ookiedokie_amd.h, "Edge cleaning") against its
restatement (tests/clean_contract.py), the interface, and the synthetic capture whose glitches it is for.  No GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests.clean_contract import assert_invariants, clean_of, clean_of_long, deleted_parity, deleted_sequential, info_of
from tests.helpers import edges_of, golden_path
from tests.pulse_contract import RATE, SPB, THR, hist_of
from tests.symbol_contract import frames_dict, py_chain, survey_of, table_from_pulses

import ookiedokie_amd as ok
from ookiedokie_amd import build as okbuild

INCLUDE = os.path.dirname(ok.HEADER_PATH)


@pytest.fixture(scope="session", autouse=True)
def built_lib():
    okbuild.build()
    return ok.lib()


def random_list(rng, max_edges=40, max_run=11):
    E = int(rng.integers(0, max_edges + 1))
    runs = rng.integers(1, max_run + 1, size=max(E - 1, 0))
    e = int(rng.integers(0, 9)) + np.concatenate([[0], np.cumsum(runs)])
    return e[:E].astype(np.uint64)


# ---- interface --------------------------------------------------------------------------------------------

def test_new_symbols_are_exported(built_lib):
    for name in ("ookd_clean_edges", "ookd_rx_clean_edges", "ookd_rx_get_clean_info", "ookd_rx_get_clean_edges",
                 "ookd_rx_pulse_hist_clean", "ookd_rx_symbol_survey_clean", "ookd_rx_clean_kernel_ms"):
        assert hasattr(built_lib, name), name
    for name in ("clean_edges", "clean_kernel_ms"):
        assert hasattr(ok.Receiver, name), name
    assert hasattr(ok, "clean_edges") and hasattr(ok, "CleanInfo")
    assert built_lib.ookd_rx_clean_kernel_ms(None) == 0.0
    assert built_lib.ookd_api_version() == 1


def test_null_arguments_need_no_gpu(built_lib):
    info, h, t, s = ok.CleanInfo(), ok.PulseHist(), ok.SymbolTable(), ok.SymbolSurvey()
    n = C.c_uint64(7)
    assert built_lib.ookd_clean_edges(None, 3, 2, 2, None, 0, C.byref(n)) == -1 and "NULL" in ok.last_error()
    assert built_lib.ookd_clean_edges(None, 0, 2, 2, None, 0, C.byref(n)) == 0 and n.value == 0
    assert built_lib.ookd_rx_clean_edges(None, 2, 2) == -1 and "NULL" in ok.last_error()
    assert built_lib.ookd_rx_get_clean_info(None, 0, C.byref(info)) == -1
    assert built_lib.ookd_rx_get_clean_edges(None, 0, None, 0, C.byref(n)) == -1
    assert built_lib.ookd_rx_pulse_hist_clean(None, 0, C.byref(h)) == -1 and "ookd_rx_pulse_hist_clean" in ok.last_error()
    assert built_lib.ookd_rx_symbol_survey_clean(None, 0, C.byref(t), None, C.byref(s)) == -1
    assert "ookd_rx_symbol_survey_clean" in ok.last_error()


def test_header_is_c99_and_the_layout_matches(tmp_path):
    src = tmp_path / "cl.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ookiedokie_amd.h"\n'
                   'int main(void) {\n'
                   '  ookd_clean_info info; uint64_t e[4] = {10, 20, 21, 40}, out[4], n = 0;\n'
                   '  if (ookd_rx_clean_edges(NULL, 2, 2) != OOKD_ERR_ARG || ookd_rx_get_clean_info(NULL, 0, &info) != OOKD_ERR_ARG\n'
                   '      || ookd_rx_get_clean_edges(NULL, 0, out, 4, &n) != OOKD_ERR_ARG || ookd_rx_clean_kernel_ms(NULL) != 0.0f\n'
                   '      || ookd_rx_pulse_hist_clean(NULL, 0, NULL) != OOKD_ERR_ARG\n'
                   '      || ookd_rx_symbol_survey_clean(NULL, 0, NULL, NULL, NULL) != OOKD_ERR_ARG) return 1;\n'
                   '  if (ookd_clean_edges(e, 4, 0, 5, out, 4, &n) != OOKD_OK || n != 2 || out[0] != 10 || out[1] != 40) return 2;\n'
                   '  printf("%d %zu %zu %zu %zu %zu %zu %zu %zu", ookd_api_version(), sizeof(ookd_clean_info),\n'
                   '    offsetof(ookd_clean_info, edges_in), offsetof(ookd_clean_info, edges_out), offsetof(ookd_clean_info, deleted),\n'
                   '    offsetof(ookd_clean_info, min_on), offsetof(ookd_clean_info, min_off), sizeof(ookd_rx_config),\n'
                   '    sizeof(ookd_rx_stats));\n'
                   '  return 0; }\n')
    exe = tmp_path / "cl"
    libdir = os.path.dirname(ok.LIB_PATH)
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", INCLUDE, str(src), "-o", str(exe),
                        "-L", libdir, "-lookiedokie_amd", "-Wl,-rpath," + libdir], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr)
    got = [int(x) for x in r.stdout.split()]
    K = ok.CleanInfo
    assert got == [1, C.sizeof(K), K.edges_in.offset, K.edges_out.offset, K.deleted.offset, K.min_on.offset,
                   K.min_off.offset, C.sizeof(ok.RxConfig), C.sizeof(ok.RxStats)]
    assert got[:7] == [1, 48, 0, 8, 16, 32, 40] and got[7:] == [80, 104]        # the last two: what they were before


def test_the_example_takes_the_minimums(tmp_path):
    exe = tmp_path / "ookd_pulses"
    libdir = os.path.dirname(ok.LIB_PATH)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", INCLUDE, os.path.join(root, "examples", "ookd_pulses.c"),
                        "-o", str(exe), "-L", libdir, "-lookiedokie_amd", "-Wl,-rpath," + libdir],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode != 0 and "--min-on-us" in r.stderr and "--min-off-us" in r.stderr
    r = subprocess.run([str(exe), "x.sc16q11", "none", "--min-on-us"], capture_output=True, text=True)
    assert r.returncode != 0 and "usage" in r.stderr


# ---- the rule ---------------------------------------------------------------------------------------------

def test_random_lists_against_both_forms():
    rng = np.random.default_rng(2012)
    seen_deleted = 0
    for _ in range(4000):
        e = random_list(rng)
        mn, mf = (int(x) for x in rng.integers(0, 9, size=2))
        assert deleted_sequential(e, mn, mf) == deleted_parity(e, mn, mf), (e.tolist(), mn, mf)
        want, deleted = clean_of(e, mn, mf)
        assert clean_of(e, mn, mf, "parity")[0].tolist() == want.tolist()
        long_form = clean_of_long(e, mn, mf)
        assert long_form[0].tolist() == want.tolist() and long_form[1] == deleted
        got = ok.clean_edges(e, mn, mf)
        assert got.dtype == np.uint64 and got.tolist() == want.tolist(), (e.tolist(), mn, mf)
        assert_invariants(e, got, mn, mf)
        assert (e.size - got.size) == 2 * sum(deleted)
        if got.size:
            assert got.size % 2 == e.size % 2
        seen_deleted += sum(deleted)
    assert seen_deleted > 4000


def test_the_comparison_is_strict():
    e = np.array([100, 105, 112, 117, 300], dtype=np.uint64)            # on 5, off 7, on 5, off 183
    assert ok.clean_edges(e, 5, 7).tolist() == e.tolist()               # L == min stays
    assert ok.clean_edges(e, 6, 7).tolist() == [300]                    # both on-runs go, each with its two edges
    assert ok.clean_edges(e, 5, 8).tolist() == [100, 117, 300]          # the off-run of 7 goes, 5 + 7 + 5 is one on-run
    assert ok.clean_edges(e, 6, 8).tolist() == [300]                    # a chain of 3: runs 0 and 2 are deleted, 1 merged
    assert ok.clean_edges(e, 6, 184).tolist() == [300]                  # a chain of 4 leaves exactly its last edge
    for mn, mf in ((5, 7), (6, 7), (5, 8), (6, 8), (6, 184)):
        assert ok.clean_edges(e, mn, mf).tolist() == clean_of(e, mn, mf)[0].tolist()


@pytest.mark.parametrize("E", [0, 1, 2, 3])
def test_the_shortest_lists(E):
    e = np.array([4, 5, 6][:E], dtype=np.uint64)
    for mn, mf in ((0, 0), (1, 1), (2, 0), (0, 2), (2, 2), (1 << 63, 1 << 63)):
        got = ok.clean_edges(e, mn, mf)
        assert got.tolist() == clean_of(e, mn, mf)[0].tolist(), (E, mn, mf)
    assert ok.clean_edges(e, 2, 2).tolist() == [[], [4], [], [6]][E]
    assert ok.clean_edges(e, 0, 2).tolist() == [[], [4], [4, 5], [4]][E]


def test_minimums_that_keep_everything_and_nothing():
    rng = np.random.default_rng(7)
    for _ in range(50):
        e = random_list(rng)
        for mn, mf in ((0, 0), (0, 1), (1, 0), (1, 1)):
            assert ok.clean_edges(e, mn, mf).tolist() == e.tolist()
        # everything is short: one chain over all runs
        got = ok.clean_edges(e, 1 << 63, 1 << 63)
        assert got.tolist() == (e[-1:].tolist() if e.size % 2 else [])
        assert got.tolist() == clean_of(e, 1 << 63, 1 << 63)[0].tolist()


@pytest.mark.parametrize("E", [2, 3, 64, 65, 1000, 1001])
def test_the_alternating_list(E):
    e = np.arange(E, dtype=np.uint64) + 3
    got = ok.clean_edges(e, 2, 2)
    assert got.tolist() == ([3 + E - 1] if E % 2 else [])
    # one chain over all E - 1 runs: every even run is deleted, and the even runs are the on-runs
    assert info_of(e, 2, 2) == dict(edges_in=E, edges_out=E % 2, deleted=[0, E // 2], min_on=2, min_off=2)


def test_the_capacity_convention(built_lib):
    e = np.array([10, 20, 21, 40, 50, 51, 52, 90], dtype=np.uint64)
    want = clean_of(e, 2, 5)[0]
    assert want.tolist() == [10, 40, 52, 90]
    n = C.c_uint64(0)
    assert built_lib.ookd_clean_edges(e.ctypes.data, e.size, 2, 5, None, 0, C.byref(n)) == 0 and n.value == 4
    out = np.full(8, 77, dtype=np.uint64)
    assert built_lib.ookd_clean_edges(e.ctypes.data, e.size, 2, 5, out.ctypes.data, 2, C.byref(n)) == 0
    assert n.value == 4 and out.tolist() == [10, 40, 77, 77, 77, 77, 77, 77]
    assert built_lib.ookd_clean_edges(e.ctypes.data, e.size, 2, 5, out.ctypes.data, 8, None) == 0
    assert out.tolist() == [10, 40, 52, 90, 77, 77, 77, 77]


# ---- the synthetic capture --------------------------------------------------------------------------------

def lib_chain(edges, n_out, rate):
    """the library's host rules on the restatement's surveys: (suggestion, coding, survey with roles)"""
    sug = ok.suggest_pulses(hist_of(edges, n_out), rate)
    table = ok.symbol_table_from_pulses(sug)
    assert table == table_from_pulses(sug)
    coding = ok.suggest_coding(sug, survey_of(edges, table))
    survey = survey_of(edges, table, coding["roles"])
    return ok.suggest_device(sug, survey, coding, rate), coding, survey


@pytest.mark.parametrize("filt", ["fs32_fs4", "fs128_fs16_dec4"])
def test_synthetic_capture_loses_its_glitches(oracle, filt):
    """2^24 samples at 3 Msps, seed 5, p3l-nexa2012 with pauses of 4 .. 20 ms, a glitch in every eighth message.  The
    noise is keyed by (seed, sample index) and a glitch only inserts an on-run of 100 us 1 ms before a message, so with
    min_on = 250 us the cleaned list of the glitched capture is the list of the capture without glitches, element for
    element, and the host chain on it gives the unglitched answer: 26 clean modal frames of 37 counted."""
    fir = oracle.load_filter_json(golden_path("filters", filt))
    rate = RATE // fir.total_decimation
    min_on = int(250e-6 * rate)
    assert min_on == {"fs32_fs4": 750, "fs128_fs16_dec4": 187}[filt]
    d = ok.Device.load(golden_path("devices", "p3l-nexa2012"), RATE)
    lists = {}
    for glitch_every in (0, 8):
        syn = ok.Synth(d, 1 << 24, seed=5, sample_rate=RATE, gap_us=(4000, 20000), glitch_every=glitch_every)
        iq = syn.fill_host()
        syn.close()
        r = oracle.rx(iq, fir, THR, None, SPB, want_bits=True)
        lists[glitch_every] = (edges_of(r.bits).astype(np.uint64), r.decimated)
    d.close()
    (plain, n_out), (glitched, n_glitched) = lists[0], lists[8]
    assert n_out == n_glitched and glitched.size > plain.size
    cleaned = ok.clean_edges(glitched, min_on, 0)
    print(filt, "edges", plain.size, "glitched", glitched.size, "cleaned", cleaned.size)
    assert cleaned.tolist() == clean_of(glitched, min_on, 0)[0].tolist()
    assert cleaned.tolist() == plain.tolist()
    assert ok.clean_edges(plain, min_on, 0).tolist() == plain.tolist()          # nothing of the capture itself is short
    assert_invariants(glitched, cleaned, min_on, 0)
    got = lib_chain(cleaned, n_out, rate)
    want = py_chain(plain, n_out, rate)
    for key, value in want[0].items():
        assert got[0][key] == value, (key, got[0], want[0])
    s = got[0]
    assert s["found"] == 1 and s["num_bits"] == 36
    assert (s["frames_seen"], s["frames_counted"], s["frames_clean"]) == (48, 37, 26)
    assert frames_dict(got[2], 1)[38] == 26 and frames_dict(got[2], 0) == {}
    # and without cleaning the glitched capture is what tests/test_symbols_host.py pins: 22 clean frames, {39: 4} not
    raw = lib_chain(glitched, n_out, rate)
    assert raw[0]["frames_clean"] == 22 and frames_dict(raw[2], 0) == {39: 4}
