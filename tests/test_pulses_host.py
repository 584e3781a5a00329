"""CPU-side tests of the pulse survey: the new symbols, constants and layouts, the bin rule against its Python
restatement, the numpy restatement of the contract (tests/pulse_contract.py) on the oracle's bits of the golden
captures -- which has to give the run lengths the feature was specified with --, and ookd_suggest_pulses on those
histograms and on hand-made ones.

test_contract_gives_the_specified_run_lengths and test_hist_of_restates_the_contract first of all validate the
REFERENCE the GPU tests compare against (tests/pulse_contract.py over the oracle's bits) against the table the
feature was specified with; beside that they hold the library's ookd_pulse_bin and ookd_suggest_pulses to the same
histograms, so they too need the feature."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

from tests.helpers import golden_path
from tests.pulse_contract import (BINS, CLASS_GAP, MAX_CLASSES, RATE, TABLE, assert_same_suggestion, golden_iq, hist_of,
                                  np_bins, oracle_edges, py_bin, py_bin_lower, py_suggest, runs_of)

import ookiedokie_amd as ok
from ookiedokie_amd import build as okbuild

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.dirname(ok.HEADER_PATH)


@pytest.fixture(scope="session", autouse=True)
def built_lib():
    okbuild.build()
    return ok.lib()


@pytest.fixture(scope="module")
def golden_hists(oracle, vectors):
    """{(capture, filter, noisy): histogram} by the numpy restatement over the oracle's bits (computed once)"""
    out = {}
    for (name, filt) in TABLE:
        for noisy in (False, True):
            e, n_out = oracle_edges(oracle, golden_iq(vectors, name, 5 if noisy else None), filt)
            h = hist_of(e, n_out)
            for a in (h["count"], h["sum"], h["runs"]):
                a.setflags(write=False)
            out[(name, filt, noisy)] = h
    return out


def _hist(on=None, off=None):
    """a histogram holding the given runs: {length: count} per level"""
    count = np.zeros((2, BINS), dtype=np.uint64)
    total = np.zeros((2, BINS), dtype=np.uint64)
    for lv, runs in ((1, on or {}), (0, off or {})):
        for d, c in runs.items():
            count[lv, py_bin(d)] += np.uint64(c)
            total[lv, py_bin(d)] += np.uint64(c * d)
    return dict(count=count, sum=total)


def _decimation(oracle, filt):
    return oracle.load_filter_json(golden_path("filters", filt)).total_decimation


# ---- interface --------------------------------------------------------------------------------------------

def test_new_symbols_are_exported(built_lib):
    for name in ("ookd_rx_pulse_hist", "ookd_rx_pulse_kernel_ms", "ookd_pulse_bin", "ookd_pulse_bin_lower",
                 "ookd_suggest_pulses"):
        assert hasattr(built_lib, name), name
    for name in ("pulse_bin", "pulse_bin_lower", "suggest_pulses", "PULSE_BINS", "PULSE_CLASS_GAP", "PULSE_MAX_CLASSES"):
        assert hasattr(ok, name), name
    assert hasattr(ok.Receiver, "pulse_hist") and hasattr(ok.Receiver, "pulse_kernel_ms")
    assert built_lib.ookd_rx_pulse_kernel_ms(None) == 0.0


def test_null_arguments_need_no_gpu(built_lib):
    h = ok.PulseHist()
    assert built_lib.ookd_rx_pulse_hist(None, 0, C.byref(h)) == -1 and "NULL" in ok.last_error()
    assert built_lib.ookd_rx_pulse_hist(None, 0, None) == -1
    s = ok.PulseSuggestion()
    assert built_lib.ookd_suggest_pulses(None, 1.0, C.byref(s)) == -1 and "NULL" in ok.last_error()
    assert built_lib.ookd_suggest_pulses(C.byref(h), 1.0, None) == -1
    assert built_lib.ookd_suggest_pulses(None, 1.0, None) == -1


def test_header_is_c99_and_the_layouts_match(tmp_path):
    src = tmp_path / "pl.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ookiedokie_amd.h"\n'
                   'int main(void) {\n'
                   '  ookd_pulse_hist *h = NULL; ookd_pulse_suggestion *s = NULL;\n'
                   '  if (ookd_rx_pulse_hist(NULL, 0, NULL) != OOKD_ERR_ARG || ookd_suggest_pulses(h, 0.0, s) != OOKD_ERR_ARG\n'
                   '      || ookd_rx_pulse_kernel_ms(NULL) != 0.0f || ookd_pulse_bin(1503) != 119\n'
                   '      || ookd_pulse_bin_lower(119) != 1472) return 1;\n'
                   '  printf("%d %d %d %d %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu", OOKD_PULSE_BINS, OOKD_PULSE_CLASS_GAP,\n'
                   '    OOKD_PULSE_MAX_CLASSES, ookd_api_version(), sizeof(ookd_pulse_hist), offsetof(ookd_pulse_hist, count),\n'
                   '    offsetof(ookd_pulse_hist, sum), offsetof(ookd_pulse_hist, open_head), offsetof(ookd_pulse_hist, tail_level),\n'
                   '    sizeof(ookd_pulse_class), offsetof(ookd_pulse_class, mean_us), sizeof(ookd_pulse_suggestion),\n'
                   '    offsetof(ookd_pulse_suggestion, dropped_runs), offsetof(ookd_pulse_suggestion, classes),\n'
                   '    sizeof(ookd_rx_config), sizeof(ookd_rx_stats));\n'
                   '  return 0; }\n')
    exe = tmp_path / "pl"
    libdir = os.path.dirname(ok.LIB_PATH)
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", INCLUDE, str(src), "-o", str(exe),
                        "-L", libdir, "-lookiedokie_amd", "-Wl,-rpath," + libdir], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = [int(x) for x in r.stdout.split()]
    assert got[:4] == [ok.PULSE_BINS, ok.PULSE_CLASS_GAP, ok.PULSE_MAX_CLASSES, 1] == [512, 2, 16, 1]
    H, K, S = ok.PulseHist, ok.PulseClass, ok.PulseSuggestion
    assert got[4:14] == [C.sizeof(H), H.count.offset, H.sum.offset, H.open_head.offset, H.tail_level.offset,
                         C.sizeof(K), K.mean_us.offset, C.sizeof(S), S.dropped_runs.offset, S.classes.offset]
    assert got[4] == 8 * (4 + 4 * 512 + 3)
    assert got[14:] == [C.sizeof(ok.RxConfig), C.sizeof(ok.RxStats)] == [80, 104]      # what they were before


def test_the_example_builds(tmp_path):
    exe = tmp_path / "ookd_pulses"
    libdir = os.path.dirname(ok.LIB_PATH)
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", INCLUDE, os.path.join(ROOT, "examples", "ookd_pulses.c"),
                        "-o", str(exe), "-L", libdir, "-lookiedokie_amd", "-Wl,-rpath," + libdir],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode != 0 and "usage" in r.stderr
    r = subprocess.run([str(exe), "x.sc16q11", "none", "--rate"], capture_output=True, text=True)
    assert r.returncode != 0 and "usage" in r.stderr


# ---- bins -------------------------------------------------------------------------------------------------

def test_pulse_bin_is_the_formula(built_lib):
    edges = [py_bin_lower(b) for b in range(1, BINS + 1)] + [1 << k for k in range(0, 64)]
    values = {0, 1, 2, 31, 32, 33, 1503, (1 << 35) - 1, 1 << 35, (1 << 63) - 1, 1 << 63, (1 << 63) + 1, (1 << 64) - 1}
    for e in edges:
        values.update(v for v in (e - 1, e, e + 1) if 0 <= v < (1 << 64))
    rng = np.random.default_rng(7)
    values.update(int(v) >> int(s) for v, s in zip(rng.integers(0, 1 << 63, size=20000, dtype=np.uint64) * 2 + 1,
                                                   rng.integers(0, 64, size=20000)))
    values = sorted(values)
    fn = built_lib.ookd_pulse_bin
    got = [fn(v) for v in values]
    want = [py_bin(v) for v in values]
    assert got == want, [(v, g, w) for v, g, w in zip(values, got, want) if g != w][:8]
    assert np_bins(np.array(values, dtype=np.uint64)).tolist() == want
    # the documented points
    assert ok.pulse_bin(0) == 0 and ok.pulse_bin(1) == 1 and ok.pulse_bin(31) == 31 and ok.pulse_bin(32) == 32
    assert ok.pulse_bin(63) == 47 and ok.pulse_bin(64) == 48 and ok.pulse_bin(1503) == 119
    assert ok.pulse_bin((1 << 35) - 1) == 511 and ok.pulse_bin(1 << 35) == 511 and ok.pulse_bin((1 << 64) - 1) == 511
    assert ok.pulse_bin(11997) == 167 and ok.pulse_bin(13197) == 169 and ok.pulse_bin(416) == ok.pulse_bin(415) + 1


def test_bin_lower_inverts_bin():
    prev = -1
    for b in range(0, 1200):
        lo = ok.pulse_bin_lower(b)
        assert lo == py_bin_lower(b), b
        assert lo > prev or lo == (1 << 64) - 1, b              # monotone; saturates at the top
        prev = lo
        if 1 <= b < BINS:
            assert ok.pulse_bin(lo) == b and ok.pulse_bin(lo - 1) == b - 1
            # sixteen bins per octave, none wider than 1/16 of its lower edge
            assert ok.pulse_bin_lower(b + 1) - lo <= max(1, lo // 16)
    assert ok.pulse_bin_lower(32) == 32 and ok.pulse_bin_lower(119) == 1472 and ok.pulse_bin_lower(512) == 1 << 35
    assert ok.pulse_bin_lower(0xffffffff) == (1 << 64) - 1


# ---- the contract on the oracle's bits --------------------------------------------------------------------

@pytest.mark.parametrize("noisy", [False, True], ids=["clean", "noise40"])
@pytest.mark.parametrize("name,filt", sorted(TABLE))
def test_contract_gives_the_specified_run_lengths(golden_hists, name, filt, noisy):
    h = golden_hists[(name, filt, noisy)]
    edges, on, off = TABLE[(name, filt)]
    assert h["num_edges"] == edges and h["tail_level"] == 0
    assert h["runs"].tolist() == [edges // 2 - 1, edges // 2]
    for level, runs in ((1, on), (0, off)):
        want = {}
        for length, c in runs.items():
            lengths = length if isinstance(length, tuple) else (length,)
            assert len({py_bin(d) for d in lengths}) == 1 == len({ok.pulse_bin(d) for d in lengths})
            b = ok.pulse_bin(lengths[0])
            assert b == py_bin(lengths[0])
            assert b not in want
            want[b] = (c, lengths)
        got = runs_of(h, level)
        assert sorted(got) == sorted(want), (level, got, want)
        for b, (c, lengths) in want.items():
            assert got[b][0] == c
            assert c * min(lengths) <= got[b][1] <= c * max(lengths)       # every run there has one of these lengths
    # the open runs and the closed ones tile the decimated capture
    total = h["open_head"] + int(h["sum"].sum()) + h["open_tail"]
    assert total == h["samples"]
    # and the library's classes of it are the rule's
    s = ok.suggest_pulses(h, RATE)
    assert_same_suggestion(s, py_suggest(h, RATE))
    assert sum(k["runs"] for k in s["classes"][0] + s["classes"][1]) == edges - 1


def test_suggestion_on_g1_matches_the_device_file(oracle, golden_hists):
    """at 3 Msps: one on-class and three off-classes whose means fall inside the windows
    the reference's state machine gives the device file's 500, 2000, 4000 and 8700 us"""
    with open(golden_path("devices", "p3l-nexa2012")) as f:
        text = f.read()
    for us in (500, 2000, 4000, 8700):
        assert '"duration_us":  %d' % us in text
    for filt in ("fs32_fs4", "fs128_fs16_dec4"):
        rate = RATE // _decimation(oracle, filt)
        for noisy in (False, True):
            h = golden_hists[("G1", filt, noisy)]
            s = ok.suggest_pulses(h, rate)
            assert_same_suggestion(s, py_suggest(h, rate))
            assert s["found"] == 1 and s["dropped_runs"] == [0, 0]
            off, on = s["classes"]
            assert [k["runs"] for k in on] == [114] and [k["runs"] for k in off] == [60, 50, 3]
            for k, us in zip(on + off, (500, 2000, 4000, 8700)):
                kmin, kmax = oracle.duration_window(rate, us)
                assert kmin <= k["mean"] <= kmax, (k, kmin, kmax)
                assert kmin / rate * 1e6 <= k["mean_us"] <= kmax / rate * 1e6
                assert k["lower"] <= k["mean"] <= k["upper"]
                assert abs(k["mean_us"] - us) <= 0.01 * us


def test_adjacent_bins_merge_and_one_empty_bin_separates(oracle, golden_hists):
    r4, r1 = RATE / _decimation(oracle, "fs128_fs16_dec4"), RATE / _decimation(oracle, "fs32_fs4")
    for noisy in (False, True):
        h = golden_hists[("G2", "fs128_fs16_dec4", noisy)]
        s = ok.suggest_pulses(h, r4)
        assert_same_suggestion(s, py_suggest(h, r4))
        off, on = s["classes"]
        # 415 x 32 and 416 x 34 sit in adjacent bins: one class of 66 runs
        assert [k["runs"] for k in on] == [66, 2]
        assert on[0]["last_bin"] == on[0]["first_bin"] + 1 and on[0]["lower"] <= 415 < 416 <= on[0]["upper"]
        assert on[0]["mean"] == pytest.approx((415 * 32 + 416 * 34) / 66, rel=1e-12)
        h = golden_hists[("G2", "fs32_fs4", noisy)]
        s = ok.suggest_pulses(h, r1)
        assert_same_suggestion(s, py_suggest(h, r1))
        off, on = s["classes"]
        # 11997 (bin 167) and 13197 (bin 169): one empty bin between them, two classes
        assert [k["runs"] for k in off] == [34, 30, 1, 2]
        assert (off[2]["first_bin"], off[3]["first_bin"]) == (167, 169)
        assert off[2]["mean"] == 11997.0 and off[3]["mean"] == 13197.0
        assert s["found"] == 1


# ---- the rule on hand-made histograms ---------------------------------------------------------------------

def test_empty_and_one_level_only():
    s = ok.suggest_pulses(_hist(), RATE)
    assert s == dict(found=0, dropped_runs=[0, 0], classes=[[], []])
    h = _hist(on={500: 10, 1000: 7})
    s = ok.suggest_pulses(h, RATE)
    assert_same_suggestion(s, py_suggest(h, RATE))
    assert s["found"] == 0 and s["classes"][0] == [] and [k["runs"] for k in s["classes"][1]] == [10, 7]
    # both levels, but one holds single runs only
    h = _hist(on={500: 10}, off={700: 1, 9000: 1})
    assert ok.suggest_pulses(h, RATE)["found"] == 0
    h = _hist(on={500: 2}, off={700: 1, 9000: 2})
    assert ok.suggest_pulses(h, RATE)["found"] == 1
    with pytest.raises(ValueError):
        ok.suggest_pulses(dict(count=np.zeros((2, 256)), sum=np.zeros((2, 256))), RATE)


def test_class_gap():
    assert CLASS_GAP == ok.PULSE_CLASS_GAP == 2
    lo = [py_bin_lower(b) for b in range(100, 110)]
    # bins 100, 101: adjacent, fewer than 2 apart, one class; 100, 102 (one empty bin between) and 100, 103: two
    for other, classes in ((1, 1), (2, 2), (3, 2)):
        h = _hist(on={lo[0]: 5, lo[other]: 4}, off={40: 2})
        s = ok.suggest_pulses(h, 0)
        assert_same_suggestion(s, py_suggest(h, 0))
        assert len(s["classes"][1]) == classes, other
    # a chain of bins each within the gap of the next is ONE class; its range spans all of it
    h = _hist(on={lo[0]: 1, lo[1]: 1, lo[2]: 1, lo[3]: 3, lo[5]: 7}, off={40: 2})
    k, other = ok.suggest_pulses(h, 0)["classes"][1]
    assert (k["first_bin"], k["last_bin"], k["runs"]) == (100, 103, 6) and other["first_bin"] == 105
    assert (k["lower"], k["upper"]) == (lo[0], py_bin_lower(104) - 1)
    assert k["mean"] == (lo[0] + lo[1] + lo[2] + 3 * lo[3]) / 6


def test_sample_rate_zero_leaves_the_microseconds_zero():
    h = _hist(on={1503: 114}, off={5997: 60})
    for rate in (0.0, -1.0, float("nan")):
        s = ok.suggest_pulses(h, rate)
        for k in s["classes"][0] + s["classes"][1]:
            assert (k["mean_us"], k["lower_us"], k["upper_us"]) == (0.0, 0.0, 0.0) and k["mean"] > 0
    k, = ok.suggest_pulses(h, 750000.0)["classes"][1]
    assert k["mean_us"] == pytest.approx(2004.0, rel=1e-12) and k["lower_us"] == pytest.approx(1472 / 0.75, rel=1e-12)
    assert k["upper"] == 1535 and k["upper_us"] == pytest.approx(1535 / 0.75, rel=1e-12)


def test_more_than_sixteen_classes():
    """20 classes, every fourth bin from 40 on: the sixteen with the most runs stay, in ascending length; among
    classes with equally many runs the shorter ones stay; the rest is counted in dropped_runs"""
    bins = [40 + 4 * i for i in range(20)]
    runs = [9, 3, 9, 3, 9, 9, 3, 9, 9, 9, 3, 3, 9, 9, 9, 9, 9, 9, 3, 9]       # fourteen nines, six threes
    assert runs.count(9) == 14 and runs.count(3) == 6
    h = _hist(on={py_bin_lower(b): c for b, c in zip(bins, runs)}, off={py_bin_lower(b): 2 for b in bins[:MAX_CLASSES]})
    s = ok.suggest_pulses(h, RATE)
    assert_same_suggestion(s, py_suggest(h, RATE))
    on = s["classes"][1]
    threes = [b for b, c in zip(bins, runs) if c == 3]
    kept = sorted([b for b, c in zip(bins, runs) if c == 9] + threes[:2])      # the two shortest of the tied ones
    assert [k["first_bin"] for k in on] == kept and len(on) == MAX_CLASSES
    assert s["dropped_runs"] == [0, 4 * 3]
    assert len(s["classes"][0]) == MAX_CLASSES                  # exactly sixteen: nothing dropped
    assert s["found"] == 1
    # all twenty tied: the sixteen shortest
    h = _hist(on={py_bin_lower(b): 5 for b in bins}, off={99: 2})
    s = ok.suggest_pulses(h, RATE)
    assert [k["first_bin"] for k in s["classes"][1]] == bins[:MAX_CLASSES] and s["dropped_runs"] == [0, 20]
    assert_same_suggestion(s, py_suggest(h, RATE))


def test_hist_of_restates_the_contract():
    """the numpy restatement itself, on lists small enough to check by hand"""
    h = hist_of([], 100)
    assert (h["num_edges"], h["open_head"], h["open_tail"], h["tail_level"]) == (0, 100, 0, 0) and not h["count"].any()
    h = hist_of([7], 100)
    assert (h["num_edges"], h["open_head"], h["open_tail"], h["tail_level"]) == (1, 7, 93, 1) and not h["count"].any()
    h = hist_of([0, 3, 40, 41, 1000], 1000)
    assert (h["open_head"], h["open_tail"], h["tail_level"]) == (0, 0, 1)
    assert runs_of(h, 1) == {3: (1, 3), 1: (1, 1)}
    assert runs_of(h, 0) == {ok.pulse_bin(37): (1, 37), ok.pulse_bin(959): (1, 959)}
    off, on = ok.suggest_pulses(h, 0)["classes"]
    assert [(k["first_bin"], k["runs"], k["mean"]) for k in on] == [(1, 1, 1.0), (3, 1, 3.0)]
    assert [(k["runs"], k["mean"]) for k in off] == [(1, 37.0), (1, 959.0)]
    assert h["runs"].tolist() == [2, 2]


def test_upper_is_no_bound_in_the_clamped_bin():
    h = _hist(on={(1 << 35) - 1: 1, 1 << 40: 1}, off={40: 2})
    k, = ok.suggest_pulses(h, 0)["classes"][1]
    assert (k["first_bin"], k["last_bin"], k["runs"]) == (511, 511, 2)
    assert k["upper"] == (1 << 35) - 1 < k["mean"]              # the header says so
