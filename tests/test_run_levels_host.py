"""CPU-side tests of the pulse levels: the new symbols and layouts, ookd_message_levels against its Python restatement
(tests/run_levels_contract.py), and the two-transmitter scenario the feature was specified with on the oracle alone
-- which pins that the margins the GPU test asks for hold for the reference before the GPU is asked."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests.helpers import edges_of, golden_path
from tests.run_levels_contract import (RATE, SPB, THR, message_levels_of, nominal_power, padded, peaks_of, runs_of,
                                       tiles_filtered_of, two_level_capture)
from tests.test_survey_host import oracle_power

import ookiedokie_amd as ok
from ookiedokie_amd import build as okbuild

INCLUDE = os.path.dirname(ok.HEADER_PATH)
FILTERS = ("fs32_fs4", "fs128_fs16_dec4")


@pytest.fixture(scope="session", autouse=True)
def built_lib():
    okbuild.build()
    return ok.lib()


# ---- interface --------------------------------------------------------------------------------------------

def test_new_symbols_are_exported(built_lib):
    for name in ("ookd_rx_run_levels", "ookd_rx_run_levels_clean", "ookd_rx_get_run_peaks", "ookd_rx_get_run_peaks_clean",
                 "ookd_rx_levels_kernel_ms", "ookd_message_levels"):
        assert hasattr(built_lib, name), name
    assert hasattr(ok, "message_levels") and hasattr(ok, "RunLevels")
    for name in ("run_levels", "message_levels", "levels_kernel_ms"):
        assert hasattr(ok.Receiver, name), name
    assert built_lib.ookd_rx_levels_kernel_ms(None) == 0.0


def test_null_arguments_need_no_gpu(built_lib):
    out = ok.RunLevels()
    n = C.c_uint64(7)
    for fn in (built_lib.ookd_rx_run_levels, built_lib.ookd_rx_run_levels_clean):
        assert fn(None, 0, C.byref(out)) == -1 and "NULL" in ok.last_error()
        assert fn(None, 0, None) == -1
    for fn in (built_lib.ookd_rx_get_run_peaks, built_lib.ookd_rx_get_run_peaks_clean):
        assert fn(None, 0, None, 0, C.byref(n)) == -1 and "NULL" in ok.last_error()
    e = np.array([1, 5], dtype=np.uint64)
    p = np.array([1.0], dtype=np.float32)
    m = np.array([9], dtype=np.uint64)
    lv = np.zeros(1, dtype=np.float32)
    f = built_lib.ookd_message_levels
    assert f(None, 2, p.ctypes.data, 1, m.ctypes.data, 1, 1, lv.ctypes.data) == -1 and "NULL" in ok.last_error()
    assert f(e.ctypes.data, 2, None, 1, m.ctypes.data, 1, 1, lv.ctypes.data) == -1
    assert f(e.ctypes.data, 2, p.ctypes.data, 1, None, 1, 1, lv.ctypes.data) == -1
    assert f(e.ctypes.data, 2, p.ctypes.data, 1, m.ctypes.data, 1, 1, None) == -1
    assert f(e.ctypes.data, 2, p.ctypes.data, 1, m.ctypes.data, 1, 1, lv.ctypes.data) == 0 and lv[0] == 1.0


def test_header_is_c99_and_the_layouts_match(tmp_path):
    src = tmp_path / "rl.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ookiedokie_amd.h"\n'
                   'int main(void) {\n'
                   '  float lv = 0.0f;\n'
                   '  if (ookd_rx_run_levels(NULL, 0, NULL) != OOKD_ERR_ARG || ookd_rx_run_levels_clean(NULL, 0, NULL) != OOKD_ERR_ARG\n'
                   '      || ookd_rx_get_run_peaks(NULL, 0, NULL, 0, NULL) != OOKD_ERR_ARG\n'
                   '      || ookd_rx_get_run_peaks_clean(NULL, 0, NULL, 0, NULL) != OOKD_ERR_ARG\n'
                   '      || ookd_rx_levels_kernel_ms(NULL) != 0.0f\n'
                   '      || ookd_message_levels(NULL, 0, NULL, 0, NULL, 0, 0, &lv) != OOKD_ERR_ARG\n'
                   '      || ookd_message_levels(NULL, 0, NULL, 0, NULL, 0, 1, &lv) != OOKD_OK) return 1;\n'
                   '  printf("%d %d %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu", OOKD_API_VERSION, ookd_api_version(),\n'
                   '    sizeof(ookd_run_levels), offsetof(ookd_run_levels, num_runs), offsetof(ookd_run_levels, tiles_total),\n'
                   '    offsetof(ookd_run_levels, tiles_filtered), offsetof(ookd_run_levels, tile_outputs),\n'
                   '    offsetof(ookd_run_levels, reserved), offsetof(ookd_run_levels, hist),\n'
                   '    sizeof(ookd_rx_config), sizeof(ookd_rx_stats), sizeof(ookd_front_info), sizeof(ookd_message));\n'
                   '  return 0; }\n')
    exe = tmp_path / "rl"
    libdir = os.path.dirname(ok.LIB_PATH)
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", INCLUDE, str(src), "-o", str(exe),
                        "-L", libdir, "-lookiedokie_amd", "-Wl,-rpath," + libdir], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = [int(x) for x in r.stdout.split()]
    L = ok.RunLevels
    assert got[:2] == [1, 1]
    assert got[2:9] == [C.sizeof(L), L.num_runs.offset, L.tiles_total.offset, L.tiles_filtered.offset, L.tile_outputs.offset,
                        L.reserved.offset, L.hist.offset] == [32 + 8 * 257, 0, 8, 16, 24, 28, 32]
    # what they were before
    assert got[9:] == [C.sizeof(ok.RxConfig), C.sizeof(ok.RxStats), C.sizeof(ok.FrontInfo), C.sizeof(ok.Message)]
    assert got[9:11] == [80, 104] and got[12] == 48


# ---- ookd_message_levels ----------------------------------------------------------------------------------

def _check_levels(edges, peaks, msgs, pulses):
    got = ok.message_levels(edges, peaks, msgs, pulses)
    want = message_levels_of(edges, peaks, msgs, pulses)
    assert got.dtype == np.float32 and got.tolist() == want.tolist(), (edges, peaks, msgs, pulses, got, want)
    return got


def test_message_levels_on_random_lists():
    rng = np.random.default_rng(4)
    for trial in range(200):
        E = int(rng.integers(0, 60))
        edges = np.sort(rng.choice(2000, size=E, replace=False)).astype(np.uint64)
        peaks = rng.random((E + 1) // 2).astype(np.float32)
        if trial % 3 == 0 and peaks.size > 2:
            peaks[1] = peaks[0]                                   # ties
        M = int(rng.integers(0, 8))
        msgs = np.sort(rng.integers(0, 2100, size=M)).astype(np.uint64)     # (equal samples occur: the later one is empty)
        _check_levels(edges, peaks, msgs, int(rng.integers(1, 12)))


def test_message_levels_corner_cases():
    e = np.array([0, 4, 10, 14, 20, 24, 30, 34, 40], dtype=np.uint64)       # E odd: the last run is open
    p = np.array([5.0, 1.0, 4.0, 2.0, 3.0], dtype=np.float32)
    assert _check_levels(e, p, [], 3).size == 0                             # M = 0
    assert _check_levels(e, p, [0], 3).tolist() == [5.0]                    # a message at output 0 takes the run that rises there
    assert _check_levels(e, p, [25, 26, 45], 9).tolist() == [4.0, 0.0, 2.0]  # a message with no run; fewer runs than pulses
    assert _check_levels(e, p, [45], 2).tolist() == [2.0]                   # the last two: {2, 3}, lower median
    assert _check_levels(e, p, [45], 1).tolist() == [3.0]
    assert _check_levels(e, p, [45], 5).tolist() == [3.0]
    assert _check_levels(e, p, [45], 4).tolist() == [2.0]                   # {1, 4, 2, 3}: element 1 of the sorted four
    assert _check_levels([], [], [7, 9], 1).tolist() == [0.0, 0.0]          # no edges at all
    with pytest.raises(ok.OokdError) as err:
        ok.message_levels(e, p, [30, 20], 3)
    assert err.value.code == -1 and "ascend" in str(err.value)
    with pytest.raises(ok.OokdError) as err:
        ok.message_levels(e, p, [20, 30], 0)
    assert err.value.code == -1 and "pulses" in str(err.value)
    with pytest.raises(ok.OokdError) as err:
        ok.message_levels(e, p[:4], [20, 30], 1)                            # R != ceil(E / 2)
    assert err.value.code == -1


def test_the_restatement_itself():
    e = [3, 5, 2048, 2050, 4000]
    power = np.arange(8192, dtype=np.float32)
    assert runs_of(e, 8192) == [(3, 5), (2048, 2050), (4000, 8192)]
    assert peaks_of(power, e, 8192).tolist() == [4.0, 2049.0, 8191.0]
    assert tiles_filtered_of(e, 8192, 1024) == 1 + 1 + 5 and tiles_filtered_of([], 8192, 1024) == 0
    assert tiles_filtered_of([1023, 1024], 8192, 1024) == 1 and tiles_filtered_of([1023, 1025], 8192, 1024) == 2
    assert tiles_filtered_of([0], 8192, 512) == 16


# ---- the two-level scenario on the oracle -----------------------------------------------------------------

@pytest.mark.parametrize("filt", FILTERS)
def test_two_transmitters_separate_on_the_reference(oracle, vectors, filt):
    g, iq, half = two_level_capture(vectors)
    fir = oracle.load_filter_json(golden_path("filters", filt))
    dec = fir.total_decimation
    odev, _ = oracle.load_device_json(golden_path("devices", g["device"]), RATE // dec)
    r = oracle.rx(iq, fir, THR, odev, SPB, want_bits=True)
    assert len(r.msg_samples) == 6 and len(r.err_samples) == 0
    edges = edges_of(r.bits).astype(np.uint64)
    assert edges.size == 2 * 228
    power = oracle_power(oracle, fir, padded(iq))
    assert power.size == r.decimated
    peaks = peaks_of(power, edges, r.decimated)
    # every on-run's peak within a factor 1.5 of its transmitter's nominal on power
    own = np.where(edges[0::2] < half // dec, nominal_power(1.0), nominal_power(0.25))
    ratio = peaks.astype(np.float64) / own
    print("peak / nominal:", ratio.min(), ratio.max())
    assert (ratio > 1 / 1.5).all() and (ratio < 1.5).all()
    # every message's level within 1.5 of its own transmitter and at least a factor 8 from the other
    pulses = ok.Device.load(golden_path("devices", g["device"]), RATE // dec).num_bits + 2
    assert pulses == 38
    levels = message_levels_of(edges, peaks, r.msg_samples, pulses)
    strong, weak = nominal_power(1.0), nominal_power(0.25)
    print("levels:", levels.tolist())
    for m, lv in enumerate(levels.astype(np.float64)):
        mine, other = (strong, weak) if m < 3 else (weak, strong)
        assert mine / 1.5 < lv < mine * 1.5, (m, lv)
        assert lv >= 8 * other or lv <= other / 8, (m, lv)
