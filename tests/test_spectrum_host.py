"""CPU-side tests of the carrier survey: the new symbols and constants, ookd_spectrum_bin_nu, and
ookd_suggest_carriers -- against the Python restatement of the rule (tests/spectrum_contract.py) on crafted spectra,
and on the float64 spectra numpy computes of the moved golden captures and of noise alone."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests.spectrum_contract import (DC, MOVES, N, NOISE, RATE, as_tuples, bin_nu, moved_golden, np_spectrum,
                                     py_suggest, two_transmitters)
from tests.tuned_contract import golden_capture, moved

import ookiedokie_amd as ok
from ookiedokie_amd import build as okbuild


@pytest.fixture(scope="session", autouse=True)
def built_lib():
    okbuild.build()
    return ok.lib()


def _same(power, frames=1, **kw):
    """the library's suggestion equals the rule's; returns it"""
    got, floor = ok.suggest_carriers(power, frames=frames, min_ratio=kw.get("min_ratio", 0.0),
                                     min_spacing_bins=kw.get("min_spacing", 0), max_carriers=kw.get("capacity", 16))
    want, wfloor = py_suggest(power, frames, **kw)
    assert floor == wfloor
    assert as_tuples(got) == want, (as_tuples(got), want)
    for c in got:
        assert c.nu == bin_nu(c.bin) and -N // 2 <= c.bin < N // 2
    return got, floor


def _flat(level=1.0, **peaks):
    p = np.full(N, level, dtype=np.float64)
    for k, v in peaks.items():
        p[int(k[1:]) % N] = v
    return p


# ---- interface --------------------------------------------------------------------------------------------

def test_new_symbols_are_exported(built_lib):
    for name in ("ookd_spectrum_create", "ookd_spectrum_destroy", "ookd_spectrum_device", "ookd_spectrum_host",
                 "ookd_spectrum_get", "ookd_spectrum_kernel_ms", "ookd_spectrum_bin_nu", "ookd_suggest_carriers"):
        assert hasattr(built_lib, name), name
    assert built_lib.ookd_spectrum_kernel_ms(None) == 0.0
    built_lib.ookd_spectrum_destroy(None)
    for name in ("Spectrum", "suggest_carriers", "spectrum_bin_nu", "Carrier"):
        assert hasattr(ok, name), name
    with pytest.raises(ValueError):
        ok.Spectrum(sample_format="cf32")
    with pytest.raises(ValueError):
        ok.suggest_carriers(np.zeros(1023))


def test_constants_and_layouts(tmp_path):
    src = tmp_path / "sp.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ookiedokie_amd.h"\n'
                   'int main(void) { printf("%d %d %d %.17g %.17g %zu %zu %zu %zu %zu", OOKD_SPECTRUM_BINS,\n'
                   '  OOKD_CARRIER_MIN_SPACING, OOKD_API_VERSION, OOKD_CARRIER_MIN_RATIO, OOKD_SPECTRUM_EPS,\n'
                   '  sizeof(ookd_spectrum_result), sizeof(ookd_carrier), offsetof(ookd_carrier, at_dc),\n'
                   '  offsetof(ookd_carrier, ratio), sizeof(ookd_level_hist));\n'
                   '  return 0; }\n')
    exe = tmp_path / "sp"
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.dirname(ok.HEADER_PATH), str(src),
                        "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = subprocess.run([str(exe)], capture_output=True, text=True).stdout.split()
    assert [int(x) for x in got[:3]] == [ok.SPECTRUM_BINS, ok.CARRIER_MIN_SPACING, 1] == [1024, 32, 1]
    assert [float(x) for x in got[3:5]] == [ok.CARRIER_MIN_RATIO, ok.SPECTRUM_EPS] == [64.0, 120.0 / 2 ** 24]
    assert [int(x) for x in got[5:]] == [C.sizeof(ok.SpectrumResult), C.sizeof(ok.CarrierStruct),
                                         ok.CarrierStruct.at_dc.offset, ok.CarrierStruct.ratio.offset,
                                         C.sizeof(ok.LevelHist)] == [8 * 1025, 32, 12, 24, 8 * 257]


def test_bin_nu(built_lib):
    assert [ok.spectrum_bin_nu(k) for k in (0, 1, 511, 512, 1023)] == [0.0, 1 / 1024, 511 / 1024, -0.5, -1 / 1024]
    assert [built_lib.ookd_spectrum_bin_nu(k) for k in range(N)] == [bin_nu(k) for k in range(N)]
    assert ok.spectrum_bin_nu(205) * RATE == pytest.approx(600e3, abs=RATE / N / 2)
    assert ok.spectrum_bin_nu(-307) * RATE == pytest.approx(-900e3, abs=RATE / N / 2)


# ---- the rule on crafted spectra --------------------------------------------------------------------------

def test_single_peak():
    got, floor = _same(_flat(b205=1000.0))
    assert floor == 1.0 and as_tuples(got) == [(205, False, 1000.0, 1000.0)]
    assert got[0].nu == 205 / 1024
    got, _ = _same(_flat(b717=1000.0))
    assert got[0].bin == -307 and got[0].nu == -307 / 1024


def test_peaks_32_bins_apart_merge_and_33_do_not():
    got, _ = _same(_flat(b100=500.0, b132=400.0))
    assert [c.bin for c in got] == [100]
    got, _ = _same(_flat(b100=500.0, b133=400.0))
    assert [c.bin for c in got] == [100, 133]
    # decreasing power whatever the bin order
    got, _ = _same(_flat(b100=400.0, b133=500.0))
    assert [c.bin for c in got] == [133, 100]


def test_suppression_wraps_across_1023_and_0():
    got, _ = _same(_flat(b1010=500.0, b18=400.0))                 # 32 apart across the wrap
    assert [c.bin for c in got] == [-14]
    got, _ = _same(_flat(b1010=500.0, b19=400.0))
    assert [c.bin for c in got] == [-14, 19]
    got, _ = _same(_flat(b5=500.0, b997=400.0))                   # and the other way round
    assert [c.bin for c in got] == [5]


def test_at_dc_is_bins_minus_1_to_1():
    for k, flag in ((1023, True), (0, True), (1, True), (2, False), (1022, False)):
        got, _ = _same(_flat(**{"b%d" % k: 900.0}))
        assert len(got) == 1 and got[0].at_dc is flag, k
        assert got[0].bin == (k if k < 512 else k - 1024)


def test_a_tie_goes_to_the_lower_bin():
    got, _ = _same(_flat(b300=700.0, b600=700.0, b900=700.0))
    assert [c.bin for c in got] == [300, 600 - 1024, 900 - 1024]
    got, _ = _same(_flat(b300=700.0, b320=700.0))                 # within the spacing: the lower one survives
    assert [c.bin for c in got] == [300]


def test_capacity_smaller_than_the_number_of_peaks():
    p = _flat(b100=900.0, b200=800.0, b300=700.0, b400=600.0)
    for cap in (1, 2, 3, 4, 16):
        got, _ = _same(p, capacity=cap)
        assert [c.bin for c in got] == [100, 200, 300, 400][:cap]
    sp = ok.SpectrumResult()
    sp.frames = 1
    C.memmove(sp.power, p.ctypes.data, p.nbytes)
    count, floor = C.c_uint32(7), C.c_double(-1.0)
    assert ok.lib().ookd_suggest_carriers(C.byref(sp), 0.0, 0, None, 0, C.byref(count), C.byref(floor)) == 0
    assert count.value == 0 and floor.value == 1.0


def test_no_frames_all_equal_and_floor_zero():
    p = _flat(b205=1000.0)
    got, floor = _same(p, frames=0)
    assert got == [] and floor == 1.0
    assert ok.suggest_carriers((0, p))[0] == [] and len(ok.suggest_carriers((3, p))[0]) == 1
    got, _ = _same(_flat(7.5))
    assert got == []
    got, floor = _same(np.zeros(N))
    assert got == [] and floor == 0.0
    # floor == 0: whatever is positive qualifies, its ratio is infinite
    p = np.zeros(N)
    p[205], p[600] = 3.0, 1e-30
    got, floor = _same(p)
    assert floor == 0.0 and [c.bin for c in got] == [205, 600 - 1024] and got[0].ratio == float("inf")


def test_default_and_explicit_ratio_and_spacing():
    p = _flat(b100=64.0, b300=63.999, b500=10.0)
    got, _ = _same(p)
    assert [c.bin for c in got] == [100]                          # 64 x floor qualifies, just under does not
    got, _ = _same(p, min_ratio=64.0)
    assert [c.bin for c in got] == [100]
    got, _ = _same(p, min_ratio=5.0)
    assert [c.bin for c in got] == [100, 300, 500]
    got, _ = _same(p, min_ratio=1000.0)
    assert got == []
    p = _flat(b100=500.0, b110=400.0, b132=300.0)
    got, _ = _same(p, min_spacing=32)
    assert [c.bin for c in got] == [100]
    got, _ = _same(p, min_spacing=9)
    assert [c.bin for c in got] == [100, 110, 132]
    got, _ = _same(p, min_spacing=10)
    assert [c.bin for c in got] == [100, 132]
    got, _ = _same(p, min_spacing=600)                            # everything within reach of the first
    assert [c.bin for c in got] == [100]


def test_null_arguments(built_lib):
    sp = ok.SpectrumResult()
    out = (ok.CarrierStruct * 4)()
    count, floor = C.c_uint32(0), C.c_double(0.0)
    fn = built_lib.ookd_suggest_carriers
    assert fn(None, 0.0, 0, out, 4, C.byref(count), C.byref(floor)) == -1 and "NULL" in ok.last_error()
    assert fn(C.byref(sp), 0.0, 0, None, 4, C.byref(count), C.byref(floor)) == -1 and "NULL" in ok.last_error()
    assert fn(C.byref(sp), 0.0, 0, out, 4, None, C.byref(floor)) == -1 and "NULL" in ok.last_error()
    assert fn(C.byref(sp), -1.0, 0, out, 4, C.byref(count), C.byref(floor)) == -1
    assert fn(C.byref(sp), float("nan"), 0, out, 4, C.byref(count), C.byref(floor)) == -1
    assert fn(C.byref(sp), 0.0, 0, out, 4, C.byref(count), None) == 0          # the floor is optional
    assert built_lib.ookd_spectrum_get(None, 0, C.byref(sp)) == -1
    assert built_lib.ookd_spectrum_device(None, None, 1, 0, 0) == -1
    assert built_lib.ookd_spectrum_host(None, None, 0) == -1


# ---- the rule on float64 spectra of the golden captures ---------------------------------------------------

@pytest.mark.parametrize("cap,nmsg,hz,want_bin", MOVES)
def test_moved_golden_captures_give_the_carrier_and_dc(cap, nmsg, hz, want_bin):
    iq, base, _ = moved_golden(cap, hz, seed=int(abs(hz)) + nmsg)
    frames, S = np_spectrum(iq)
    assert frames == (iq.size // 2) // N and frames > 0
    got, floor = _same(S, frames)
    print(cap, hz, [(c.bin, c.at_dc, round(c.ratio, 1)) for c in got], floor)
    assert sorted((c.bin, c.at_dc) for c in got) == sorted([(want_bin, False), (0, True)])
    assert round(hz / RATE * N) == want_bin
    # the capture that was never moved: only the peak at DC (its own carrier, and the DC term on top)
    still = moved(base, 0.0, DC, NOISE, seed=3)
    frames, S = np_spectrum(still)
    got, _ = _same(S, frames)
    assert [(c.bin, c.at_dc) for c in got] == [(0, True)]


def test_two_transmitters_in_one_capture():
    iq, _, _ = two_transmitters(seed=5)
    frames, S = np_spectrum(iq)
    got, _ = _same(S, frames)
    assert sorted((c.bin, c.at_dc) for c in got) == sorted([(205, False), (-307, False), (0, True)])


@pytest.mark.parametrize("frames", [1, 100])
def test_noise_alone_gives_no_carrier(frames):
    worst = 0.0
    for seed in range(50):
        iq = np.random.default_rng(1000 * frames + seed).integers(-NOISE, NOISE + 1, size=2 * N * frames)
        f, S = np_spectrum(iq.astype(np.int16))
        assert f == frames
        got, floor = _same(S, f)
        assert got == [], (seed, as_tuples(got))
        worst = max(worst, S.max() / floor)
    print("worst max / median over 50 seeds,", frames, "frames:", worst)
    assert worst < ok.CARRIER_MIN_RATIO


def test_np_spectrum_is_the_definition():
    """the restatement against the contract's sum, written out for a few bins of a short capture"""
    rng = np.random.default_rng(9)
    iq = rng.integers(-2000, 2001, size=2 * (2 * N + 300)).astype(np.int16)
    frames, S = np_spectrum(iq)
    assert frames == 2
    z = (iq[0::2] + 1j * iq[1::2]) / 2048.0
    n = np.arange(N)
    w = 0.5 - 0.5 * np.cos(2 * np.pi * n / N)
    for k in (0, 1, 205, 512, 717, 1023):
        want = sum(abs(np.sum(w * z[N * f:N * f + N] * np.exp(-2j * np.pi * k * n / N))) ** 2 for f in range(2))
        assert S[k] == pytest.approx(want, rel=1e-10)
    assert np_spectrum(iq[:2 * 1023]) [0] == 0 and not np_spectrum(iq[:2 * 1023])[1].any()
    # a capture moved to +600 kHz peaks at bin 205: the sign convention of ookd_tune.nu
    base, _ = golden_capture("G1")
    _, S = np_spectrum(moved(base, 600e3 / RATE))
    assert int(np.argmax(S)) == 205


def test_spectrum_fails_loudly_without_a_gpu_or_on_bad_flags(built_lib):
    both = ok.RX_SAMPLES_CS8 | ok.RX_SAMPLES_CU8
    assert not built_lib.ookd_spectrum_create(0, both, 1, None)
    assert "sample_flags" in ok.last_error()
    assert not built_lib.ookd_spectrum_create(0, 1, 1, None)          # a bit that is no sample format
    assert "sample_flags" in ok.last_error()
    assert not built_lib.ookd_spectrum_create(0, 0, 0, None)
    assert "max_captures" in ok.last_error()
    h = built_lib.ookd_spectrum_create(-1, 0, 1, None)
    assert not h and "no CPU fallback" in ok.last_error()
