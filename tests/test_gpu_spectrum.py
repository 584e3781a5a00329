"""The carrier survey on the GPU (ookd_spectrum_*; spectrum.hip).  Expected values come from the float64 restatement
of the contract (tests/spectrum_contract.py): every bin within the header's bound B[k], the worst |power - S| / B
recorded per test; runs are bitwise reproducible; and the feature end to end: Spectrum -> suggest_carriers ->
Receiver(tune=carrier.nu) returns the oracle's messages of the capture that was never moved, in Python and through
examples/ookd_rx.c --tune auto.

Worst |power - S| / B measured on an MI355X over every parity case of this file: see DESIGN.md 4.12."""
import subprocess
import zlib

import numpy as np
import pytest

from tests.helpers import golden_path
from tests.spectrum_contract import (DC, MOVES, N, NOISE, RATE, moved_golden, np_spectrum, two_transmitters,
                                     worst_over_bound)
from tests.tuned_contract import SPB, THR, golden_capture, moved, to_8bit

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ok():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from ookiedokie_amd import build as okbuild
    okbuild.build()
    import ookiedokie_amd as okm
    okm.lib()
    return okm


def _check(record_property, label, result, iq16):
    """frames and every bin of `result` against the float64 spectrum of the SC16Q11 capture iq16"""
    frames, power = result
    want_frames, S = np_spectrum(iq16)
    assert frames == want_frames == (np.asarray(iq16).size // 2) // N
    assert power.shape == (N,) and power.dtype == np.float64 and np.isfinite(power).all()
    worst = worst_over_bound(power, S)
    record_property("worst_over_bound", worst)
    print("worst |power - S| / B", label, worst)
    assert worst <= 1.0, label
    return worst


def _seed(*parts):
    return zlib.crc32("/".join(str(p) for p in parts).encode())


# ------------------------------------------------------------------------------- 1. parity ----

@pytest.mark.parametrize("fmt", ["sc16q11", "cs8", "cu8"])
@pytest.mark.parametrize("cap,nmsg,hz,want_bin", MOVES)
def test_parity_on_the_moved_golden_captures(ok, record_property, cap, nmsg, hz, want_bin, fmt):
    iq, _, _ = moved_golden(cap, hz, seed=_seed(cap, hz))
    raw = iq
    if fmt != "sc16q11":
        raw, iq = to_8bit(iq, fmt)
    sp = ok.Spectrum(sample_format=fmt)
    res = sp.spectrum(raw)
    _check(record_property, "%s %g %s" % (cap, hz, fmt), res, iq)
    assert sp.kernel_ms > 0.0
    carriers, _ = ok.suggest_carriers(res)
    assert [c.bin for c in carriers if not c.at_dc] == [want_bin]
    sp.close()


def test_parity_on_full_range_noise(ok, record_property):
    rng = np.random.default_rng(31)
    iq = rng.integers(-32768, 32768, size=2 * (37 * N)).astype(np.int16)
    iq[[0, 1, 2 * 5000, 2 * 20000 + 1]] = -32768
    assert iq.min() == -32768 and iq.max() == 32767
    sp = ok.Spectrum()
    _check(record_property, "uniform int16", sp.spectrum(iq), iq)
    for fmt, dt, lo, hi in (("cs8", np.int8, -128, 128), ("cu8", np.uint8, 0, 256)):
        raw = rng.integers(lo, hi, size=2 * (9 * N + 5)).astype(dt)
        raw[:2] = lo
        wide = (raw.astype(np.int16) - (128 if fmt == "cu8" else 0)) * 16
        s8 = ok.Spectrum(sample_format=fmt)
        _check(record_property, "uniform " + fmt, s8.spectrum(raw), wide)
        s8.close()
    sp.close()


@pytest.mark.parametrize("cycles", [205.0, 205.5, -307.0, 0.0, 512.0], ids=["on_bin", "half_way", "negative", "dc",
                                                                             "nyquist"])
def test_parity_on_full_scale_tones(ok, record_property, cycles):
    n = np.arange(8 * N, dtype=np.float64)
    z = 32767.0 * np.exp(2j * np.pi * ((cycles / N * n) % 1.0))
    iq = np.empty(2 * n.size, np.int16)
    iq[0::2], iq[1::2] = np.rint(z.real), np.rint(z.imag)
    sp = ok.Spectrum()
    frames, power = sp.spectrum(iq)
    _check(record_property, "tone %g" % cycles, (frames, power), iq)
    if cycles == int(cycles):
        assert int(np.argmax(power)) == int(cycles) % N
    sp.close()


@pytest.mark.parametrize("n", [N * 5 + 777, N * 33 + 777, N * 64, N, 1023, 1, 0])
def test_lengths(ok, record_property, n):
    iq = np.random.default_rng(n).integers(-2000, 2001, size=2 * n).astype(np.int16)
    sp = ok.Spectrum()
    frames, power = sp.spectrum(iq)
    _check(record_property, "n = %d" % n, (frames, power), iq)
    if n < N:
        assert frames == 0 and not power.any() and sp.kernel_ms == 0.0
        assert ok.suggest_carriers((frames, power))[0] == []
    sp.close()


@pytest.mark.parametrize("fmt", ["sc16q11", "cs8"])
def test_batched_device_and_unaligned_pointers(ok, record_property, fmt):
    import torch
    base, _ = golden_capture("G2")
    n = base.size // 2
    caps = 3
    # stride > length, once a multiple of 8 samples (every capture starts on a 16-byte boundary in both formats: the
    # vector path) and once one sample more (the scalar path)
    for extra in (0, 1):
        stride = n + 1000 + (-n) % 8 + extra
        host16 = np.zeros((caps, 2 * stride), np.int16)
        for c in range(caps):
            host16[c, :2 * n] = moved(base, (0.2, -0.3, 0.05)[c], DC, NOISE, seed=90 + c)
        if fmt == "sc16q11":
            raw = host16
        else:
            raw8 = [to_8bit(host16[c], fmt) for c in range(caps)]
            raw = np.stack([r for r, _ in raw8])
            host16 = np.stack([w for _, w in raw8])
        dev_t = torch.from_numpy(raw).cuda()
        sp = ok.Spectrum(sample_format=fmt, max_captures=caps)
        sp.spectrum_device(dev_t.data_ptr(), n, num_captures=caps, stride=stride)
        for c in range(caps):
            _check(record_property, "batched %s stride %d capture %d" % (fmt, stride, c), sp.result(c),
                   host16[c, :2 * n])
        with pytest.raises(ok.OokdError):
            sp.result(caps)
        with pytest.raises(ok.OokdError):
            sp.spectrum_device(dev_t.data_ptr(), n, num_captures=caps + 1, stride=stride)
        sp.close()

    # one capture: the device path equals the host path bit for bit, and a pointer moved on by one sample (4 or 2
    # bytes: the scalar path) gives the spectrum of the capture that starts there
    one = np.ascontiguousarray(raw[0, :2 * n])
    dev_t = torch.from_numpy(one).cuda()
    sp = ok.Spectrum(sample_format=fmt)
    h = sp.spectrum(one)
    sp.spectrum_device(dev_t.data_ptr(), n)
    d = sp.result()
    assert d[0] == h[0] and (d[1].view(np.uint64) == h[1].view(np.uint64)).all()
    sp.spectrum_device(dev_t.data_ptr() + one.itemsize * 2, n - 1)
    off = sp.result()
    _check(record_property, "offset by one sample " + fmt, off, host16[0, 2:2 * n])
    # the same samples through the vector path (the host copy is staged to an aligned buffer): the same bits
    via_host = sp.spectrum(np.ascontiguousarray(one[2:]))
    assert off[0] == via_host[0] and (off[1].view(np.uint64) == via_host[1].view(np.uint64)).all()
    sp.close()


# ---------------------------------------------------------------------- 2. reproducibility ----

def test_runs_are_bitwise_reproducible(ok):
    iq, _, _ = moved_golden("G2", 600e3, seed=4)
    short = iq[:2 * (N * 7 + 100)]
    sp = ok.Spectrum()
    a = sp.spectrum(iq)
    b = sp.spectrum(iq)
    assert a[0] == b[0] and (a[1].view(np.uint64) == b[1].view(np.uint64)).all()
    s1 = sp.spectrum(short)
    c = sp.spectrum(iq)
    assert (a[1].view(np.uint64) == c[1].view(np.uint64)).all()      # nothing of the short run leaks into this one
    assert sp.spectrum(np.zeros(0, np.int16))[0] == 0
    s2 = sp.spectrum(short)
    assert s1[0] == s2[0] == 7 and (s1[1].view(np.uint64) == s2[1].view(np.uint64)).all()
    sp.close()
    other = ok.Spectrum()                                            # and another context agrees
    d = other.spectrum(iq)
    assert (a[1].view(np.uint64) == d[1].view(np.uint64)).all()
    other.close()


# -------------------------------------------------------------------------------- 3. size ----

FOLD = 32               # kSpecFold: frames a lane sums in fp32 before it folds them into doubles
WAVES_PER_CU = 3 * 4    # kSpecGroupsPerCu workgroups of kSpecWaves waves: the grid fills the device once


def test_a_capture_of_2_28_samples(ok, record_property):
    """the grid stride, the 32-frame fold and the reduce kernel: a capture made on the device by repeating a moved
    golden capture, long enough that every wave of the grid takes more than 2 x 32 frames -- two folds and a
    remainder (85 frames per wave on 256 CUs); the reference is numpy's over the host copy"""
    import torch
    iq, _, _ = moved_golden("G1", -900e3, seed=8)
    one = iq.size // 2
    reps = -(-(1 << 28) // one)
    n = reps * one
    assert n >= 1 << 28
    waves = torch.cuda.get_device_properties(0).multi_processor_count * WAVES_PER_CU
    assert (n // N) // waves > 2 * FOLD, "the capture is too short for this device: no wave folds twice"
    dev_t = torch.from_numpy(iq).cuda().repeat(reps)
    assert dev_t.numel() == 2 * n
    host = np.tile(iq, reps)
    sp = ok.Spectrum()
    sp.spectrum_device(dev_t.data_ptr(), n)
    res = sp.result()
    print("%d samples, %d frames per wave: %.3f ms" % (n, (n // N) // waves, sp.kernel_ms))
    _check(record_property, "%d samples" % n, res, host)
    sp.spectrum_device(dev_t.data_ptr(), n)
    assert (sp.result()[1].view(np.uint64) == res[1].view(np.uint64)).all()
    sp.close()
    # three captures share the grid: a third of the groups each, a third of the frames each, so again two folds
    # and a remainder per wave, now through the batched addressing
    sp3 = ok.Spectrum(max_captures=3)
    third = n // 3
    assert (third // N) // -(-waves // 3) > 2 * FOLD
    sp3.spectrum_device(dev_t.data_ptr(), third, num_captures=3, stride=third)
    for c in range(3):
        _check(record_property, "third %d" % c, sp3.result(c), host[2 * c * third:2 * (c + 1) * third])
    sp3.close()


@pytest.mark.parametrize("per_wave", [31, 32, 33, 65])
def test_frames_per_wave_around_the_fold(ok, record_property, per_wave):
    """as many captures as the grid has workgroups, so each capture gets one workgroup and each of its four waves
    exactly `per_wave` frames: one short of a fold, exactly one, one more, and two folds plus one"""
    import torch
    caps = torch.cuda.get_device_properties(0).multi_processor_count * (WAVES_PER_CU // 4)
    n = 4 * per_wave * N                                        # samples per capture
    block = np.random.default_rng(per_wave).integers(-3000, 3001, size=2 * ((1 << 20) + 331)).astype(np.int16)
    reps = -(-(2 * n * caps) // block.size)
    dev_t = torch.from_numpy(block).cuda().repeat(reps)
    sp = ok.Spectrum(max_captures=caps)
    sp.spectrum_device(dev_t.data_ptr(), n, num_captures=caps, stride=n)
    for c in (0, 1, caps // 2, caps - 1):
        host = block[(2 * n * c + np.arange(2 * n)) % block.size]
        _check(record_property, "%d frames per wave, capture %d" % (per_wave, c), sp.result(c), host)
    sp.close()


# ---------------------------------------------------------------------------- 4. recovery ----

def _devs(ok, oracle, g):
    return (ok.Device.load(golden_path("devices", g["device"]), RATE),
            oracle.load_device_json(golden_path("devices", g["device"]), RATE)[0])


@pytest.mark.parametrize("cap,nmsg,hz,want_bin", MOVES)
def test_recovery_end_to_end(ok, oracle, cap, nmsg, hz, want_bin):
    iq, base, g = moved_golden(cap, hz, seed=int(abs(hz)) + nmsg)
    n = iq.size // 2
    sp = ok.Spectrum()
    carriers, floor = ok.suggest_carriers(sp.spectrum(iq))
    print(cap, hz, [(c.bin, c.at_dc, round(c.ratio, 1)) for c in carriers], floor)
    first = [c for c in carriers if not c.at_dc][0]
    assert first.bin == want_bin and first.nu == want_bin / N
    f = ok.Filter.load(golden_path("filters", "fs32_fs4"))
    d, od = _devs(ok, oracle, g)
    want = oracle.rx(base, oracle.load_filter_json(golden_path("filters", "fs32_fs4")), THR, od, SPB)
    assert len(want.msg_samples) == nmsg
    rx = ok.Receiver(f, d, max_samples=n, tune=first.nu)
    got = rx.rx(iq)
    assert list(got.msg_samples) == list(want.msg_samples)
    assert (got.payloads == want.payloads).all()
    rx.close()
    # at 1/16 of nominal level the carrier is still found (only the bin is asserted there)
    quiet, _, _ = moved_golden(cap, hz, scale=1 / 16, seed=int(abs(hz)) + nmsg)
    carriers, _ = ok.suggest_carriers(sp.spectrum(quiet))
    found = [c for c in carriers if not c.at_dc]
    print(cap, hz, "1/16:", [(c.bin, round(c.ratio, 1)) for c in found])
    assert found and found[0].bin == want_bin
    sp.close()


def test_two_transmitters_each_decode_their_own_device(ok, oracle):
    iq, (b1, g1), (b2, g2) = two_transmitters(seed=5)
    n = iq.size // 2
    sp = ok.Spectrum()
    carriers, _ = ok.suggest_carriers(sp.spectrum(iq))
    sp.close()
    by_bin = {c.bin: c for c in carriers}
    assert sorted(by_bin) == [-307, 0, 205] and by_bin[0].at_dc
    f = ok.Filter.load(golden_path("filters", "fs32_fs4"))
    of = oracle.load_filter_json(golden_path("filters", "fs32_fs4"))
    for want_bin, base, g, nmsg in ((205, b1, g1, 3), (-307, b2, g2, 2)):
        d, od = _devs(ok, oracle, g)
        want = oracle.rx(base, of, THR, od, SPB)
        assert len(want.msg_samples) == nmsg
        rx = ok.Receiver(f, d, max_samples=n, tune=by_bin[want_bin].nu)
        got = rx.rx(iq)
        assert list(got.msg_samples) == list(want.msg_samples), g["device"]
        assert (got.payloads == want.payloads).all(), g["device"]
        rx.close()


# ----------------------------------------------------------------------------- 5. example ----

def test_c_example_tune_auto(ok, tmp_path):
    from tests.test_host import _build_c_example
    exe = _build_c_example(tmp_path)
    iq, _, g = moved_golden("G1", 600e3, seed=12)
    cap = tmp_path / "moved.sc16q11"
    iq.tofile(str(cap))
    args = [str(cap), golden_path("devices", g["device"]), golden_path("filters", "fs32_fs4"), str(RATE), "csv"]
    auto = subprocess.run([exe, "--tune", "auto"] + args, capture_output=True, text=True, timeout=120)
    assert auto.returncode == 0, auto.stderr
    fixed = subprocess.run([exe, "--tune", "600000"] + args, capture_output=True, text=True, timeout=120)
    assert fixed.returncode == 0, fixed.stderr
    print(auto.stderr)
    assert "tune auto: carrier at" in auto.stderr and "at DC" in auto.stderr
    assert "tune auto: tuned to %.6g Hz" % (205 / N * RATE) in auto.stderr
    # the same rows, but for the value of the first column: "Decode Timestamp" is the wall clock
    rows, rows_fixed = auto.stdout.split("\n"), fixed.stdout.split("\n")
    assert rows[0] == rows_fixed[0] and rows[0].startswith("Decode Timestamp,") and len(rows) == len(rows_fixed) == 5
    assert [ln.split(",", 1)[1:] for ln in rows[1:]] == [ln.split(",", 1)[1:] for ln in rows_fixed[1:]]
    # untuned, the moved capture decodes nothing
    plain = subprocess.run([exe] + args, capture_output=True, text=True, timeout=120)
    assert plain.returncode == 0 and len(plain.stdout.split("\n")) < 5
    # no carrier beside DC: says so and decodes untuned, as a run without --tune does
    base, _ = golden_capture("G1")
    still = tmp_path / "still.sc16q11"
    moved(base, 0.0, DC, NOISE, seed=2).tofile(str(still))
    args[0] = str(still)
    none = subprocess.run([exe, "--tune", "auto"] + args, capture_output=True, text=True, timeout=120)
    untuned = subprocess.run([exe] + args, capture_output=True, text=True, timeout=120)
    assert none.returncode == 0 and "tune auto: no carrier beside DC" in none.stderr
    assert [ln.split(",", 1)[1:] for ln in none.stdout.split("\n")] == \
        [ln.split(",", 1)[1:] for ln in untuned.stdout.split("\n")]
    both = subprocess.run([exe, "--threshold", "auto", "--tune", "auto"] + args, capture_output=True, text=True)
    assert both.returncode != 0 and "--tune" in both.stderr and both.stdout == ""
