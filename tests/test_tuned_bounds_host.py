"""The input builders of the tuned / carrier bound tests (tests/tuned_bounds_inputs.py) do what they claim, checked
against the numpy contract with the library's own taps.  No GPU."""
import numpy as np
import pytest

import ookiedokie_amd as ok
from ookiedokie_amd import build as okbuild
from tests import tuned_bounds_inputs as B
from tests.helpers import golden_path
from tests.tuned_contract import SPB, contract_rx, lib_stages

NUS = [0.2, 0.125, 1.0 / 3000.0, 0.5]


@pytest.fixture(scope="module")
def built_lib():
    okbuild.build()
    return ok.lib()


def _filter(tmp_path, name):
    if name == "fs32_fs4":
        return ok.Filter.load(golden_path("filters", name))
    n = int(name[1:])
    return ok.Filter.load(B.write_filter(tmp_path, name, [(1, B.rand_taps(n, n))]))


def test_tap_pad_and_sweep_capture(built_lib):
    assert [B.ntaps_pad(t) for t in (1, 31, 32, 33, 255, 256)] == [32, 32, 32, 64, 256, 256]
    assert sorted({B.ntaps_pad(t) for t in B.SWEEP_TAPS}) == list(range(32, 257, 32))
    iq = B.sweep_capture()
    assert iq.size == 2 * B.SWEEP_N and B.SWEEP_N % 1024 and B.SWEEP_N > 3 * B.SWEEP_SPB
    z = B.as_complex(iq)
    assert np.abs(z.real).max() > 1400
    for lo, hi in B.SWEEP_STRETCHES:
        assert np.abs(iq[2 * lo:2 * hi]).max() <= 30
        # a whole R = 8 window with the longest tap history fits at any alignment
        t0 = -(-(lo + 256) // B.WINDOW) * B.WINDOW
        assert t0 + B.WINDOW <= hi and t0 + B.WINDOW <= B.SWEEP_N


@pytest.mark.parametrize("ntaps", [33, 256])
def test_sweep_stretches_are_quiet_and_the_rest_is_not(built_lib, tmp_path, ntaps):
    """the documented inequality holds in a window of every stretch and fails in the noise, at the sweep's threshold;
    the contract's bits are not all alike"""
    f = _filter(tmp_path, "t%d" % ntaps)
    (_, re, im), = lib_stages(f, 0.37)
    iq = B.sweep_capture()
    Tp = B.ntaps_pad(ntaps)
    lhs = {t0: B.documented_lhs(iq, re, im, t0, Tp) for t0 in B.interior_tiles(B.SWEEP_N, Tp)}
    quiet = [t0 for t0, v in lhs.items() if v < 0.5 * 0.1]
    assert len(quiet) >= len(B.SWEEP_STRETCHES) and len(quiet) < len(lhs)
    bits, _ = contract_rx(iq, [(1, re, im)], 0.1, B.SWEEP_SPB)
    assert bits.any() and not bits.all()
    for t0 in quiet:
        assert not bits[t0:t0 + B.WINDOW].any()


def test_unaligned_view_is_misaligned(built_lib):
    iq = B.sweep_capture()
    v = B.unaligned_view(iq)
    assert v.ctypes.data % 16 == 4 and v.flags["C_CONTIGUOUS"] and v.dtype == np.int16
    assert (v == iq).all()
    assert np.ascontiguousarray(v, dtype=np.int16).ctypes.data == v.ctypes.data     # handed over as it is


@pytest.mark.parametrize("A", [2047, 32767])
@pytest.mark.parametrize("nu", [0.2, -0.3, 1.0 / 3000.0, 0.5])
@pytest.mark.parametrize("name", ["t32", "t255", "t256"])
def test_margin_capture(built_lib, tmp_path, name, nu, A):
    f = _filter(tmp_path, name)
    (_, re, im), = lib_stages(f, nu)
    iq, outs = B.margin_capture(re, im, nu, A, np.random.default_rng(7))
    assert iq.size == 2 * 4 * B.MARGIN_SEG and outs.size >= 14
    S = float(np.abs(re.astype(np.float64)).sum() + np.abs(im.astype(np.float64)).sum())
    y = B.sum64(iq, re, im, SPB)
    # the aligned outputs reach S A, all of it in the real component
    assert y[outs, 0].max() >= 0.999 * S * A / 2048.0
    assert np.abs(y[:, 0]).max() <= S * 16.0
    # the cancelling windows run as high on the way and come back down
    cancel = y[B.MARGIN_SEG:2 * B.MARGIN_SEG]
    assert np.abs(cancel[outs, 0]).max() <= 0.1 * S * A / 2048.0
    # the contract is the same sum to float32 accuracy
    _, yc = contract_rx(iq, [(1, re, im)], 0.1, SPB)
    assert np.abs(yc.astype(np.float64) - y).max() <= 2.0 ** -24 * (2 * re.size + 1) * 1.01 * S * 16.0
    z = B.as_complex(iq)
    if A == 32767:
        assert z.real.min() == -32768 and z.real.max() == 32767
        assert (z[:B.MARGIN_SEG].real == -32768).any() and (z[3 * B.MARGIN_SEG:].real == -32768).any()
    else:
        assert np.abs(iq.astype(np.int32)).max() == 2047
    # the tone segment is full scale
    tone = z[2 * B.MARGIN_SEG:3 * B.MARGIN_SEG]
    assert np.abs(tone.real).max() >= 0.95 * A


def test_scale_capture(built_lib, tmp_path):
    iq = B.scale_capture()
    lo, hi = B.SCALE_STRETCH
    assert np.abs(iq[2 * lo:2 * hi]).max() <= 10 and np.abs(iq).max() > 1400
    for name in ("t32", "t255"):
        f = _filter(tmp_path, name)
        (_, re, im), = lib_stages(f, 0.2)
        _, y = contract_rx(iq, [(1, re, im)], 0.1, SPB)
        thr = float(np.float32(np.median(np.hypot(y[:, 0].astype(np.float64), y[:, 1].astype(np.float64)))))
        # a window inside the stretch satisfies the documented inequality at the median threshold
        t0 = -(-(lo + 256) // B.WINDOW) * B.WINDOW
        assert B.documented_lhs(iq, re, im, t0, B.ntaps_pad(re.size)) < 0.5 * thr


def test_spike_offsets():
    for T in (32, 255):
        Tp = B.ntaps_pad(T)
        offs = B.spike_offsets(T)
        assert len(set(offs)) == len(offs)
        for want in (-(T - 1), -(T - 2), -T, -1, 0, 1, 3, 4, 255, 256, B.WINDOW - 4, B.WINDOW - 1, -Tp):
            assert want in offs
        assert min(offs) == -Tp and max(offs) == B.WINDOW - 1


@pytest.mark.parametrize("thr", [0.02, 0.1, 0.5])
@pytest.mark.parametrize("nu", NUS, ids=["0.2", "0.125", "1_3000", "0.5"])
@pytest.mark.parametrize("name", ["fs32_fs4", "t255"])
def test_quiet_capture(built_lib, tmp_path, name, nu, thr):
    f = _filter(tmp_path, name)
    (_, re, im), = lib_stages(f, nu)
    T, Tp = re.size, B.ntaps_pad(re.size)
    iq, feats = B.quiet_capture(re, im, thr)
    n = iq.size // 2
    z = B.as_complex(iq)
    kinds = [k for k, _, _ in feats]
    assert kinds.count("spread") == 63 and kinds.count("spike") == len(B.spike_offsets(T)) and "extremes" in kinds
    interior = set(B.interior_tiles(n, Tp))
    A, G = B.tap_sums(re, im)
    bits, y = contract_rx(iq, [(1, re, im)], thr, SPB)
    mag = np.hypot(y[:, 0].astype(np.float64), y[:, 1].astype(np.float64))
    for kind, t0, detail in feats:
        assert t0 % (2 * B.WINDOW) == 0 and t0 in interior
        win = z[t0 - Tp:t0 + B.WINDOW]
        if kind == "spike":
            # the spike lands where it is documented, alone over DC
            height, off = detail
            assert z[t0 + off] == B.DC + height
            rest = np.delete(z[t0 - B.WINDOW:t0 + B.WINDOW], off + B.WINDOW)
            assert (rest == B.DC).all()
            in_taps = off > -T                              # it weighs in some output of the tile
            base = y[t0 - B.WINDOW + T]                     # an output of the own region that sees DC only
            dev = np.abs(y[t0:t0 + B.WINDOW].astype(np.float64) - base.astype(np.float64)).max()
            assert (dev > 0.0) == in_taps, (off, dev)
        elif kind == "spread":
            half, pos, fac = detail
            k = np.arange(T)
            d = z[t0 - B.WINDOW]
            got = z[t0 + pos - k] - d
            assert (np.abs(got.real) == half).all() and (np.abs(got.imag) == half).all()
            # laid on the taps: the output's real component is d's plus S half
            S = float(np.abs(re.astype(np.float64)).sum() + np.abs(im.astype(np.float64)).sum())
            c = re.astype(np.float64) + 1j * im.astype(np.float64)
            want = (d * c.sum()).real / 2048.0 + S * half / 2048.0
            assert abs(float(y[t0 + pos, 0]) - want) <= (2 * T + 1) * 2.0 ** -24 * S * 16.0
            # the sweep crosses the documented decision where the offset leaves room for it
            lhs = B.documented_lhs(iq, re, im, t0, Tp)
            b = 2.0 * max(abs(d.real), abs(d.imag))
            if B.SQRT2 / 4096.0 * G * b < 0.5 * thr and half > 8:
                assert (lhs < thr) == (fac < 1.0) or fac == 1.0, (fac, lhs, thr)
        elif kind == "extremes":
            assert win.real.min() == -32768 and win.real.max() == 32767
            assert win.imag.min() == -32768 and win.imag.max() == 32767
        elif kind == "dc":
            assert (z[t0 - B.WINDOW:t0 + B.WINDOW] == detail).all()
    # the two counts the GPU test holds quiet_waves between: both non-zero, and apart
    lo, hi = B.quiet_count_bounds(iq, re, im, thr, bits, Tp)
    assert 0 < lo < hi, (lo, hi)
    # the thresholds straddle the planted outputs
    assert bits.any() and not bits.all()
    spread_out = np.array([t0 + d[1] for k, t0, d in feats if k == "spread"])
    assert mag[spread_out].min() < thr <= mag[spread_out].max()
    # a window the documented inequality calls quiet holds no set bit
    for t0 in interior:
        if B.documented_lhs(iq, re, im, t0, Tp) < thr * 0.999:
            assert not bits[t0:t0 + B.WINDOW].any(), t0


def test_dc_windows_are_loud_in_the_pass_band_and_quiet_beside_it(built_lib):
    """fs32_fs4, threshold 0.1, a DC-only window of 1000 LSB: every bit set at nu = 1/3000 (0 Hz is in the pass
    band), the documented inequality holds with room at nu = 0.2 (0 Hz is in the stop band)"""
    f = _filter(None, "fs32_fs4")
    for nu, loud in ((1.0 / 3000.0, True), (0.2, False)):
        (_, re, im), = lib_stages(f, nu)
        iq, feats = B.quiet_capture(re, im, 0.1)
        t0, = [t for k, t, d in feats if k == "dc" and d == 1000]
        bits, _ = contract_rx(iq, [(1, re, im)], 0.1, SPB)
        lhs = B.documented_lhs(iq, re, im, t0, 32)
        if loud:
            assert bits[t0:t0 + B.WINDOW].all() and lhs > 0.1
        else:
            assert not bits[t0:t0 + B.WINDOW].any() and lhs < 0.05


def test_split_capture_length():
    assert B.SPLIT_N == 5 * 65536 + 777
    iq = B.tiled(np.arange(10, dtype=np.int16), 12)
    assert iq.size == 24 and iq[10] == 0 and iq[23] == 3
