"""CPU-side tests of the envelope survey: the new symbols and constants, the bin rule against its numpy restatement,
and ookd_suggest_threshold -- against an exact Python restatement of the rule, on hand-made histograms, and on
histograms numpy builds from the oracle's filter output, where the suggested threshold has to decode the golden
captures at every level down to 1/16 of nominal.  tests/test_gpu_survey.py imports the fixture builders below."""
import ctypes as C
import json
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from tests.helpers import golden_path, iq_from_rle

import ookiedokie_amd as ok
from ookiedokie_amd import build as okbuild

RATE = 3000000
BINS = 256
BIN_BASE = (127 - 40) << 2
SCALES = (1.0, 1 / 4, 1 / 8, 1 / 16)
GOLDENS = (("G1", 3, 36), ("G2", 2, 32))


@pytest.fixture(scope="session", autouse=True)
def built_lib():
    okbuild.build()
    return ok.lib()


# ---- numpy / Python restatements (independent of the library) ---------------------------------------------

def np_bins(power):
    """b = clamp((bits(p) >> 21) - ((127 - 40) << 2) + 1, 0, 255)"""
    bits = np.ascontiguousarray(power, dtype=np.float32).view(np.uint32)
    return np.clip((bits >> 21).astype(np.int64) - BIN_BASE + 1, 0, BINS - 1)


def np_hist(power):
    return np.bincount(np_bins(power), minlength=BINS).astype(np.uint64)


def np_bin_lower(b):
    if b == 0:
        return np.float32(0.0)
    return np.array([(b - 1 + BIN_BASE) << 21], dtype=np.uint32).view(np.float32)[0]


def oracle_power(oracle, fir, iq):
    """complexf_power of the oracle's filter output (of the unpacked samples when fir is None), float32"""
    y = oracle.unpack(iq)
    if fir is not None:
        y = oracle.fir_run(fir, y)
    if y.shape[0] == 0:
        return np.zeros(0, dtype=np.float32)
    rr = (y[:, 0] * y[:, 0]).astype(np.float32)
    ii = (y[:, 1] * y[:, 1]).astype(np.float32)
    return (rr + ii).astype(np.float32)


def py_amplitude(b):
    return 0.0 if b == 0 else float(np.sqrt(np.sqrt(np.float64(np_bin_lower(b)) * np.float64(np_bin_lower(b + 1)))))


def py_median(h, lo, hi):
    total = sum(h[lo:hi])
    c = 0
    for b in range(lo, hi):
        c += h[b]
        if c >= (total + 1) // 2:
            return b
    raise AssertionError("empty side")


def py_suggest(hist):
    """the header's rule in Python integers and Fractions"""
    h = [int(x) for x in hist]
    n = sum(h)
    S = sum(i * x for i, x in enumerate(h))
    out = dict(found=0, threshold=0.0, off_level=0.0, on_level=0.0, split_bin=0, off_bin=0, on_bin=0, on_fraction=0.0)
    occupied = [i for i, x in enumerate(h) if x]
    if n == 0:
        return out
    if len(occupied) == 1:
        out.update(split_bin=occupied[0], off_bin=occupied[0], on_bin=occupied[0])
        return out
    best, tied = None, []
    a = s0 = 0
    for k in range(BINS - 1):
        a += h[k]
        s0 += k * h[k]
        if a == 0 or a == n:
            continue
        v = Fraction((n * s0 - a * S) ** 2, a * (n - a))
        if best is None or v > best:
            best, tied = v, [k]
        elif v == best:
            tied.append(k)
    k = (tied[0] + tied[-1]) // 2
    n_off = sum(h[:k + 1])
    off_bin, on_bin = py_median(h, 0, k + 1), py_median(h, k + 1, BINS)
    off, on = np.float32(py_amplitude(off_bin)), np.float32(py_amplitude(on_bin))
    out.update(split_bin=k, off_bin=off_bin, on_bin=on_bin, off_level=float(off), on_level=float(on),
               on_fraction=(n - n_off) / n)
    if on_bin - off_bin >= ok.LEVEL_MIN_SEPARATION and min(n_off, n - n_off) >= ok.LEVEL_MIN_SIDE:
        out.update(found=1, threshold=float((off + on) / np.float32(2.0)))
    return out


def assert_same_suggestion(got, want):
    for key in ("found", "split_bin", "off_bin", "on_bin"):
        assert got[key] == want[key], (key, got, want)
    for key in ("threshold", "off_level", "on_level"):
        assert got[key] == pytest.approx(want[key], rel=1e-6, abs=0), (key, got, want)
    assert got["on_fraction"] == pytest.approx(want["on_fraction"], rel=1e-12, abs=0)


# ---- fixtures ---------------------------------------------------------------------------------------------

def scaled_golden(vectors, name, scale, noise_seed=None, noise=40):
    """golden capture G1 / G2 at `scale` of its nominal level, clean or with +-noise LSB of uniform noise"""
    g = vectors[name]
    iq = np.round(iq_from_rle(g["i_rle"], g["num_samples"]).astype(np.float64) * scale)
    if noise_seed is not None:
        iq = iq + np.random.default_rng(noise_seed).integers(-noise, noise + 1, size=iq.size)
    return g, np.clip(iq, -32768, 32767).astype(np.int16)


def quiet_cs8(vectors):
    """The end-to-end fixture: noisy G1 at 1/16 of nominal level (on level 121 LSB, noise +-40 LSB) cut to 8 bits
    -- on level 7, noise within -3 .. 2 -- as int8 values.  The cut keeps the signal: 7 steps of an 8-bit
    converter, where 1/32 of nominal level would leave 3."""
    g, iq = scaled_golden(vectors, "G1", 1 / 16, noise_seed=11)
    return g, (iq >> 4).astype(np.int8)


def _decode(oracle, g, iq, threshold):
    of = oracle.load_filter_json(golden_path("filters", g["filter"]))
    od, _ = oracle.load_device_json(golden_path("devices", g["device"]), RATE)
    return oracle.rx(iq, of, threshold, od, g["spb"])


# ---- interface --------------------------------------------------------------------------------------------

def test_new_symbols_are_exported(built_lib):
    for name in ("ookd_survey_create", "ookd_survey_destroy", "ookd_survey_device", "ookd_survey_host",
                 "ookd_survey_get_hist", "ookd_survey_kernel_ms", "ookd_level_bin", "ookd_level_bin_lower",
                 "ookd_suggest_threshold"):
        assert hasattr(built_lib, name), name
    assert built_lib.ookd_survey_kernel_ms(None) == 0.0
    built_lib.ookd_survey_destroy(None)
    assert built_lib.ookd_suggest_threshold(None, None) == -1 and "NULL" in ok.last_error()
    for name in ("Survey", "level_bin", "level_bin_lower", "suggest_threshold"):
        assert hasattr(ok, name), name
    with pytest.raises(ValueError):
        ok.Survey(None, sample_format="cf32")


def test_constants_and_layouts(tmp_path):
    src = tmp_path / "sv.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ookiedokie_amd.h"\n'
                   'int main(void) { printf("%d %d %d %d %zu %zu %zu %zu %zu %zu %zu %zu", OOKD_LEVEL_BINS,\n'
                   '  OOKD_LEVEL_MIN_SEPARATION, OOKD_LEVEL_MIN_SIDE, OOKD_API_VERSION, sizeof(ookd_level_hist),\n'
                   '  sizeof(ookd_threshold_suggestion), offsetof(ookd_threshold_suggestion, split_bin),\n'
                   '  offsetof(ookd_threshold_suggestion, on_fraction), sizeof(ookd_rx_config), sizeof(ookd_rx_stats),\n'
                   '  sizeof(ookd_front_info), sizeof(ookd_message));\n'
                   '  return 0; }\n')
    exe = tmp_path / "sv"
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.dirname(ok.HEADER_PATH), str(src), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True).stdout.split()]
    assert got[:3] == [ok.LEVEL_BINS, ok.LEVEL_MIN_SEPARATION, ok.LEVEL_MIN_SIDE] == [256, 18, 512]
    assert got[3] == 1 == ok.lib().ookd_api_version()             # symbols were added, nothing else
    assert got[4:8] == [C.sizeof(ok.LevelHist), C.sizeof(ok.ThresholdSuggestion),
                        ok.ThresholdSuggestion.split_bin.offset, ok.ThresholdSuggestion.on_fraction.offset]
    assert got[4] == 8 * 257
    # what they were before the survey
    assert got[8:] == [C.sizeof(ok.RxConfig), C.sizeof(ok.RxStats), C.sizeof(ok.FrontInfo), C.sizeof(ok.Message)] \
        == [80, 104, 56, 48]
    assert (ok.RX_SAMPLES_CS8, ok.RX_SAMPLES_CU8, ok.FRONT_FIR2_MFMA_8) == (1 << 10, 1 << 11, 11)


# ---- bins -------------------------------------------------------------------------------------------------

def test_level_bin_is_the_formula(built_lib):
    edges = np.array([np_bin_lower(b) for b in range(1, BINS)], dtype=np.float32)
    eb = edges.view(np.uint32)
    special = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1e-45, 1e-40, 1.1754942e-38, 1.17549435e-38,
                        2.0 ** -41, 2.0 ** -40, 2.0 ** 23.5, 3.4028235e38, 1.0, 0.01], dtype=np.float32)
    nan_patterns = np.array([0x7fc00000, 0xffc00000, 0x7f800001, 0xff800000], dtype=np.uint32)
    rng = np.random.default_rng(2024)
    patterns = np.concatenate([eb, eb - 1, eb + 1, special.view(np.uint32), nan_patterns,
                               rng.integers(0, 1 << 32, size=100000, dtype=np.uint64).astype(np.uint32)])
    want = np_bins(patterns.view(np.float32))
    fn = built_lib.ookd_level_bin
    got = np.array([fn(C.c_float.from_buffer_copy(int(p).to_bytes(4, "little"))) for p in patterns], dtype=np.int64)
    assert (got == want).all(), patterns[got != want][:8]
    # the documented edges
    assert ok.level_bin(0.0) == 0 and ok.level_bin(float(np.float32(2.0 ** -40)) * 0.999) == 0
    assert ok.level_bin(2.0 ** -40) == 1 and ok.level_bin(2.0 ** -39) == 5
    assert ok.level_bin(1.5 * 2.0 ** 23) == 255 and ok.level_bin(1.5 * 2.0 ** 23 - 1.0) == 254
    assert ok.level_bin(2.0 ** 24) == 255
    assert ok.level_bin(float("inf")) == 255 and ok.level_bin(float("nan")) == 255
    assert want[len(eb):2 * len(eb)].tolist() == list(range(0, BINS - 1))    # just under an edge: the bin below


def test_bin_lower_inverts_bin(built_lib):
    assert ok.level_bin_lower(0) == 0.0
    for b in range(1, BINS):
        lo = ok.level_bin_lower(b)
        assert lo == float(np_bin_lower(b)) and ok.level_bin(lo) == b
        # four bins per octave, cut at 1, 1.25, 1.5 and 1.75 times the power of two
        assert lo == 2.0 ** (-40 + (b - 1) // 4) * (1 + ((b - 1) % 4) / 4)


# ---- the rule on hand-made histograms ---------------------------------------------------------------------

def _hist(**counts):
    h = np.zeros(BINS, dtype=np.uint64)
    for k, v in counts.items():
        h[int(k[1:])] = v
    return h


def test_two_spikes_give_the_amplitude_midpoint():
    h = _hist(b40=1000, b100=1000)
    s = ok.suggest_threshold(h)
    # every split 40..99 separates the spikes equally well: the middle of the tied range
    assert (s["found"], s["split_bin"], s["off_bin"], s["on_bin"]) == (1, (40 + 99) // 2, 40, 100)
    off, on = py_amplitude(40), py_amplitude(100)
    assert s["off_level"] == pytest.approx(off, rel=1e-6) and s["on_level"] == pytest.approx(on, rel=1e-6)
    assert s["threshold"] == pytest.approx((off + on) / 2, rel=1e-6)
    assert s["on_fraction"] == 0.5
    # the amplitude of a bin: fourth root of the product of its power edges (bin 100 = 1.75 .. 2 x 2^-16)
    assert on == pytest.approx((1.75 * 2.0 ** -16 * 2.0 ** -15) ** 0.25, rel=1e-12)
    assert_same_suggestion(s, py_suggest(h))


def test_off_level_of_bin_zero_is_zero():
    s = ok.suggest_threshold(_hist(b0=5000, b160=700))
    assert s["found"] == 1 and s["off_bin"] == 0 and s["off_level"] == 0.0
    assert s["threshold"] == pytest.approx(py_amplitude(160) / 2, rel=1e-6)
    assert s["split_bin"] == (0 + 159) // 2


def test_plateau_between_the_spikes():
    """a flat floor of single counts between two heavy spikes: unequal weights move the split, the medians stay"""
    h = _hist(b30=9000, b120=3000)
    h[31:120] = 1
    s = ok.suggest_threshold(h)
    assert_same_suggestion(s, py_suggest(h))
    assert s["found"] == 1 and s["off_bin"] == 30 and s["on_bin"] == 120 and 30 < s["split_bin"] < 120
    # a symmetric histogram splits at its centre
    h = np.zeros(BINS, dtype=np.uint64)
    h[50:54] = (7, 3, 3, 7)
    p = py_suggest(h)
    s = ok.suggest_threshold(h)
    assert_same_suggestion(s, p)
    assert s["split_bin"] == 51 and s["found"] == 0            # 3 bins apart: not two levels


def test_one_side_empty_and_empty_histogram():
    s = ok.suggest_threshold(np.zeros(BINS, dtype=np.uint64))
    assert s == dict(found=0, threshold=0.0, off_level=0.0, on_level=0.0, split_bin=0, off_bin=0, on_bin=0,
                     on_fraction=0.0)
    s = ok.suggest_threshold(_hist(b77=123456))
    assert s["found"] == 0 and s["threshold"] == 0.0 and s["off_bin"] == s["on_bin"] == 77
    assert_same_suggestion(s, py_suggest(_hist(b77=123456)))
    with pytest.raises(ValueError):
        ok.suggest_threshold(np.zeros(255, dtype=np.uint64))


def test_separation_and_side_limits():
    sep, side = ok.LEVEL_MIN_SEPARATION, ok.LEVEL_MIN_SIDE
    assert ok.suggest_threshold(_hist(b100=5000, **{"b%d" % (100 + sep): 5000}))["found"] == 1
    s = ok.suggest_threshold(_hist(b100=5000, **{"b%d" % (100 + sep - 1): 5000}))
    assert s["found"] == 0 and s["threshold"] == 0.0 and s["on_bin"] - s["off_bin"] == sep - 1
    assert ok.suggest_threshold(_hist(b60=side, b160=10 ** 7))["found"] == 1
    assert ok.suggest_threshold(_hist(b60=side - 1, b160=10 ** 7))["found"] == 0
    assert ok.suggest_threshold(_hist(b60=10 ** 7, b160=side - 1))["found"] == 0


def test_exact_arithmetic_at_64_bit_counts():
    """counts near 2^63: the criterion's products need some 400 bits; a float comparison would tie or misorder"""
    big = (1 << 62)
    h = _hist(b10=big, b11=1, b200=big - 1, b201=2)
    assert_same_suggestion(ok.suggest_threshold(h), py_suggest(h))
    rng = np.random.default_rng(77)
    for _ in range(20):
        h = np.zeros(BINS, dtype=np.uint64)
        idx = rng.choice(BINS, size=6, replace=False)
        h[idx] = rng.integers(1, 1 << 60, size=6, dtype=np.uint64)
        assert_same_suggestion(ok.suggest_threshold(h), py_suggest(h))


# ---- the rule on the oracle's histograms ------------------------------------------------------------------

@pytest.mark.parametrize("noise_seed", [None, 3])
@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("name,nmsg,nbits", GOLDENS)
def test_suggested_threshold_decodes_the_golden_captures(oracle, vectors, name, nmsg, nbits, scale, noise_seed):
    g, iq = scaled_golden(vectors, name, scale, noise_seed)
    of = oracle.load_filter_json(golden_path("filters", g["filter"]))
    h = np_hist(oracle_power(oracle, of, iq))
    assert int(h.sum()) == g["num_samples"] // of.total_decimation
    s = ok.suggest_threshold(h)
    assert_same_suggestion(s, py_suggest(h))
    print(name, scale, noise_seed, s)
    assert s["found"] == 1
    assert s["off_level"] < s["threshold"] < s["on_level"]
    got = _decode(oracle, g, iq, s["threshold"])
    assert len(got.err_samples) == 0
    assert [got.payload_bits(i, nbits) for i in range(len(got.msg_samples))] == [g["survey"]["payload_bits"]] * nmsg
    if noise_seed is not None and scale <= 1 / 8:
        # the point of the feature: the reference's default threshold decodes nothing here
        assert len(_decode(oracle, g, iq, 0.1).msg_samples) == 0


def test_separation_constants_are_the_measured_ones(oracle, vectors):
    """the two measurements OOKD_LEVEL_MIN_SEPARATION is placed between (header)"""
    g, iq = scaled_golden(vectors, "G1", 1 / 16, 3)
    of = oracle.load_filter_json(golden_path("filters", g["filter"]))
    s = ok.suggest_threshold(np_hist(oracle_power(oracle, of, iq)))
    assert s["on_bin"] - s["off_bin"] == 26
    for amp in (5, 40, 1000):
        noise = np.random.default_rng(amp).integers(-amp, amp + 1, size=2 * g["num_samples"]).astype(np.int16)
        s = ok.suggest_threshold(np_hist(oracle_power(oracle, of, noise)))
        assert 10 <= s["on_bin"] - s["off_bin"] <= 12 < ok.LEVEL_MIN_SEPARATION < 26


@pytest.mark.parametrize("name", ["G1", "G2"])
def test_captures_without_two_levels(oracle, vectors, name):
    g = vectors[name]
    n = g["num_samples"]
    of = oracle.load_filter_json(golden_path("filters", g["filter"]))
    rng = np.random.default_rng(21)
    noise = rng.integers(-40, 41, size=2 * n).astype(np.int16)
    zeros = np.zeros(2 * n, dtype=np.int16)
    carrier = zeros.copy()
    carrier[0::2] = 1945
    for label, iq in (("noise", noise), ("zeros", zeros), ("carrier", carrier), ("noisy carrier", carrier + noise)):
        for fir in (of, None):
            h = np_hist(oracle_power(oracle, fir, iq))
            s = ok.suggest_threshold(h)
            assert_same_suggestion(s, py_suggest(h))
            assert s["found"] == 0 and s["threshold"] == 0.0, (label, fir is not None, s)


def test_quiet_cs8_fixture_decodes_on_the_oracle(oracle, vectors):
    """what tests/test_gpu_survey.py sends through Survey -> suggest_threshold -> Receiver, on the oracle alone"""
    g, v8 = quiet_cs8(vectors)
    assert 7 <= v8.max() <= 10 and v8.min() == -3
    iq = v8.astype(np.int16) * 16                               # the widening rule
    of = oracle.load_filter_json(golden_path("filters", g["filter"]))
    s = ok.suggest_threshold(np_hist(oracle_power(oracle, of, iq)))
    assert s["found"] == 1 and s["threshold"] < 0.1
    got = _decode(oracle, g, iq, s["threshold"])
    assert len(got.err_samples) == 0
    assert [got.payload_bits(i, 36) for i in range(len(got.msg_samples))] == [g["survey"]["payload_bits"]] * 3
    assert len(_decode(oracle, g, iq, 0.1).msg_samples) == 0


def test_survey_fails_loudly_without_a_gpu_or_on_bad_flags(built_lib):
    both = ok.RX_SAMPLES_CS8 | ok.RX_SAMPLES_CU8
    assert not built_lib.ookd_survey_create(0, None, both, 1, None)
    assert "sample_flags" in ok.last_error()
    assert not built_lib.ookd_survey_create(0, None, 1, 1, None)      # a bit that is no sample format
    assert not built_lib.ookd_survey_create(0, None, 0, 0, None)
    assert "max_captures" in ok.last_error()
    h = built_lib.ookd_survey_create(-1, None, 0, 1, None)
    assert not h and "no CPU fallback" in ok.last_error()
