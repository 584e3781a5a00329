"""The envelope survey on an MI355X: every count of the GPU's histogram equals numpy's bincount of the bin rule
over the oracle's filter output -- all filter shapes, the three sample formats, awkward lengths, batches --, a
full-size capture beyond 2^32 samples, and the feature end to end: a quiet CS8 capture the default threshold
cannot decode goes through Survey -> suggest_threshold -> Receiver, in Python and through examples/ookd_rx.c."""
import json
import subprocess

import numpy as np
import pytest

from tests.helpers import golden_path
from tests.test_survey_host import RATE, np_hist, oracle_power, quiet_cs8, scaled_golden

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


def _sinc(ntaps, cutoff):
    k = np.arange(ntaps) - (ntaps - 1) / 2
    h = np.sinc(k / cutoff) * np.hamming(ntaps)
    return h / h.sum()


def _stages(shape):
    """(decimation, taps) per stage, or None for no filter"""
    if shape == "none":
        return None
    if shape in ("fs32_fs4", "fs128_fs16_dec4", "unity16"):
        with open(golden_path("filters", shape)) as f:
            return [(st.get("decimation", 1), st["taps"]) for st in json.load(f)["filter"]["stages"]]
    if shape == "sinc255":
        return [(1, list(_sinc(255, 32.0)))]
    if shape == "three_stage":                                  # decimations 3, 2, 5: no tuned form of any kernel
        return [(3, list(_sinc(21, 3.0))), (2, list(_sinc(9, 2.0))), (5, list(_sinc(40, 5.0)))]
    raise KeyError(shape)


SHAPES = ("none", "fs32_fs4", "fs128_fs16_dec4", "unity16", "sinc255", "three_stage")


def _filters(ok, oracle, shape):
    st = _stages(shape)
    if st is None:
        return None, None
    return ok.Filter.from_stages(st), oracle.make_fir([(d, np.array(t, dtype=np.float64)) for d, t in st])


def _capture(rng, n, loud=False):
    """n samples: silence with noise, bursts of carrier, a stretch of exact zeros (several bins, uneven counts)"""
    iq = rng.integers(-40, 41, size=2 * n).astype(np.int16)
    for start in range(n // 7, n, max(n // 5, 1)):
        iq[2 * start:2 * (start + n // 11)] += np.int16(20000 if loud else 1500)
    iq[2 * (n // 2):2 * (n // 2 + n // 13)] = 0
    return iq


def _as8(iq16, fmt):
    v = (iq16 >> 4).astype(np.int8)
    return v if fmt == "cs8" else (v.astype(np.int16) + 128).astype(np.uint8)


def _widen(x, fmt):
    return ((x.astype(np.int16) - (0 if fmt == "cs8" else 128)) * 16).astype(np.int16)


def _want(oracle, ofir, iq16):
    """(histogram, floor(n / D)) from the oracle"""
    n = iq16.size // 2
    d = ofir.total_decimation if ofir is not None else 1
    h = np_hist(oracle_power(oracle, ofir, iq16))
    assert int(h.sum()) == n // d
    return h, n // d


def _check(sv, got, want, samples):
    assert got.dtype == np.uint64 and got.shape == (256,)
    assert sv.samples == samples == int(got.sum())
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, [(int(b), int(got[b]), int(want[b])) for b in bad[:8]]


@pytest.mark.parametrize("shape", SHAPES)
def test_histogram_equals_the_oracle_for_every_shape_and_format(ok, oracle, shape):
    """lengths that are no multiple of the tile or of D, shorter than the tap count, one sample, none"""
    flt, ofir = _filters(ok, oracle, shape)
    rng = np.random.default_rng(SHAPES.index(shape))
    sv = {fmt: ok.Survey(flt, sample_format=fmt) for fmt in ("sc16q11", "cs8", "cu8")}
    for n in (100003, 4097, 1024, 31, 7, 1, 0):
        iq = _capture(rng, n)
        want, samples = _want(oracle, ofir, iq)
        _check(sv["sc16q11"], sv["sc16q11"].survey(iq), want, samples)
        for fmt in ("cs8", "cu8"):
            x = _as8(iq, fmt)
            w = _widen(x, fmt)
            want8, samples8 = _want(oracle, ofir, w)
            got8 = sv[fmt].survey(x)
            _check(sv[fmt], got8, want8, samples8)
            # the 8-bit result is the SC16Q11 result on the widened capture
            assert (got8 == sv["sc16q11"].survey(w)).all()
    for s in sv.values():
        s.close()


@pytest.mark.parametrize("shape", ["none", "fs32_fs4", "fs128_fs16_dec4"])
def test_extreme_values_and_silence(ok, oracle, shape):
    flt, ofir = _filters(ok, oracle, shape)
    sv = ok.Survey(flt)
    n = 20001
    for value in (32767, -32768):
        iq = np.full(2 * n, value, dtype=np.int16)
        iq[1::4] = -value if value > 0 else 32767            # both signs on the Q rail
        want, samples = _want(oracle, ofir, iq)
        got = sv.survey(iq)
        _check(sv, got, want, samples)
        # full scale is 16: the I rail alone carries a power of 256 through these unity-gain low-passes
        assert int(np.nonzero(got)[0].max()) >= ok.level_bin(128.0)
    zeros = np.zeros(2 * n, dtype=np.int16)
    got = sv.survey(zeros)
    assert int(got[0]) == sv.samples == n // (flt.total_decimation if flt else 1) and int(got[1:].sum()) == 0
    sv.close()


def test_batch_with_a_stride_and_repeat_runs_on_one_handle(ok, oracle):
    import torch
    flt, ofir = _filters(ok, oracle, "fs128_fs16_dec4")
    rng = np.random.default_rng(99)
    ncap, n, stride = 5, 50001, 50001 + 77
    caps = [_capture(rng, n, loud=(c == 3)) for c in range(ncap)]
    host = np.full(2 * stride * ncap, 12345, dtype=np.int16)       # the gaps hold a loud level: never counted
    for c, iq in enumerate(caps):
        host[2 * stride * c:2 * stride * c + 2 * n] = iq
    buf = torch.from_numpy(host).cuda()
    sv = ok.Survey(flt, max_captures=ncap)
    sv.survey_device(buf.data_ptr(), n, num_captures=ncap, stride=stride)
    for c, iq in enumerate(caps):
        want, samples = _want(oracle, ofir, iq)
        _check(sv, sv.hist(c), want, samples)
    assert sv.kernel_ms > 0.0
    # a second, shorter run on the same handle leaves nothing behind from the first
    m = 1237
    sv.survey_device(buf.data_ptr(), m, num_captures=2, stride=stride)
    for c in range(2):
        want, samples = _want(oracle, ofir, caps[c][:2 * m])
        _check(sv, sv.hist(c), want, samples)
    with pytest.raises(ok.OokdError):
        sv.hist(2)                                              # not part of the last run
    with pytest.raises(ok.OokdError):
        sv.survey_device(buf.data_ptr(), n, num_captures=ncap + 1, stride=stride)
    sv.survey_device(buf.data_ptr(), 3, num_captures=1)         # fewer samples than the decimation: nothing to count
    assert sv.hist(0).sum() == 0 and sv.samples == 0
    sv.close()


def test_full_size_capture_beyond_32_bit_indices(ok, oracle):
    """2^32 + 4099 synthesised samples: the counts sum to floor(n / D), and on a 2^24-sample prefix the
    histogram is the oracle's.  Skipped only when the card lacks the memory (tests/test_gpu_fullsize.py's gate)."""
    import torch
    torch.cuda.empty_cache()
    free, _ = torch.cuda.mem_get_info()
    if free < 24 * (1 << 30):
        pytest.skip("needs 24 GiB of free HBM, the card has %.0f" % (free / (1 << 30)))
    n = (1 << 32) + 4099
    dev = ok.Device.load(golden_path("devices", "p3l-nexa2012"), RATE)
    syn = ok.Synth(dev, n, seed=0x5EED, sample_rate=RATE)
    cap = torch.empty(2 * n + 64, dtype=torch.int16, device="cuda")
    syn.fill_device(cap.data_ptr())
    torch.cuda.synchronize()
    for shape in ("fs32_fs4", "fs128_fs16_dec4"):
        flt, ofir = _filters(ok, oracle, shape)
        sv = ok.Survey(flt)
        sv.survey_device(cap.data_ptr(), n)
        h = sv.hist()
        assert sv.samples == n // flt.total_decimation == int(h.sum(dtype=np.uint64))
        s = ok.suggest_threshold(h)
        print(shape, "kernel ms", sv.kernel_ms, s)
        assert s["found"] == 1 and 0.3 < s["threshold"] < 0.6      # on level 1945 LSB = 0.95, off = +-40 LSB of noise
        m = 1 << 24
        sv.survey_device(cap.data_ptr(), m)
        prefix = cap[:2 * m].cpu().numpy()
        want, samples = _want(oracle, ofir, prefix)
        _check(sv, sv.hist(), want, samples)
        sv.close()
    # captures that START beyond the 32-bit sample range: a batch of two, a stride of 2^32 + 64 samples apart
    m, off = 4035, (1 << 32) + 64
    cap[2 * off:2 * (off + m)].copy_(cap[2 * 1000:2 * (1000 + m)])
    flt, ofir = _filters(ok, oracle, "fs128_fs16_dec4")
    sv = ok.Survey(flt, max_captures=2)
    sv.survey_device(cap.data_ptr(), m, num_captures=2, stride=off)
    for c, first in ((0, 0), (1, 1000)):
        want, samples = _want(oracle, ofir, prefix[2 * first:2 * (first + m)])
        _check(sv, sv.hist(c), want, samples)
    sv.close()
    # samples READ beyond the 32-bit range: without a filter a histogram is the sum of its parts', and each part
    # is surveyed with small indices
    sv = ok.Survey(None)
    sv.survey_device(cap.data_ptr(), n)
    whole = sv.hist()
    assert sv.samples == n
    parts = np.zeros(256, dtype=np.uint64)
    step = (1 << 31) - 5
    for first in range(0, n, step):
        sv.survey_device(cap.data_ptr() + 4 * first, min(step, n - first))
        parts += sv.hist()
    assert (whole == parts).all()
    sv.close()


def test_quiet_cs8_capture_end_to_end(ok, oracle, vectors):
    g, v8 = quiet_cs8(vectors)
    n = v8.size // 2
    flt = ok.Filter.load(golden_path("filters", g["filter"]))
    dev = ok.Device.load(golden_path("devices", g["device"]), RATE)
    sv = ok.Survey(flt, sample_format="cs8")
    h = sv.survey(v8)
    ofir = oracle.load_filter_json(golden_path("filters", g["filter"]))
    want, samples = _want(oracle, ofir, v8.astype(np.int16) * 16)
    _check(sv, h, want, samples)
    s = ok.suggest_threshold(h)
    assert s["found"] == 1 and s["threshold"] < 0.1
    rx = ok.Receiver(flt, dev, max_samples=n, threshold=s["threshold"], samples_per_buffer=g["spb"], sample_format="cs8")
    got = rx.rx(v8)
    assert [got.payload_bits(i, 36) for i in range(len(got.msg_samples))] == [g["survey"]["payload_bits"]] * 3
    assert got.stats["num_errors"] == 0
    rx.close()
    deaf = ok.Receiver(flt, dev, max_samples=n, samples_per_buffer=g["spb"], sample_format="cs8")
    assert len(deaf.rx(v8).msg_samples) == 0                    # the default threshold hears nothing
    deaf.close()
    sv.close()


def test_c_example_threshold_auto(ok, vectors, tmp_path):
    from tests.test_host import _build_c_example
    exe = _build_c_example(tmp_path)
    g, v8 = quiet_cs8(vectors)
    cap = tmp_path / "quiet.cs8"
    v8.tofile(str(cap))
    flt = ok.Filter.load(golden_path("filters", g["filter"]))
    sv = ok.Survey(flt, sample_format="cs8")
    s = ok.suggest_threshold(sv.survey(v8))
    sv.close()
    args = [str(cap), golden_path("devices", g["device"]), golden_path("filters", g["filter"]), str(RATE), "csv"]
    auto = subprocess.run([exe, "--threshold", "auto"] + args, capture_output=True, text=True, timeout=120)
    assert auto.returncode == 0, auto.stderr
    assert "threshold auto: %.6g" % s["threshold"] in auto.stderr
    fixed = subprocess.run([exe] + args + ["--threshold", repr(float(np.float32(s["threshold"])))],
                           capture_output=True, text=True, timeout=120)
    assert fixed.returncode == 0, fixed.stderr
    # the same rows, but for the value of the first column: "Decode Timestamp" is the wall clock
    rows, rows_fixed = auto.stdout.split("\n"), fixed.stdout.split("\n")
    assert rows[0] == rows_fixed[0] and rows[0].startswith("Decode Timestamp,") and len(rows) == len(rows_fixed) == 5
    assert [ln.split(",", 1)[1:] for ln in rows[1:]] == [ln.split(",", 1)[1:] for ln in rows_fixed[1:]]
    assert [ln.split(",", 1)[1] for ln in rows[1:4]] == ["0x27,0xd5,2,21.500,70.700,0x00"] * 3
    # the default behaves as before: 0.1 decodes nothing of this capture
    plain = subprocess.run([exe] + args, capture_output=True, text=True, timeout=120)
    assert plain.returncode == 0 and "0x27" not in plain.stdout
    # no two levels: says so, decodes nothing, exits non-zero
    silence = tmp_path / "silence.cs8"
    np.random.default_rng(5).integers(-3, 3, size=2 * 200000).astype(np.int8).tofile(str(silence))
    args[0] = str(silence)
    none = subprocess.run([exe, "--threshold", "auto"] + args, capture_output=True, text=True, timeout=120)
    assert none.returncode != 0 and none.stdout == "" and "no two envelope levels" in none.stderr
