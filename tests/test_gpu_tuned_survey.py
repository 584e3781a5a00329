"""The tuned envelope survey on an MI355X.  Equality means all 256 counts and `samples`: the GPU's histogram against
the numpy restatement of the contract (tests/tuned_survey_contract.py), the register-blocked form against the
generic one, for every tap count around the chunk of 16, the three sample formats, awkward lengths, batches with
odd strides, captures that are not 16-byte aligned, a capture beyond 2^32 samples, and the feature end to end:
Spectrum -> suggest_carriers -> Survey(tune=) -> suggest_threshold -> Receiver(tune=, threshold=) in Python and
through examples/ookd_scan.c."""
import json
import subprocess

import numpy as np
import pytest

from tests.helpers import golden_path
from tests.spectrum_contract import N as SPEC_N, two_transmitters
from tests.tuned_contract import RATE, SPB, contract_rx, golden_capture, lib_stages, moved, to_8bit
from tests.tuned_survey_contract import DC, NOISE, contract_hist, oracle_device

pytestmark = pytest.mark.gpu

NUS = (0.2, -0.3, 1.0 / 3000.0, 0.5)
FORMATS = ("sc16q11", "cs8", "cu8")


@pytest.fixture(scope="module")
def ok():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from ookiedokie_amd import build as okbuild
    okbuild.build()
    import ookiedokie_amd as okm
    okm.lib()
    return okm


def _rand_taps(ntaps, seed):
    h = np.random.default_rng(1000 + seed).normal(0, 1, ntaps)
    return [float(t) for t in h / np.abs(h).sum()]


def _shape(name):
    """-> [(decimation, taps)], the form a tuned survey of it takes"""
    if name.startswith("t"):
        nt = int(name[1:])
        return [(1, _rand_taps(nt, nt))], (3 if nt <= 256 else 2)
    with open(golden_path("filters", name)) as f:
        st = [(s.get("decimation", 1), s["taps"]) for s in json.load(f)["filter"]["stages"]]
    return st, (3 if len(st) == 1 and st[0][0] == 1 else 2)


def _capture(rng, n):
    """half nominal noise, half full range"""
    iq = rng.integers(-2048, 2048, size=2 * n).astype(np.int16)
    iq[2 * (n // 2):] = rng.integers(-32768, 32768, size=2 * (n - n // 2)).astype(np.int16)
    return iq


def _as8(iq16, fmt):
    v = (iq16 >> 8).astype(np.int8)                             # the full byte range
    return v if fmt == "cs8" else (v.astype(np.int16) + 128).astype(np.uint8)


def _widen(x, fmt):
    return ((x.astype(np.int16) - (0 if fmt == "cs8" else 128)) * 16).astype(np.int16)


def _check(sv, got, want, samples, what=None):
    assert got.dtype == np.uint64 and got.shape == (256,)
    assert sv.samples == samples == int(got.sum()), what
    assert np.array_equal(got, want), (what, [(int(b), int(got[b]), int(want[b])) for b in np.nonzero(got != want)[0][:8]])


# ----------------------------------------------------------------------------- 1. nu = 0 ----

@pytest.mark.parametrize("shape", ["fs32_fs4", "fs128_fs16_dec4"])
def test_nu_0_is_the_untuned_survey(ok, shape):
    st, _ = _shape(shape)
    flt = ok.Filter.from_stages(st)
    iq = _capture(np.random.default_rng(1), 70001)
    plain = ok.Survey(flt)
    want = plain.survey(iq)
    assert plain.form == ok.SURVEY_GENERIC and plain.tune == 0.0
    # ookd_survey_create_tuned with nu = 0 (a Tune is passed); exact alone passes tune = NULL
    for kw in (dict(tune=0.0), dict(tune=0.0, exact=True), dict(exact=True), dict(tune_hz=0.0, sample_rate=RATE)):
        sv = ok.Survey(flt, **kw)
        assert sv.form == ok.SURVEY_GENERIC and sv.tune == 0.0, kw
        _check(sv, sv.survey(iq), want, plain.samples, kw)
        sv.close()
    # tune = NULL through the C entry point itself, with and without OOKD_RX_EXACT_FIR
    import ctypes as C
    L = ok.lib()
    for flags in (0, ok.RX_EXACT_FIR):
        h = L.ookd_survey_create_tuned(0, flt._h, flags, 1, None, None)
        assert h, ok.last_error()
        try:
            assert L.ookd_survey_form(h) == ok.SURVEY_GENERIC and L.ookd_survey_tune(h) == 0.0
            assert L.ookd_survey_host(h, iq.ctypes.data, iq.size // 2) == 0, ok.last_error()
            lh = ok.LevelHist()
            assert L.ookd_survey_get_hist(h, 0, C.byref(lh)) == 0, ok.last_error()
            assert int(lh.samples) == plain.samples
            assert np.array_equal(np.frombuffer(bytes(lh.bins), dtype=np.uint64), want), flags
        finally:
            L.ookd_survey_destroy(h)
    plain.close()


# ----------------------------------------------------------------------------- 2. parity ----

@pytest.mark.parametrize("shape", ["t1", "t15", "t16", "t17", "t32", "t33", "t255", "t256", "t257", "fs128_fs16_dec4"])
def test_both_forms_equal_the_contract(ok, shape):
    st, form = _shape(shape)
    flt = ok.Filter.from_stages(st)
    T = len(st[0][1])
    rng = np.random.default_rng(len(shape) * 1000 + T)
    lengths = sorted({0, 1, T - 1, T, 511, 512, 513, 1031, (1 << 17) + 5})
    caps = []
    for n in lengths:
        iq = _capture(rng, n)
        caps.append((n, {"sc16q11": (iq, iq), "cs8": (_as8(iq, "cs8"), _widen(_as8(iq, "cs8"), "cs8")),
                         "cu8": (_as8(iq, "cu8"), _widen(_as8(iq, "cu8"), "cu8"))}))
    for nu in NUS:
        stages = lib_stages(flt, nu)
        svs = {(fmt, exact): ok.Survey(flt, tune=nu, exact=exact, sample_format=fmt)
               for fmt in FORMATS for exact in (False, True)}
        for (fmt, exact), sv in svs.items():
            assert sv.form == (ok.SURVEY_TUNED_GENERIC if exact else form) and sv.tune == nu
        for n, by_fmt in caps:
            want16 = contract_hist(by_fmt["sc16q11"][1], stages)
            want8 = contract_hist(by_fmt["cs8"][1], stages)     # cu8 holds the same values
            assert (by_fmt["cu8"][1] == by_fmt["cs8"][1]).all()
            for (fmt, exact), sv in svs.items():
                want, samples = want16 if fmt == "sc16q11" else want8
                assert samples == n // flt.total_decimation
                _check(sv, sv.survey(by_fmt[fmt][0]), want, samples, (shape, nu, n, fmt, exact))
        for sv in svs.values():
            sv.close()


# ----------------------------------------------------------------------------- 3. persistent walk ----

def test_more_tiles_than_workgroups(ok):
    st, _ = _shape("fs32_fs4")
    flt = ok.Filter.from_stages(st)
    n = (1 << 21) + 777                                         # 4098 tiles of 512 outputs
    iq = _capture(np.random.default_rng(3), n)
    want, samples = contract_hist(iq, lib_stages(flt, 0.2))
    for exact, form in ((False, ok.SURVEY_TUNED_FIR1), (True, ok.SURVEY_TUNED_GENERIC)):
        sv = ok.Survey(flt, tune=0.2, exact=exact)
        got = sv.survey(iq)
        assert sv.form == form and sv.kernel_ms > 0.0
        _check(sv, got, want, samples, exact)
        sv.close()


@pytest.mark.parametrize("shape", ["8x1", "8x2", "8x4", "16x1", "16x2", "16x4"])
def test_every_register_blocked_shape(ok, monkeypatch, shape):
    """The six shapes (outputs per lane x waves per workgroup) the rate tool sweeps through the developer variable:
    each gives the contract's histogram, as the default 8x4 does -- 32 taps and 33 (padded to three chunks), a
    ragged last tile, more tiles than one workgroup has waves, 16-bit and 8-bit, aligned and not."""
    import torch
    monkeypatch.setenv("OOKD_DEVELOPER", "1")
    monkeypatch.setenv("OOKD_SURVEY_TUNED_SHAPE", shape)
    n, nu = 70001, -0.3
    iq = _capture(np.random.default_rng(8), n + 1)
    for name in ("fs32_fs4", "t33"):
        st, _ = _shape(name)
        flt = ok.Filter.from_stages(st)
        stages = lib_stages(flt, nu)
        for fmt in ("sc16q11", "cs8"):
            raw = iq if fmt == "sc16q11" else _as8(iq, fmt)
            wide = iq if fmt == "sc16q11" else _widen(raw, fmt)
            buf = torch.from_numpy(raw).cuda()
            sv = ok.Survey(flt, tune=nu, sample_format=fmt)
            ex = ok.Survey(flt, tune=nu, sample_format=fmt, exact=True)
            assert sv.form == ok.SURVEY_TUNED_FIR1 and ex.form == ok.SURVEY_TUNED_GENERIC
            for lead in (0, 1):                                 # one sample in: no longer 16-byte aligned
                want, samples = contract_hist(wide[2 * lead:2 * (lead + n)], stages)
                for s in (sv, ex):
                    s.survey_device(buf.data_ptr() + 2 * lead * raw.itemsize, n)
                    _check(s, s.hist(), want, samples, (shape, name, fmt, lead, s.form))
            sv.close()
            ex.close()
    monkeypatch.setenv("OOKD_SURVEY_TUNED_SHAPE", "12x3")
    with pytest.raises(ok.OokdError, match="OOKD_SURVEY_TUNED_SHAPE"):
        ok.Survey(flt, tune=nu)


# ----------------------------------------------------------------------------- 4. extremes ----

def test_extremes(ok):
    st, _ = _shape("fs32_fs4")
    flt = ok.Filter.from_stages(st)
    nu = 0.2
    n = 20001
    rng = np.random.default_rng(4)
    k = np.arange(n)
    tone = np.empty(2 * n, np.int16)
    tone[0::2] = np.clip(np.rint(32767 * np.cos(2 * np.pi * ((nu * k) % 1.0))), -32768, 32767)
    tone[1::2] = np.clip(np.rint(32767 * np.sin(2 * np.pi * ((nu * k) % 1.0))), -32768, 32767)
    gaps = rng.integers(-300, 301, size=2 * n).astype(np.int16)
    for a in range(1000, n - 3000, 4000):
        gaps[2 * a:2 * (a + 2500)] = 0                          # far longer than the 32 taps: outputs exactly 0
    cases = {"zeros": np.zeros(2 * n, np.int16), "floor": np.full(2 * n, -32768, np.int16), "tone": tone, "gaps": gaps}
    svs = [ok.Survey(flt, tune=nu), ok.Survey(flt, tune=nu, exact=True)]
    stages = lib_stages(flt, nu)
    for name, iq in cases.items():
        want, samples = contract_hist(iq, stages)
        for sv in svs:
            _check(sv, sv.survey(iq), want, samples, name)
        if name == "zeros":
            assert int(want[0]) == n
        if name == "gaps":
            assert int(want[0]) > 4 * 2400
        if name == "tone":
            # the filter tuned to the tone passes it: amplitude 16, power 256, for all but the start-up ramp
            assert int(want[ok.level_bin(200.0):].sum()) > n - 64
    for sv in svs:
        sv.close()
    # taps that drive every power into bin 255 -- finite, and through inf and NaN
    iq = _capture(rng, n)
    iq[iq == 0] = 1
    for scale in (2.0 ** 40, 1e30):
        big = ok.Filter.from_stages([(1, [t * scale for t in st[0][1]])])
        want, samples = contract_hist(iq, lib_stages(big, nu))
        assert int(want[255]) > n - 64
        for exact in (False, True):
            sv = ok.Survey(big, tune=nu, exact=exact)
            _check(sv, sv.survey(iq), want, samples, (scale, exact))
            sv.close()


# ----------------------------------------------------------------------------- 5. batches ----

@pytest.mark.parametrize("fmt", FORMATS)
def test_batches_strides_alignment_and_reuse(ok, fmt):
    import torch
    st, _ = _shape("fs32_fs4")
    flt = ok.Filter.from_stages(st)
    nu = -0.3
    stages = lib_stages(flt, nu)
    rng = np.random.default_rng(5)
    ncap, n, stride, lead = 3, 5000, 5003, (1 if fmt != "sc16q11" else 0)
    caps16 = [_capture(rng, n) for _ in range(ncap)]
    raws = [c if fmt == "sc16q11" else _as8(c, fmt) for c in caps16]
    wide = [c if fmt == "sc16q11" else _widen(r, fmt) for c, r in zip(caps16, raws)]
    host = np.full(2 * (lead + stride * ncap), 77, dtype=raws[0].dtype)     # the gaps hold a level: never counted
    for c, r in enumerate(raws):
        host[2 * (lead + stride * c):2 * (lead + stride * c + n)] = r
    buf = torch.from_numpy(host).cuda()
    first = buf.data_ptr() + 2 * lead * host.itemsize           # 8-bit: the batch starts at an odd sample
    wants = [contract_hist(w, stages) for w in wide]
    for exact, form in ((False, ok.SURVEY_TUNED_FIR1), (True, ok.SURVEY_TUNED_GENERIC)):
        sv = ok.Survey(flt, tune=nu, exact=exact, max_captures=ncap, sample_format=fmt)
        sv.survey_device(first, n, num_captures=ncap, stride=stride)
        # unaligned captures are read sample by sample by the same kernel: the form does not change
        assert sv.form == form
        hists = [sv.hist(c) for c in range(ncap)]
        for c in range(ncap):
            _check(sv, hists[c], wants[c][0], wants[c][1], (exact, c))
        sv.survey_device(first, n, num_captures=ncap, stride=stride)
        assert all(np.array_equal(sv.hist(c), hists[c]) for c in range(ncap))    # two runs are identical
        m = 1237                                                # a second, shorter run replaces them
        sv.survey_device(first, m, num_captures=2, stride=stride)
        for c in range(2):
            want, samples = contract_hist(wide[c][:2 * m], stages)
            _check(sv, sv.hist(c), want, samples, (exact, c, m))
        with pytest.raises(ok.OokdError):
            sv.hist(2)
        sv.close()


# ----------------------------------------------------------------------------- 6. beyond 2^32 ----

def test_capture_beyond_32_bit_indices(ok):
    """2^32 + 70001 CS8 samples built on the device from a period of 2^16 + 3 samples.  Behind the first period
    the outputs repeat with the capture, so the histogram is the first period's (with the start-up ramp) plus
    whole steady periods plus a steady rest, all taken from the contract on two periods."""
    import torch
    torch.cuda.empty_cache()
    free, _ = torch.cuda.mem_get_info()
    if free < 12 * (1 << 30):
        pytest.skip("needs 12 GiB of free HBM, the card has %.0f" % (free / (1 << 30)))
    st, _ = _shape("fs32_fs4")
    flt = ok.Filter.from_stages(st)
    nu = 0.2
    P = (1 << 16) + 3
    n = (1 << 32) + 70001
    period16 = _capture(np.random.default_rng(6), P)
    period = _as8(period16, "cs8")
    from tests.test_survey_host import np_hist
    from tests.tuned_survey_contract import contract_power
    p2 = contract_power(np.concatenate([_widen(period, "cs8")] * 2), lib_stages(flt, nu))
    reps, rest = divmod(n, P)
    want = np_hist(p2[:P]) + np.uint64(reps - 1) * np_hist(p2[P:]) + np_hist(p2[P:P + rest])
    assert int(want.sum()) == n
    dev_p = torch.from_numpy(period.reshape(-1, 2)).cuda()
    cap = dev_p.repeat(reps + 1, 1)[:n].contiguous()
    assert cap.numel() == 2 * n
    torch.cuda.synchronize()
    for exact, form in ((False, ok.SURVEY_TUNED_FIR1), (True, ok.SURVEY_TUNED_GENERIC)):
        sv = ok.Survey(flt, tune=nu, exact=exact, sample_format="cs8")
        sv.survey_device(cap.data_ptr(), n)
        got = sv.hist()
        print("form", form, "kernel ms", sv.kernel_ms)
        assert sv.form == form
        _check(sv, got, want, n, exact)
        sv.close()


# ----------------------------------------------------------------------------- 7. end to end ----

def _chain(ok, oracle, iq16, raw, fmt, g, want_bin, ref_pay):
    """Spectrum -> suggest_carriers -> Survey(tune) -> suggest_threshold -> Receiver(tune, threshold)"""
    n = raw.size // 2
    flt = ok.Filter.load(golden_path("filters", "fs32_fs4"))
    sp = ok.Spectrum(sample_format=fmt)
    carriers, _ = ok.suggest_carriers(sp.spectrum(raw))
    sp.close()
    car = {c.bin: c for c in carriers if not c.at_dc}[want_bin]
    sv = ok.Survey(flt, tune=car.nu, sample_format=fmt)
    h = sv.survey(raw)
    assert sv.form == ok.SURVEY_TUNED_FIR1
    stages = lib_stages(flt, car.nu)
    want_h, samples = contract_hist(iq16, stages)
    _check(sv, h, want_h, samples)
    sv.close()
    s = ok.suggest_threshold(h)
    print(g["device"], want_bin, fmt, s)
    assert s["found"] == 1
    dev = ok.Device.load(golden_path("devices", g["device"]), RATE)
    rx = ok.Receiver(flt, dev, max_samples=n, tune=car.nu, threshold=s["threshold"], sample_format=fmt)
    got = rx.rx(raw)
    bits, _ = contract_rx(iq16, stages, s["threshold"], SPB)
    ms, pay, es = oracle.sm_stream(oracle_device(oracle, g["device"]), bits, SPB)
    assert list(got.msg_samples) == list(ms)
    assert got.payloads.shape == pay.shape and (got.payloads == pay).all()
    errs, nerr = rx.errors()
    assert nerr == len(es) and list(errs) == list(es)
    assert [bytes(p) for p in pay] == ref_pay
    rx.close()
    return s


def _ref_payloads(ok, oracle, base, g):
    flt = ok.Filter.load(golden_path("filters", "fs32_fs4"))
    bits, _ = contract_rx(base, lib_stages(flt, 0.0), 0.1, SPB)
    _, pay, es = oracle.sm_stream(oracle_device(oracle, g["device"]), bits, SPB)
    assert len(pay) >= 2 and len(es) == 0
    return [bytes(p) for p in pay]


@pytest.mark.parametrize("cap,hz,want_bin", [("G1", 600e3, 205), ("G1", -900e3, -307), ("G2", 600e3, 205),
                                             ("G2", -900e3, -307)])
def test_chain_on_a_moved_quiet_capture(ok, oracle, cap, hz, want_bin):
    base, g = golden_capture(cap)
    iq = moved(base, hz / RATE, DC, NOISE, seed=1, scale=1 / 8)
    s = _chain(ok, oracle, iq, iq, "sc16q11", g, want_bin, _ref_payloads(ok, oracle, base, g))
    assert s["threshold"] < 0.1                                 # where the default hears nothing usable


def test_chain_on_the_cs8_cut(ok, oracle):
    base, g = golden_capture("G1")
    raw, iq16 = to_8bit(moved(base, 600e3 / RATE, DC, NOISE, seed=2), "cs8")
    _chain(ok, oracle, iq16, raw, "cs8", g, 205, _ref_payloads(ok, oracle, base, g))


def test_chain_on_two_transmitters(ok, oracle):
    iq, (b1, g1), (b2, g2) = two_transmitters(seed=2)
    for want_bin, base, g in ((205, b1, g1), (-307, b2, g2)):
        _chain(ok, oracle, iq, iq, "sc16q11", g, want_bin, _ref_payloads(ok, oracle, base, g))


# ----------------------------------------------------------------------------- 8. the C program ----

def _rows(text):
    """stdout rows without the first column: "Decode Timestamp" is the wall clock"""
    return [ln.split(",", 1)[1:] for ln in text.split("\n")]


def test_c_scan_program(ok, tmp_path):
    from tests.test_host import _build_c_example
    from tests.test_tuned_survey_host import build_scan
    scan, rx_exe = build_scan(tmp_path), _build_c_example(tmp_path)
    iq, (_, g1), (_, g2) = two_transmitters(seed=3)
    cap = tmp_path / "two.sc16q11"
    iq.tofile(str(cap))
    filt = golden_path("filters", "fs32_fs4")
    devs = [golden_path("devices", g1["device"]), golden_path("devices", g2["device"])]
    r = subprocess.run([scan, str(cap), str(RATE), filt] + devs + ["csv"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    print(r.stderr)
    assert "carrier %+.6g Hz: at DC, skipped" % 0.0 in r.stderr  # bin 0
    flt = ok.Filter.load(filt)
    blocks = []
    sp = ok.Spectrum()
    carriers, _ = ok.suggest_carriers(sp.spectrum(iq), max_carriers=8)
    sp.close()
    assert sorted(c.bin for c in carriers) == [-307, 0, 205]
    for c in carriers:                                          # in the program's order: decreasing power
        if c.at_dc:
            continue
        hz = c.bin / SPEC_N * RATE
        sv = ok.Survey(flt, tune=c.nu)
        s = ok.suggest_threshold(sv.survey(iq))
        sv.close()
        assert s["found"] == 1
        assert "carrier %+.6g Hz: threshold %.6g (off %.6g, on %.6g)" % (hz, s["threshold"], s["off_level"],
                                                                          s["on_level"]) in r.stderr
        for d in devs:
            one = subprocess.run([rx_exe, "--tune", repr(hz), "--threshold", repr(float(np.float32(s["threshold"]))),
                                  str(cap), d, filt, str(RATE), "csv"], capture_output=True, text=True, timeout=300)
            assert one.returncode == 0, one.stderr
            if one.stdout:
                blocks.append(one.stdout)
    assert len(blocks) >= 2 and r.stderr.count(" messages\n") == len(blocks)
    assert _rows(r.stdout) == _rows("".join(blocks))
    # a still capture: the only peak is the one at DC
    base, _ = golden_capture("G1")
    still = tmp_path / "still.sc16q11"
    moved(base, 0.0, DC, NOISE, seed=2).tofile(str(still))
    none = subprocess.run([scan, str(still), str(RATE), filt] + devs + ["csv"], capture_output=True, text=True,
                          timeout=300)
    assert none.returncode == 0 and none.stdout == "" and "no carrier beside DC" in none.stderr
    assert "at DC, skipped" in none.stderr
