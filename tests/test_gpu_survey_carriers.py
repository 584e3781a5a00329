"""The carriers survey on an MI355X: several carriers in one pass, every S-th output counted.  Equality means all
256 counts and `samples`: the GPU's histograms against the numpy restatement of the contract
(tests/survey_carriers_contract.py) for every tap count around the chunk of 16, every kernel instantiation (strides
1, 2, 4 and >= 8), 1 .. 16 carriers, awkward lengths, the three sample formats, batches with odd strides, captures
that are not 16-byte aligned; at stride 1 against the single tuned surveys and the generic form; the shapes without
the multi form; a capture beyond 2^32 samples; and the feature end to end, in Python and through
examples/ookd_scan.c."""
import json
import subprocess

import numpy as np
import pytest

from tests.helpers import golden_path
from tests.spectrum_contract import two_transmitters
from tests.test_survey_host import np_hist
from tests.tuned_contract import RATE, SPB, contract_rx, lib_stages
from tests.tuned_survey_contract import contract_power, oracle_device

pytestmark = pytest.mark.gpu

FORMATS = ("sc16q11", "cs8", "cu8")
NUS16 = [0.0, 0.5, -0.5, 0.2, 0.2, -0.3, 1.0 / 3000.0, 0.11, -0.07, 0.33, -0.41, 0.25, -0.125, 0.4999, -0.0003, 0.05]
CARRIER_SETS = {1: [0.2], 2: [0.0, -0.5], 5: [0.5, 0.2, -0.3, 0.2, 1.0 / 3000.0], 16: NUS16}


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


def _golden_stages(name):
    with open(golden_path("filters", name)) as f:
        return [(s.get("decimation", 1), s["taps"]) for s in json.load(f)["filter"]["stages"]]


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


def _power(iq16, flt, nu):
    with np.errstate(over="ignore", invalid="ignore"):
        return contract_power(iq16, lib_stages(flt, nu))


def _check(sv, got, p, S, what=None):
    """one carrier's counts against the contract's power p of every output"""
    want = np_hist(p[::S])
    samples = -(-p.size // S)
    assert got.dtype == np.uint64 and got.shape == (256,)
    assert sv.samples == samples == int(got.sum()), (what, sv.samples, samples, int(got.sum()))
    assert np.array_equal(got, want), (what, [(int(b), int(got[b]), int(want[b])) for b in np.nonzero(got != want)[0][:8]])


# ----------------------------------------------------------------------------- 1. the contract ----

@pytest.mark.parametrize("ntaps", [1, 15, 16, 17, 32, 33, 255, 256])
def test_equals_the_contract(ok, ntaps):
    flt = ok.Filter.from_stages([(1, _rand_taps(ntaps, ntaps))])
    rng = np.random.default_rng(ntaps)
    strides = (1, 2, 8, 64)
    lengths = sorted({0, 1, 511, 512, 513, 3 * 512 + 5, max(ntaps - 1, 0), ntaps} |
                     {n for S in strides for n in (S - 1, S, S + 1)})
    caps = {n: _capture(rng, n) for n in lengths}
    power = {(nu, n): _power(caps[n], flt, nu) for nu in set(NUS16) for n in lengths}
    for K, nus in CARRIER_SETS.items():
        for S in strides:
            sv = ok.Survey(flt, carriers=nus, stride=S)
            assert sv.form == ok.SURVEY_TUNED_MULTI and sv.num_carriers == K and sv.stride == S
            assert sv.tune == nus[0]
            for n in lengths:
                hists = sv.survey(caps[n])
                assert hists.shape == (K, 256)
                for k, nu in enumerate(nus):
                    _check(sv, hists[k], power[nu, n], S, (ntaps, K, S, n, k))
                assert np.array_equal(sv.hist(), hists[0])      # ookd_survey_get_hist: carrier 0
            sv.close()


def test_stride_4(ok):
    """the one kernel instantiation (two counted outputs per lane) the strides above do not reach"""
    flt = ok.Filter.from_stages([(1, _rand_taps(33, 4))])
    iq = _capture(np.random.default_rng(44), 70001)
    nus = [0.2, 0.0, -0.3]
    sv = ok.Survey(flt, carriers=nus, stride=4)
    hists = sv.survey(iq)
    for k, nu in enumerate(nus):
        _check(sv, hists[k], _power(iq, flt, nu), 4, k)
    sv.close()


@pytest.mark.parametrize("R", ["8", "16", "32", "64"])
def test_both_window_shapes(ok, monkeypatch, R):
    """8, 16, 32 and 64 output positions per lane (the developer variable the rate tool compares them with), every
    stride each exists for: 33 taps (padded to three chunks), a ragged last tile, more tiles than one workgroup has waves, 16-bit and 8-bit"""
    monkeypatch.setenv("OOKD_DEVELOPER", "1")
    monkeypatch.setenv("OOKD_SURVEY_MULTI_R", R)
    flt = ok.Filter.from_stages([(1, _rand_taps(33, 5))])
    iq = _capture(np.random.default_rng(45), 70001)
    nus = [0.2, 0.0, -0.3]
    for fmt in ("sc16q11", "cs8"):
        raw = iq if fmt == "sc16q11" else _as8(iq, fmt)
        wide = iq if fmt == "sc16q11" else _widen(raw, fmt)
        power = [_power(wide, flt, nu) for nu in nus]
        for S in (1, 2, 4, 8, 16, 32, 64):
            if int(R) >= 32 and S < int(R):                      # the large windows: one counted output per lane
                with pytest.raises(ok.OokdError, match="OOKD_SURVEY_MULTI_R"):
                    ok.Survey(flt, carriers=nus, stride=S, sample_format=fmt)
                continue
            sv = ok.Survey(flt, carriers=nus, stride=S, sample_format=fmt)
            hists = sv.survey(raw)
            for k in range(3):
                _check(sv, hists[k], power[k], S, (R, fmt, S, k))
            sv.close()
    monkeypatch.setenv("OOKD_SURVEY_MULTI_R", "12")
    with pytest.raises(ok.OokdError, match="OOKD_SURVEY_MULTI_R"):
        ok.Survey(flt, carriers=nus)


# ----------------------------------------------------------------------------- 2. persistent walk ----

def test_more_tiles_than_workgroups(ok):
    flt = ok.Filter.from_stages(_golden_stages("fs32_fs4"))
    n = (1 << 21) + 777                                         # 4098 tiles of 512 outputs
    iq = _capture(np.random.default_rng(3), n)
    nus = [0.2, -0.3, 0.0]
    sv = ok.Survey(flt, carriers=nus, stride=8)
    hists = sv.survey(iq)
    assert sv.form == ok.SURVEY_TUNED_MULTI and sv.kernel_ms > 0.0
    for k, nu in enumerate(nus):
        _check(sv, hists[k], _power(iq, flt, nu), 8, k)
    sv.close()


# ----------------------------------------------------------------------------- 3. formats and batches ----

@pytest.mark.parametrize("fmt", FORMATS)
def test_formats_batches_strides_and_alignment(ok, fmt):
    import torch
    flt = ok.Filter.from_stages(_golden_stages("fs32_fs4"))
    nus = [-0.3, 0.0, 0.2]
    rng = np.random.default_rng(5)
    ncap, n, cstride, lead = 3, 5000, 5003, (1 if fmt != "sc16q11" else 0)
    caps16 = [_capture(rng, n) for _ in range(ncap)]
    raws = [c if fmt == "sc16q11" else _as8(c, fmt) for c in caps16]
    wide = [c if fmt == "sc16q11" else _widen(r, fmt) for c, r in zip(caps16, raws)]
    host = np.full(2 * (lead + cstride * ncap), 77, dtype=raws[0].dtype)    # the gaps hold a level: never counted
    for c, r in enumerate(raws):
        host[2 * (lead + cstride * c):2 * (lead + cstride * c + n)] = r
    buf = torch.from_numpy(host).cuda()
    first = buf.data_ptr() + 2 * lead * host.itemsize           # 8-bit: the batch starts at an odd sample
    power = [[_power(w, flt, nu) for nu in nus] for w in wide]
    for S in (1, 8):
        sv = ok.Survey(flt, carriers=nus, stride=S, max_captures=ncap, sample_format=fmt)
        sv.survey_device(first, n, num_captures=ncap, stride=cstride)
        # unaligned captures are read sample by sample by the same kernel: the form does not change
        assert sv.form == ok.SURVEY_TUNED_MULTI
        hists = [[sv.hist(c, k) for k in range(3)] for c in range(ncap)]
        for c in range(ncap):
            for k in range(3):                                  # the layout: per capture, per carrier
                _check(sv, hists[c][k], power[c][k], S, (fmt, S, c, k))
        sv.survey_device(first, n, num_captures=ncap, stride=cstride)
        assert all(np.array_equal(sv.hist(c, k), hists[c][k]) for c in range(ncap) for k in range(3))
        m = 1237                                                # a second, shorter run replaces them
        sv.survey_device(first, m, num_captures=2, stride=cstride)
        for c in range(2):
            for k in range(3):
                _check(sv, sv.hist(c, k), power[c][k][:m], S, (fmt, S, c, k, m))
        with pytest.raises(ok.OokdError):
            sv.hist(2, 0)
        with pytest.raises(ok.OokdError):
            sv.hist(0, 3)
        sv.close()
    # one aligned 8-bit (or 16-bit) capture, read in place with 16-byte loads
    one = torch.from_numpy(raws[0]).cuda()
    sv = ok.Survey(flt, carriers=nus, stride=2, sample_format=fmt)
    sv.survey_device(one.data_ptr(), n)
    for k in range(3):
        _check(sv, sv.hist(0, k), power[0][k], 2, (fmt, "aligned", k))
    sv.close()


# ----------------------------------------------------------------------------- 4. extremes ----

def test_extremes(ok):
    """taps of 1e15 and 1e-15 on full-scale samples, and taps that drive the power through inf and NaN: the order of
    the roundings is the contract's, so the counts are"""
    st = _golden_stages("fs32_fs4")
    n = 20001
    rng = np.random.default_rng(4)
    full = rng.choice(np.array([-32768, 32767], np.int16), size=2 * n)
    noise = _capture(rng, n)
    noise[noise == 0] = 1
    nus = [0.2, 0.0, -0.5]
    for scale, iq in ((1e15, full), (1e-15, full), (2.0 ** 40, noise), (1e30, noise)):
        flt = ok.Filter.from_stages([(1, [t * scale for t in st[0][1]])])
        power = [_power(iq, flt, nu) for nu in nus]
        if scale == 1e30:
            assert not np.isfinite(power[0]).all()
        for S in (1, 8):
            sv = ok.Survey(flt, carriers=nus, stride=S)
            hists = sv.survey(iq)
            for k in range(3):
                _check(sv, hists[k], power[k], S, (scale, S, k))
            sv.close()


# ----------------------------------------------------------------------------- 5. stride 1 against the singles ----

def _singles(ok, flt, nus, iq, **kw):
    out = []
    for nu in nus:
        one = ok.Survey(flt, tune=nu, **kw)
        out.append((one.survey(iq), one.samples))
        one.close()
    return out


def test_stride_1_equals_the_single_surveys_and_the_generic_form(ok):
    flt = ok.Filter.from_stages(_golden_stages("fs32_fs4"))
    iq = _capture(np.random.default_rng(9), 70001)
    nus = [0.2, -0.3, 0.0, 0.5, 0.2]
    singles = _singles(ok, flt, nus, iq)
    for exact, form in ((False, ok.SURVEY_TUNED_MULTI), (True, ok.SURVEY_TUNED_GENERIC)):
        sv = ok.Survey(flt, carriers=nus, exact=exact)
        assert sv.form == form and sv.stride == 1 and sv.num_carriers == 5
        hists = sv.survey(iq)
        assert sv.kernel_ms > 0.0
        for k in range(5):
            assert sv.samples == singles[k][1] == int(hists[k].sum())
            assert np.array_equal(hists[k], singles[k][0]), (exact, k)
        sv.close()


@pytest.mark.parametrize("shape", ["fs128_fs16_dec4", "t257"])
def test_other_shapes_take_the_generic_form_at_stride_1_only(ok, shape):
    st = _golden_stages(shape) if shape != "t257" else [(1, _rand_taps(257, 257))]
    flt = ok.Filter.from_stages(st)
    iq = _capture(np.random.default_rng(10), 20003)
    nus = [0.2, 0.0, -0.3]
    singles = _singles(ok, flt, nus, iq)
    sv = ok.Survey(flt, carriers=nus)
    assert sv.form == ok.SURVEY_TUNED_GENERIC and sv.stride == 1
    hists = sv.survey(iq)
    for k in range(3):
        assert sv.samples == singles[k][1] == 20003 // flt.total_decimation
        assert np.array_equal(hists[k], singles[k][0]), k
    sv.close()
    with pytest.raises(ok.OokdError, match="stride"):
        ok.Survey(flt, carriers=nus, stride=8)


# ----------------------------------------------------------------------------- 6. end to end ----

def test_chain_on_two_transmitters(ok, oracle):
    """Spectrum -> suggest_carriers -> Survey(carriers, stride 8) -> suggest_threshold per carrier ->
    Receiver(carriers): each transmitter's reference payloads"""
    iq, (b1, g1), (b2, g2) = two_transmitters(seed=2)
    n = iq.size // 2
    flt = ok.Filter.load(golden_path("filters", "fs32_fs4"))
    sp = ok.Spectrum()
    carriers, _ = ok.suggest_carriers(sp.spectrum(iq))
    sp.close()
    found = [c for c in carriers if not c.at_dc]
    assert sorted(c.bin for c in found) == [-307, 205]
    sv = ok.Survey(flt, carriers=[c.nu for c in found], stride=8)
    hists = sv.survey(iq)
    assert sv.form == ok.SURVEY_TUNED_MULTI
    thr = []
    for k, c in enumerate(found):
        _check(sv, hists[k], _power(iq, flt, c.nu), 8, k)
        s = ok.suggest_threshold(hists[k])
        assert s["found"] == 1
        thr.append(s["threshold"])
    sv.close()
    for c, t, (base, g) in ((c, t, {205: (b1, g1), -307: (b2, g2)}[c.bin]) for c, t in zip(found, thr)):
        od = oracle_device(oracle, g["device"])
        bits, _ = contract_rx(base, lib_stages(flt, 0.0), 0.1, SPB)
        _, ref_pay, ref_es = oracle.sm_stream(od, bits, SPB)
        assert len(ref_pay) >= 2 and len(ref_es) == 0
        dev = ok.Device.load(golden_path("devices", g["device"]), RATE)
        rx = ok.Receiver(flt, dev, max_samples=n, carriers=[(x.nu, y) for x, y in zip(found, thr)])
        got = rx.rx(iq)
        k = found.index(c)
        mine = [bytes(p) for p, cap in zip(got.payloads, got.captures) if cap == k]
        assert mine == [bytes(p) for p in ref_pay], (c.bin, len(mine))
        rx.close()


def test_c_scan_program_with_a_stride(ok, tmp_path):
    from tests.test_tuned_survey_host import build_scan
    scan = build_scan(tmp_path)
    iq, (_, g1), (_, g2) = two_transmitters(seed=3)
    cap = tmp_path / "two.sc16q11"
    iq.tofile(str(cap))
    filt = golden_path("filters", "fs32_fs4")
    devs = [golden_path("devices", g1["device"]), golden_path("devices", g2["device"])]
    plain = subprocess.run([scan, str(cap), str(RATE), filt] + devs + ["csv"], capture_output=True, text=True,
                           timeout=300)
    assert plain.returncode == 0, plain.stderr
    rows = lambda text: [ln.split(",", 1)[1:] for ln in text.split("\n")]       # without the wall clock
    assert plain.stderr.count(" messages\n") >= 2 and plain.stdout
    for args in (["--survey-stride", "8", str(cap), str(RATE), filt] + devs + ["csv"],
                 [str(cap), str(RATE), filt] + devs + ["--survey-stride", "8", "csv"]):
        r = subprocess.run([scan] + args, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        print(r.stderr)
        assert rows(r.stdout) == rows(plain.stdout)
        assert [ln for ln in r.stderr.split("\n") if "messages" in ln] == \
               [ln for ln in plain.stderr.split("\n") if "messages" in ln]
    bad = subprocess.run([scan, "--survey-stride", "3", str(cap), str(RATE), filt] + devs, capture_output=True,
                         text=True, timeout=300)
    assert bad.returncode != 0 and "stride" in bad.stderr and bad.stdout == ""


# ----------------------------------------------------------------------------- 7. beyond 2^32 ----

def test_capture_beyond_32_bit_indices(ok):
    """2^32 + 70001 CS8 samples built on the device from a period of 2^16 + 3 samples, two carriers, stride 8:
    `samples` and the sum of the bins per carrier, and two runs give the same counts.  (A workgroup's shared 32-bit
    counters: the launch sizes the grid so that none can wrap.)"""
    import torch
    torch.cuda.empty_cache()
    flt = ok.Filter.from_stages(_golden_stages("fs32_fs4"))
    P = (1 << 16) + 3
    n = (1 << 32) + 70001
    period = _as8(_capture(np.random.default_rng(6), P), "cs8")
    reps = n // P
    dev_p = torch.from_numpy(period.reshape(-1, 2)).cuda()
    cap = dev_p.repeat(reps + 1, 1)[:n].contiguous()
    assert cap.numel() == 2 * n
    torch.cuda.synchronize()
    sv = ok.Survey(flt, carriers=[0.2, -0.3], stride=8, sample_format="cs8")
    sv.survey_device(cap.data_ptr(), n)
    first = [sv.hist(0, k) for k in range(2)]
    print("kernel ms", sv.kernel_ms)
    samples = -(-n // 8)
    for k in range(2):
        assert sv.samples == samples == int(first[k].sum()), k
    assert not np.array_equal(first[0], first[1])
    sv.survey_device(cap.data_ptr(), n)
    for k in range(2):
        assert np.array_equal(sv.hist(0, k), first[k]), k
    sv.close()
    del cap
    torch.cuda.empty_cache()
