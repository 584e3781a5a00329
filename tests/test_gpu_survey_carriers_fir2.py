"""The carriers survey's fused two-stage form (OOKD_SURVEY_TUNED_MULTI_FIR2) on an MI355X: several carriers in one pass
through two decimate-by-2 stages, every S-th output counted.  Equality means all 256 counts and `samples`: the GPU's
histograms against the numpy restatement of the contract (tests/survey_carriers_contract.py) on the library's own taps,
for the tap counts around both stages' chunks, 1 .. 16 carriers, every stride, lengths around the zero history, the
first whole window, every residue mod 4 and the tile edges; more tiles than the grid has waves; the three sample
formats, batches with odd strides, unaligned captures; taps that drive the power through inf and NaN; at stride 1
against the generic form and the single tuned surveys; the shapes on which the flag has no effect; a capture beyond
2^32 samples; and the feature end to end, in Python and through examples/ookd_scan.c."""
import subprocess

import numpy as np
import pytest

from tests.helpers import golden_path
from tests.spectrum_contract import two_transmitters
from tests.survey_carriers_contract import contract_hist_strided
from tests.test_gpu_survey_carriers import (CARRIER_SETS, FORMATS, NUS16, _as8, _capture, _check, _golden_stages,
                                            _power, _rand_taps, _singles, _widen)
from tests.test_survey_host import np_hist
from tests.tuned_contract import RATE, SPB, contract_rx, lib_stages
from tests.tuned_survey_contract import oracle_device

pytestmark = pytest.mark.gpu

STRIDES = (1, 2, 4, 8, 16, 32, 64)
DEC4 = "fs128_fs16_dec4"


@pytest.fixture(scope="module")
def ok():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from ookiedokie_amd import build as okbuild
    okbuild.build()
    import ookiedokie_amd as okm
    okm.lib()
    return okm


def _two_stage(ok, t1, t2, seed=0):
    return ok.Filter.from_stages([(2, _rand_taps(t1, 7 * t1 + seed)), (2, _rand_taps(t2, 11 * t2 + seed + 1))])


def _dec4(ok):
    return ok.Filter.from_stages(_golden_stages(DEC4))


# ----------------------------------------------------------------------------- 1. the contract ----

@pytest.mark.parametrize("shape", [(1, 1), (2, 3), (15, 31), (16, 32), (16, 1), (1, 32), DEC4])
def test_equals_the_contract(ok, shape):
    flt = _dec4(ok) if shape == DEC4 else _two_stage(ok, *shape)
    rng = np.random.default_rng(17)
    lengths = sorted({0, 1, 3, 4, 5, 7, 8, 73, 74, 75, 76, 77, 78, 79, 1023, 1024, 1025, 1027, 4095, 4096, 4099,
                      3 * 4096 + 5, 70001} | {n for S in STRIDES for n in (4 * S - 1, 4 * S, 4 * S + 1)})
    caps = {n: _capture(rng, n) for n in lengths}
    power = {(nu, n): _power(caps[n], flt, nu) for nu in set(NUS16) for n in lengths}
    # the helper's slices of one power are contract_hist_strided's histograms
    h, s = contract_hist_strided(caps[70001], lib_stages(flt, 0.2), 8)
    assert s == -(-(70001 // 4) // 8) and np.array_equal(h, np_hist(power[0.2, 70001][::8]))
    for K, nus in CARRIER_SETS.items():
        for S in STRIDES:
            sv = ok.Survey(flt, carriers=nus, stride=S, tuned_fir2=True)
            assert sv.form == ok.SURVEY_TUNED_MULTI_FIR2 and sv.num_carriers == K and sv.stride == S
            assert sv.tune == nus[0]
            for n in lengths:
                hists = sv.survey(caps[n])
                assert hists.shape == (K, 256)
                for k, nu in enumerate(nus):
                    assert power[nu, n].size == n // 4
                    _check(sv, hists[k], power[nu, n], S, (shape, K, S, n, k))
                assert np.array_equal(sv.hist(), hists[0])      # ookd_survey_get_hist: carrier 0
            sv.close()


@pytest.mark.parametrize("thin", ["0", "1"])
def test_both_stage_0_shapes_at_the_large_strides(ok, monkeypatch, thin):
    """strides 32 and 64 with stage 0 thinned to the row entries a counted output reads (the default) and with every
    row entry computed (the developer variable the rate tool compares the two with): full and partial chunks, a
    ragged last tile, more tiles than one workgroup has waves, 16-bit and 8-bit"""
    monkeypatch.setenv("OOKD_DEVELOPER", "1")
    monkeypatch.setenv("OOKD_SURVEY_FIR2_THIN", thin)
    iq = _capture(np.random.default_rng(45), 70001)
    nus = [0.2, 0.0, -0.3]
    for flt in (_dec4(ok), _two_stage(ok, 15, 31)):
        for fmt in ("sc16q11", "cs8"):
            raw = iq if fmt == "sc16q11" else _as8(iq, fmt)
            wide = iq if fmt == "sc16q11" else _widen(raw, fmt)
            power = [_power(wide, flt, nu) for nu in nus]
            for S in (16, 32, 64):
                sv = ok.Survey(flt, carriers=nus, stride=S, sample_format=fmt, tuned_fir2=True)
                hists = sv.survey(raw)
                assert sv.form == ok.SURVEY_TUNED_MULTI_FIR2
                for k in range(3):
                    _check(sv, hists[k], power[k], S, (thin, fmt, S, k))
                sv.close()


# ----------------------------------------------------------------------------- 2. persistent walk ----

def test_more_tiles_than_the_grid_has_waves(ok):
    flt = _dec4(ok)
    n = (1 << 22) + 777                                         # 4097 tiles of 256 outputs
    iq = _capture(np.random.default_rng(3), n)
    nus = [0.2, -0.3, 0.0]
    sv = ok.Survey(flt, carriers=nus, stride=8, tuned_fir2=True)
    hists = sv.survey(iq)
    assert sv.form == ok.SURVEY_TUNED_MULTI_FIR2 and sv.kernel_ms > 0.0
    for k, nu in enumerate(nus):
        _check(sv, hists[k], _power(iq, flt, nu), 8, k)
    sv.close()


# ----------------------------------------------------------------------------- 3. formats and batches ----

@pytest.mark.parametrize("fmt", FORMATS)
def test_formats_batches_strides_and_alignment(ok, fmt):
    import torch
    flt = _dec4(ok)
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
        sv = ok.Survey(flt, carriers=nus, stride=S, max_captures=ncap, sample_format=fmt, tuned_fir2=True)
        sv.survey_device(first, n, num_captures=ncap, stride=cstride)
        # unaligned captures are read sample by sample by the same kernel: the form does not change
        assert sv.form == ok.SURVEY_TUNED_MULTI_FIR2
        hists = [[sv.hist(c, k) for k in range(3)] for c in range(ncap)]
        for c in range(ncap):
            for k in range(3):                                  # the layout: per capture, per carrier
                _check(sv, hists[c][k], power[c][k], S, (fmt, S, c, k))
        m = 1237                                                # a second, shorter run replaces them
        sv.survey_device(first, m, num_captures=2, stride=cstride)
        for c in range(2):
            for k in range(3):
                _check(sv, sv.hist(c, k), power[c][k][:m // 4], S, (fmt, S, c, k, m))
        with pytest.raises(ok.OokdError):
            sv.hist(2, 0)
        with pytest.raises(ok.OokdError):
            sv.hist(0, 3)
        assert sv.form == ok.SURVEY_TUNED_MULTI_FIR2
        sv.close()
    # one aligned capture, read in place with 16-byte loads
    one = torch.from_numpy(raws[0]).cuda()
    assert one.data_ptr() % 16 == 0
    sv = ok.Survey(flt, carriers=nus, stride=2, sample_format=fmt, tuned_fir2=True)
    sv.survey_device(one.data_ptr(), n)
    assert sv.form == ok.SURVEY_TUNED_MULTI_FIR2
    for k in range(3):
        _check(sv, sv.hist(0, k), power[0][k], 2, (fmt, "aligned", k))
    sv.close()


# ----------------------------------------------------------------------------- 4. extremes ----

def test_extremes(ok):
    """stage-0 taps of 1e15 and 1e-15 on full-scale samples, and taps that drive the stage-1 inputs and the power
    through inf and NaN: the order of the roundings is the contract's, so the counts are"""
    st = _golden_stages(DEC4)
    n = 20001
    rng = np.random.default_rng(4)
    full = rng.choice(np.array([-32768, 32767], np.int16), size=2 * n)
    noise = _capture(rng, n)
    noise[noise == 0] = 1
    nus = [0.2, 0.0, -0.5]
    # (the last two: stage 0 itself overflows, so stage 1 reads inf and NaN -- also behind 15 / 31 taps, where a
    # chunk's padding must not touch them)
    r15 = [(2, _rand_taps(15, 15)), (2, _rand_taps(31, 31))]
    for (s0, s1), iq, base in (((1e15, 1.0), full, st), ((1e-15, 1.0), full, st), ((2.0 ** 40, 1.0), noise, st),
                               ((2.0 ** 20, 2.0 ** 20), noise, st), ((1e15, 1e15), noise, st), ((1e30, 1.0), noise, st),
                               ((1e38, 1.0), noise, st), ((1e38, 1.0), noise, r15)):
        flt = ok.Filter.from_stages([(2, [t * s0 for t in base[0][1]]), (2, [t * s1 for t in base[1][1]])])
        power = [_power(iq, flt, nu) for nu in nus]
        if s0 * s1 >= 1e30:
            assert not np.isfinite(power[0]).all()
        if s0 == 1e38:
            assert np.isnan(power[0]).any() and np.isinf(power[0]).any()
        for S in (1, 8):
            sv = ok.Survey(flt, carriers=nus, stride=S, tuned_fir2=True)
            assert sv.form == ok.SURVEY_TUNED_MULTI_FIR2
            hists = sv.survey(iq)
            for k in range(3):
                _check(sv, hists[k], power[k], S, (s0, s1, S, k))
            sv.close()


# ----------------------------------------------------------------------------- 5. stride 1 against what exists ----

def test_stride_1_equals_the_generic_form_and_the_single_surveys(ok):
    flt = _dec4(ok)
    iq = _capture(np.random.default_rng(9), 20003)
    nus = [0.2, -0.3, 0.0, 0.5, 0.2]
    singles = _singles(ok, flt, nus, iq)
    for exact, form in ((False, ok.SURVEY_TUNED_MULTI_FIR2), (True, ok.SURVEY_TUNED_GENERIC)):
        sv = ok.Survey(flt, carriers=nus, exact=exact, tuned_fir2=True)
        assert sv.form == form and sv.stride == 1 and sv.num_carriers == 5
        hists = sv.survey(iq)
        assert sv.kernel_ms > 0.0
        for k in range(5):
            assert sv.samples == singles[k][1] == 20003 // 4 == int(hists[k].sum())
            assert np.array_equal(hists[k], singles[k][0]), (exact, k)
        sv.close()


def test_flag_without_effect(ok):
    iq = _capture(np.random.default_rng(10), 20003)
    nus = [0.2, 0.0, -0.3]
    fs32 = ok.Filter.from_stages(_golden_stages("fs32_fs4"))
    got = {}
    for flag in (False, True):
        sv = ok.Survey(fs32, carriers=nus, stride=8, tuned_fir2=flag)
        assert sv.form == ok.SURVEY_TUNED_MULTI
        got[flag] = (sv.survey(iq), sv.samples)
        sv.close()
    assert got[True][1] == got[False][1] and np.array_equal(got[True][0], got[False][0])
    flt = _two_stage(ok, 17, 32)
    sv = ok.Survey(flt, carriers=nus, tuned_fir2=True)
    assert sv.form == ok.SURVEY_TUNED_GENERIC and sv.stride == 1
    hists = sv.survey(iq)
    for k, nu in enumerate(nus):
        _check(sv, hists[k], _power(iq, flt, nu), 1, k)
    sv.close()
    with pytest.raises(ok.OokdError, match="stride"):
        ok.Survey(flt, carriers=nus, stride=2, tuned_fir2=True)
    with pytest.raises(ok.OokdError, match="stride"):
        ok.Survey(_dec4(ok), carriers=nus, stride=8, exact=True, tuned_fir2=True)


# ----------------------------------------------------------------------------- 6. end to end ----

def test_chain_on_two_transmitters(ok, oracle):
    """Spectrum -> suggest_carriers -> Survey(dec4, carriers, stride 8, tuned_fir2) -> suggest_threshold per carrier
    -> Receiver(dec4, carriers, tuned_fir2): each transmitter's reference payloads"""
    iq, (b1, g1), (b2, g2) = two_transmitters(seed=2)
    n = iq.size // 2
    flt = ok.Filter.load(golden_path("filters", DEC4))
    sp = ok.Spectrum()
    carriers, _ = ok.suggest_carriers(sp.spectrum(iq))
    sp.close()
    found = [c for c in carriers if not c.at_dc]
    assert sorted(c.bin for c in found) == [-307, 205]
    sv = ok.Survey(flt, carriers=[c.nu for c in found], stride=8, tuned_fir2=True)
    hists = sv.survey(iq)
    assert sv.form == ok.SURVEY_TUNED_MULTI_FIR2
    thr = []
    for k, c in enumerate(found):
        _check(sv, hists[k], _power(iq, flt, c.nu), 8, k)
        s = ok.suggest_threshold(hists[k])
        assert s["found"] == 1
        thr.append(s["threshold"])
    sv.close()
    for c, (base, g) in ((c, {205: (b1, g1), -307: (b2, g2)}[c.bin]) for c in found):
        od = oracle_device(oracle, g["device"], decimation=4)
        bits, _ = contract_rx(base, lib_stages(flt, 0.0), 0.1, SPB)
        _, ref_pay, ref_es = oracle.sm_stream(od, bits, SPB)
        assert len(ref_pay) >= 2 and len(ref_es) == 0
        dev = ok.Device.load(golden_path("devices", g["device"]), RATE // 4)
        rx = ok.Receiver(flt, dev, max_samples=n, carriers=[(x.nu, y) for x, y in zip(found, thr)], tuned_fir2=True)
        got = rx.rx(iq)
        k = found.index(c)
        mine = [bytes(p) for p, cap in zip(got.payloads, got.captures) if cap == k]
        assert mine == [bytes(p) for p in ref_pay], (c.bin, len(mine))
        rx.close()


def test_c_scan_program_with_a_stride_on_the_default_filter(ok, tmp_path):
    from tests.test_tuned_survey_host import build_scan
    scan = build_scan(tmp_path)
    iq, (_, g1), (_, g2) = two_transmitters(seed=3)
    cap = tmp_path / "two.sc16q11"
    iq.tofile(str(cap))
    filt = golden_path("filters", DEC4)
    devs = [golden_path("devices", g1["device"]), golden_path("devices", g2["device"])]
    plain = subprocess.run([scan, str(cap), str(RATE), filt] + devs + ["csv"], capture_output=True, text=True,
                           timeout=300)
    assert plain.returncode == 0, plain.stderr
    rows = lambda text: [ln.split(",", 1)[1:] for ln in text.split("\n")]       # without the wall clock
    assert plain.stderr.count(" messages\n") >= 2 and plain.stdout
    r = subprocess.run([scan, "--survey-stride", "8", str(cap), str(RATE), filt] + devs + ["csv"], capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    print(r.stderr)
    assert rows(r.stdout) == rows(plain.stdout)
    assert [ln for ln in r.stderr.split("\n") if "messages" in ln] == \
           [ln for ln in plain.stderr.split("\n") if "messages" in ln]


# ----------------------------------------------------------------------------- 7. beyond 2^32 ----

def test_capture_beyond_32_bit_indices(ok):
    """2^32 + 70001 CS8 samples built on the device from a period of 2^16 + 3 samples, two carriers, stride 8:
    `samples` and the sum of the bins per carrier, and two runs give the same counts."""
    import torch
    torch.cuda.empty_cache()
    flt = _dec4(ok)
    P = (1 << 16) + 3
    n = (1 << 32) + 70001
    period = _as8(_capture(np.random.default_rng(6), P), "cs8")
    reps = n // P
    dev_p = torch.from_numpy(period.reshape(-1, 2)).cuda()
    cap = dev_p.repeat(reps + 1, 1)[:n].contiguous()
    assert cap.numel() == 2 * n
    torch.cuda.synchronize()
    sv = ok.Survey(flt, carriers=[0.2, -0.3], stride=8, sample_format="cs8", tuned_fir2=True)
    sv.survey_device(cap.data_ptr(), n)
    assert sv.form == ok.SURVEY_TUNED_MULTI_FIR2
    first = [sv.hist(0, k) for k in range(2)]
    print("kernel ms", sv.kernel_ms)
    samples = -(-(n // 4) // 8)
    for k in range(2):
        assert sv.samples == samples == int(first[k].sum()), k
    assert not np.array_equal(first[0], first[1])
    sv.survey_device(cap.data_ptr(), n)
    for k in range(2):
        assert np.array_equal(sv.hist(0, k), first[k]), k
    sv.close()
    del cap
    torch.cuda.empty_cache()
