"""Host side of the tuned envelope survey: the new symbols and their refusals (all before any HIP call), Survey's
tune arguments, the numpy restatement the GPU tests compare against (at nu = 0 it must be the CPU oracle's
histogram), and the reason for the feature on the oracle alone: on a capture whose carrier sits beside the centre
the untuned histogram shows no two levels, the tuned one does, and its threshold decodes what 0.1 cannot.  Also
that examples/ookd_scan.c compiles against the header and the library only."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import ookiedokie_amd as ok
from ookiedokie_amd import build as okbuild
from tests.helpers import ROOT, golden_path
from tests.spectrum_contract import two_transmitters
from tests.test_survey_host import assert_same_suggestion, np_hist, oracle_power, py_suggest
from tests.tuned_contract import RATE, golden_capture, lib_stages, moved
from tests.tuned_survey_contract import DC, NOISE, contract_hist, decode, oracle_device


@pytest.fixture(scope="module")
def built_lib():
    okbuild.build()
    return ok.lib()


@pytest.fixture(scope="module")
def fs32(built_lib):
    return ok.Filter.load(golden_path("filters", "fs32_fs4"))


def _tune(nu, reserved=0):
    t = ok.Tune()
    t.nu = nu
    t.reserved[1] = reserved
    return t


# ---- interface --------------------------------------------------------------------------------------------

def test_new_symbols_and_form_values(built_lib, tmp_path):
    for name in ("ookd_survey_create_tuned", "ookd_survey_tune", "ookd_survey_form"):
        assert hasattr(built_lib, name), name
    assert built_lib.ookd_survey_tune(None) == 0.0
    assert built_lib.ookd_survey_form(None) == 0
    src = tmp_path / "forms.c"
    src.write_text('#include <stdio.h>\n#include "ookiedokie_amd.h"\n'
                   'int main(void) { printf("%d %d %d %d", OOKD_SURVEY_GENERIC, OOKD_SURVEY_TUNED_GENERIC,\n'
                   '  OOKD_SURVEY_TUNED_FIR1, OOKD_API_VERSION); return 0; }\n')
    exe = tmp_path / "forms"
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o",
                        str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True).stdout.split()]
    assert got == [1, 2, 3, 1]
    assert (ok.SURVEY_GENERIC, ok.SURVEY_TUNED_GENERIC, ok.SURVEY_TUNED_FIR1) == (1, 2, 3)


def test_create_tuned_refusals_need_no_gpu(built_lib, fs32):
    L = built_lib
    both = ok.RX_SAMPLES_CS8 | ok.RX_SAMPLES_CU8

    def refused(filt, flags, max_captures, tune, *words):
        h = L.ookd_survey_create_tuned(-1, filt, flags, max_captures, None, C.byref(tune) if tune is not None else None)
        assert not h
        err = ok.last_error()
        for w in words:
            assert w in err, (w, err)
        assert "no CPU fallback" not in err, err         # refused on its arguments, before any HIP call

    refused(fs32._h, 0, 1, _tune(float("nan")), "ookd_survey_create_tuned", "nu")
    refused(fs32._h, 0, 1, _tune(0.6), "ookd_survey_create_tuned", "[-0.5, 0.5]")
    refused(fs32._h, 0, 1, _tune(-0.500001), "[-0.5, 0.5]")
    refused(None, 0, 1, _tune(0.2), "ookd_survey_create_tuned", "needs a filter")
    refused(fs32._h, both, 1, _tune(0.2), "ookd_survey_create_tuned", "flags")
    refused(fs32._h, ok.RX_KEEP_FIR, 1, _tune(0.2), "flags")              # a stray bit
    refused(fs32._h, ok.RX_KEEP_FIR, 1, None, "flags")                    # ... also on an untuned one
    refused(fs32._h, 0, 0, _tune(0.2), "max_captures")
    refused(fs32._h, ok.RX_EXACT_FIR, 0, None, "max_captures")
    refused(fs32._h, 0, 1, _tune(0.2, reserved=7), "reserved")
    # valid arguments reach the device check: no GPU (or no device -1) is said loudly
    for tune, flags in ((_tune(0.2), ok.RX_EXACT_FIR | ok.RX_SAMPLES_CS8), (_tune(0.0), ok.RX_EXACT_FIR), (None, 0)):
        h = L.ookd_survey_create_tuned(-1, fs32._h, flags, 1, None, C.byref(tune) if tune is not None else None)
        assert not h and "no CPU fallback" in ok.last_error()
    h = L.ookd_survey_create_tuned(-1, None, 0, 1, None, None)              # no filter, untuned: ookd_survey_create
    assert not h and "no CPU fallback" in ok.last_error()


def test_survey_tune_arguments():
    """both ways of saying the offset at once, or half of the second one, is an error before anything is created"""
    f = object()
    with pytest.raises(ValueError):
        ok.Survey(f, tune=0.1, tune_hz=1e5, sample_rate=3e6)
    with pytest.raises(ValueError):
        ok.Survey(f, tune_hz=1e5)
    with pytest.raises(ValueError):
        ok.Survey(f, sample_rate=3e6)
    with pytest.raises(ValueError):
        ok.Survey(f, tune_hz=1e5, sample_rate=0)
    with pytest.raises(ValueError):
        ok.Survey(f, tune=0.1, sample_format="cf32")
    assert isinstance(ok.Survey.tune, property) and isinstance(ok.Survey.form, property)


# ---- the restatement ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["G1", "G2"])
def test_contract_histogram_at_nu_0_is_the_oracles(built_lib, oracle, name):
    iq, _ = golden_capture(name)
    iq = (iq + np.random.default_rng(7).integers(-40, 41, size=iq.size)).astype(np.int16)
    iq = iq[:2 * (iq.size // 2 - 3)]                            # no multiple of the decimation
    for fname in ("fs32_fs4", "fs128_fs16_dec4"):
        f = ok.Filter.load(golden_path("filters", fname))
        of = oracle.load_filter_json(golden_path("filters", fname))
        h, samples = contract_hist(iq, lib_stages(f, 0.0))
        want = np_hist(oracle_power(oracle, of, iq))
        assert samples == (iq.size // 2) // f.total_decimation == int(want.sum())
        assert np.array_equal(h, want), fname
        assert np.count_nonzero(want) > 20


# ---- the reason for the feature, on the oracle alone --------------------------------------------------------

@pytest.fixture(scope="module")
def unmoved(built_lib, oracle, fs32):
    """the golden captures decoded where they are, at the reference's default threshold"""
    out = {}
    for name in ("G1", "G2"):
        base, g = golden_capture(name)
        od = oracle_device(oracle, g["device"])
        ms, pay, es = decode(oracle, od, base, lib_stages(fs32, 0.0), 0.1)
        assert len(ms) == (3 if name == "G1" else 2) and len(es) == 0
        out[name] = (base, od, ms, pay)
    return out


@pytest.mark.parametrize("seed", [0, 3])
@pytest.mark.parametrize("scale", [1.0, 1 / 4, 1 / 8])
@pytest.mark.parametrize("hz", [600e3, -900e3])
@pytest.mark.parametrize("name", ["G1", "G2"])
def test_tuned_histogram_finds_the_threshold_the_untuned_one_cannot(built_lib, oracle, fs32, unmoved, name, hz, scale,
                                                                    seed):
    base, od, ref_ms, ref_pay = unmoved[name]
    nu = hz / RATE
    iq = moved(base, nu, DC, NOISE, seed, scale)
    untuned, _ = contract_hist(iq, lib_stages(fs32, 0.0))
    s0 = ok.suggest_threshold(untuned)
    assert s0["found"] == 0, s0                                 # the DC term, not the carrier
    stages = lib_stages(fs32, nu)
    tuned, samples = contract_hist(iq, stages)
    assert samples == iq.size // 2 == int(tuned.sum())
    s = ok.suggest_threshold(tuned)
    assert_same_suggestion(s, py_suggest(tuned))
    print(name, hz, scale, seed, s)
    assert s["found"] == 1 and s["on_bin"] - s["off_bin"] >= 30
    ms, pay, es = decode(oracle, od, iq, stages, s["threshold"])
    assert [bytes(p) for p in pay] == [bytes(p) for p in ref_pay]
    assert len(es) <= 1
    assert np.abs(ms.astype(np.int64) - ref_ms.astype(np.int64)).max() <= 2     # they move with the threshold
    if scale == 1 / 8:
        ms1, pay1, _ = decode(oracle, od, iq, stages, 0.1)
        assert [bytes(p) for p in pay1] != [bytes(p) for p in ref_pay]


@pytest.mark.parametrize("seed", [0, 1])
def test_two_transmitters_each_carrier_has_its_threshold(built_lib, oracle, fs32, seed):
    iq, (b1, g1), (b2, g2) = two_transmitters(seed)
    for base, g, hz in ((b1, g1, 600e3), (b2, g2, -900e3)):
        od = oracle_device(oracle, g["device"])
        _, ref_pay, ref_es = decode(oracle, od, base, lib_stages(fs32, 0.0), 0.1)
        assert len(ref_pay) >= 2 and len(ref_es) == 0
        stages = lib_stages(fs32, hz / RATE)
        h, _ = contract_hist(iq, stages)
        s = ok.suggest_threshold(h)
        print(hz, seed, s)
        assert s["found"] == 1
        _, pay, es = decode(oracle, od, iq, stages, s["threshold"])
        assert [bytes(p) for p in pay] == [bytes(p) for p in ref_pay]
        assert len(es) == 0


# ---- the C program ------------------------------------------------------------------------------------------

def build_scan(tmp_path):
    exe = tmp_path / "ookd_scan"
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "examples", "ookd_scan.c"), "-o", str(exe),
                        "-L" + os.path.dirname(ok.LIB_PATH), "-lookiedokie_amd",
                        "-Wl,-rpath," + os.path.dirname(ok.LIB_PATH)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return str(exe)


def test_scan_example_compiles_and_prints_usage(built_lib, tmp_path):
    exe = build_scan(tmp_path)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode != 0 and "usage" in r.stderr and r.stdout == ""
    r = subprocess.run([exe, "capture.sc16q11", str(RATE), golden_path("filters", "fs32_fs4")], capture_output=True,
                       text=True)                               # no device
    assert r.returncode != 0 and "usage" in r.stderr
