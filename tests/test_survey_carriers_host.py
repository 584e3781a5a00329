"""Host side of the carriers survey (ookd_survey_create_carriers): the new symbols and constants, every refusal
(all before any HIP call), Survey's carriers / stride arguments, and the reason for the stride on the numpy contract
alone: a histogram of every 8th or 64th output of the tuned filter shows the same two levels as the full one, and
its threshold decodes the reference payloads.  Also that examples/ookd_scan.c still compiles and prints its usage."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import ookiedokie_amd as ok
from ookiedokie_amd import build as okbuild
from tests.helpers import ROOT, golden_path
from tests.survey_carriers_contract import contract_hist_strided
from tests.test_survey_host import assert_same_suggestion, np_hist, py_suggest
from tests.test_tuned_survey_host import build_scan
from tests.tuned_contract import RATE, golden_capture, lib_stages, moved
from tests.tuned_survey_contract import DC, NOISE, contract_hist, contract_power, decode, oracle_device

WHO = "ookd_survey_create_carriers"


@pytest.fixture(scope="module")
def built_lib():
    okbuild.build()
    return ok.lib()


@pytest.fixture(scope="module")
def fs32(built_lib):
    return ok.Filter.load(golden_path("filters", "fs32_fs4"))


def _tunes(nus, reserved=0):
    t = (ok.Tune * len(nus))()
    for x, nu in zip(t, nus):
        x.nu = nu
    if reserved:
        t[len(nus) - 1].reserved[2] = reserved
    return t


# ---- interface --------------------------------------------------------------------------------------------

def test_new_symbols_and_constants(built_lib, tmp_path):
    for name in ("ookd_survey_create_carriers", "ookd_survey_num_carriers", "ookd_survey_stride",
                 "ookd_survey_get_carrier_hist"):
        assert hasattr(built_lib, name), name
    assert built_lib.ookd_survey_num_carriers(None) == 0
    assert built_lib.ookd_survey_stride(None) == 0
    lh = ok.LevelHist()
    assert built_lib.ookd_survey_get_carrier_hist(None, 0, 0, C.byref(lh)) != 0
    assert "ookd_survey_get_carrier_hist" in ok.last_error()
    src = tmp_path / "forms.c"
    src.write_text('#include <stdio.h>\n#include "ookiedokie_amd.h"\n'
                   'int main(void) { printf("OOKD_SURVEY_TUNED_MULTI == %d\\n%d %d %d %d %d", OOKD_SURVEY_TUNED_MULTI,\n'
                   '  OOKD_SURVEY_MAX_CARRIERS, OOKD_SURVEY_MAX_STRIDE, OOKD_SURVEY_GENERIC, OOKD_SURVEY_TUNED_GENERIC,\n'
                   '  OOKD_SURVEY_TUNED_FIR1); return 0; }\n')
    exe = tmp_path / "forms"
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o",
                        str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = subprocess.run([str(exe)], capture_output=True, text=True).stdout.split("\n")
    assert out[0] == "OOKD_SURVEY_TUNED_MULTI == 4"
    assert [int(x) for x in out[1].split()] == [16, 64, 1, 2, 3]
    assert (ok.SURVEY_TUNED_MULTI, ok.SURVEY_MAX_CARRIERS, ok.SURVEY_MAX_STRIDE) == (4, 16, 64)


def test_create_carriers_refusals_need_no_gpu(built_lib, fs32):
    L = built_lib
    both = ok.RX_SAMPLES_CS8 | ok.RX_SAMPLES_CU8
    dec4 = ok.Filter.load(golden_path("filters", "fs128_fs16_dec4"))
    t257 = ok.Filter.from_stages([(1, [1.0 / 257] * 257)])

    def refused(filt, flags, max_captures, tunes, k, stride, *words):
        h = L.ookd_survey_create_carriers(-1, filt, flags, max_captures, None, tunes, k, stride)
        assert not h
        err = ok.last_error()
        for w in (WHO,) + words:
            assert w in err, (w, err)
        assert "no CPU fallback" not in err, err         # refused on its arguments, before any HIP call

    two = _tunes([0.2, -0.3])
    refused(fs32._h, 0, 1, two, 0, 1, "num_carriers")
    refused(fs32._h, 0, 1, _tunes([0.01 * k for k in range(17)]), 17, 1, "num_carriers")
    refused(fs32._h, 0, 1, None, 2, 1, "tunes")
    refused(fs32._h, 0, 1, _tunes([0.2, float("nan")]), 2, 1, "nu")
    refused(fs32._h, 0, 1, _tunes([0.6, 0.1]), 2, 1, "[-0.5, 0.5]")
    refused(fs32._h, 0, 1, _tunes([0.1, -0.500001]), 2, 1, "[-0.5, 0.5]")
    refused(fs32._h, 0, 1, _tunes([0.2, -0.3], reserved=7), 2, 1, "reserved")
    refused(None, 0, 1, two, 2, 1, "needs a filter")
    for stride in (0, 3, 6, 65, 128, 1 << 31):
        refused(fs32._h, 0, 1, two, 2, stride, "stride")
    refused(fs32._h, ok.RX_KEEP_FIR, 1, two, 2, 1, "flags")                 # a stray bit
    refused(fs32._h, both, 1, two, 2, 1, "flags")
    refused(fs32._h, 0, 0, two, 2, 1, "max_captures")
    # a stride on a shape (or with the flag) that has no OOKD_SURVEY_TUNED_MULTI form
    refused(dec4._h, 0, 1, two, 2, 8, "stride")
    refused(t257._h, 0, 1, two, 2, 2, "stride")
    refused(fs32._h, ok.RX_EXACT_FIR, 1, two, 2, 8, "stride")
    # valid arguments reach the device check: no GPU (or no device -1) is said loudly
    for filt, flags, tunes, k, stride in ((fs32, 0, two, 2, 1), (fs32, ok.RX_SAMPLES_CS8, two, 2, 64),
                                          (fs32, ok.RX_EXACT_FIR | ok.RX_SAMPLES_CU8, two, 1, 1),
                                          (dec4, 0, two, 2, 1), (t257, 0, _tunes([0.0, 0.5, -0.5, 0.0]), 4, 1),
                                          (fs32, 0, _tunes([0.01 * k for k in range(16)]), 16, 8)):
        h = L.ookd_survey_create_carriers(-1, filt._h, flags, 1, None, tunes, k, stride)
        assert not h and "no CPU fallback" in ok.last_error(), ok.last_error()


def test_survey_carriers_arguments():
    """carriers beside tune / tune_hz, or a stride without carriers, is an error before anything is created"""
    f = object()
    with pytest.raises(ValueError):
        ok.Survey(f, carriers=[0.1], tune=0.1)
    with pytest.raises(ValueError):
        ok.Survey(f, carriers=[0.1], tune_hz=1e5, sample_rate=3e6)
    with pytest.raises(ValueError):
        ok.Survey(f, stride=8)
    with pytest.raises(ValueError):
        ok.Survey(f, stride=1, tune=0.1)
    with pytest.raises(ValueError):
        ok.Survey(f, carriers=[0.1], stride=8, sample_format="cf32")
    assert isinstance(ok.Survey.num_carriers, property) and isinstance(ok.Survey.stride, property)


def test_contract_at_stride_1_is_the_tuned_surveys(fs32):
    iq = np.random.default_rng(2).integers(-2048, 2048, size=2 * 1237).astype(np.int16)
    stages = lib_stages(fs32, 0.2)
    h1, n1 = contract_hist_strided(iq, stages, 1)
    h, n = contract_hist(iq, stages)
    assert n1 == n == 1237 and np.array_equal(h1, h)
    for S in (2, 8, 64):
        hs, ns = contract_hist_strided(iq, stages, S)
        assert ns == -(-1237 // S) == int(hs.sum())


# ---- the reason for the stride, on the numpy contract alone -------------------------------------------------

@pytest.fixture(scope="module")
def unmoved(built_lib, oracle, fs32):
    """the golden captures decoded where they are, at the reference's default threshold"""
    out = {}
    for name in ("G1", "G2"):
        base, g = golden_capture(name)
        od = oracle_device(oracle, g["device"])
        ms, pay, es = decode(oracle, od, base, lib_stages(fs32, 0.0), 0.1)
        assert len(ms) == (3 if name == "G1" else 2) and len(es) == 0
        out[name] = (base, od, pay)
    return out


@pytest.mark.parametrize("seed", [0, 3])
@pytest.mark.parametrize("scale", [1.0, 1 / 4, 1 / 8])
@pytest.mark.parametrize("hz", [600e3, -900e3])
@pytest.mark.parametrize("name", ["G1", "G2"])
def test_thinned_histogram_shows_the_same_levels(built_lib, oracle, fs32, unmoved, name, hz, scale, seed):
    base, od, ref_pay = unmoved[name]
    nu = hz / RATE
    iq = moved(base, nu, DC, NOISE, seed, scale)
    stages = lib_stages(fs32, nu)
    with np.errstate(over="ignore", invalid="ignore"):
        p = contract_power(iq, stages)                      # once: every stride is a slice of it
    s1 = ok.suggest_threshold(np_hist(p))
    assert s1["found"] == 1
    for S in (8, 64):
        h = np_hist(p[::S])
        assert int(h.sum()) == -(-p.size // S)
        s = ok.suggest_threshold(h)
        assert_same_suggestion(s, py_suggest(h))
        print(name, hz, scale, seed, S, s["threshold"], s1["threshold"], s["off_bin"], s1["off_bin"])
        assert s["found"] == 1
        assert s["on_bin"] == s1["on_bin"]
        assert abs(int(s["off_bin"]) - int(s1["off_bin"])) <= 1
        _, pay, _ = decode(oracle, od, iq, stages, s["threshold"])
        assert [bytes(x) for x in pay] == [bytes(x) for x in ref_pay]


# ---- the C program ------------------------------------------------------------------------------------------

def test_scan_example_still_compiles_and_prints_usage(built_lib, tmp_path):
    exe = build_scan(tmp_path)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode != 0 and "usage" in r.stderr and "--survey-stride" in r.stderr and r.stdout == ""
    r = subprocess.run([exe, "--survey-stride", "8", "capture.sc16q11", str(RATE), golden_path("filters", "fs32_fs4")],
                       capture_output=True, text=True)          # no device
    assert r.returncode != 0 and "usage" in r.stderr
