"""Host side of the carriers survey's fused two-stage form (OOKD_SURVEY_TUNED_MULTI_FIR2, asked for with
OOKD_RX_TUNED_FIR2): the new constant, which create calls now pass their argument checks and which are still refused
(all before any HIP call), Survey's tuned_fir2 argument, and the reason for the feature on the numpy contract and the
oracle alone: through the backend default fs128_fs16_dec4 a histogram of every 8th or 64th output still yields a
threshold that decodes each transmitter's payloads.  Also that examples/ookd_scan.c still compiles and prints its
usage."""
import os
import subprocess

import numpy as np
import pytest

import ookiedokie_amd as ok
from ookiedokie_amd import build as okbuild
from tests.helpers import ROOT, golden_path
from tests.spectrum_contract import two_transmitters
from tests.test_survey_host import np_hist
from tests.test_tuned_survey_host import build_scan
from tests.tuned_contract import RATE, lib_stages
from tests.tuned_survey_contract import contract_power, decode, oracle_device

WHO = "ookd_survey_create_carriers"


@pytest.fixture(scope="module")
def built_lib():
    okbuild.build()
    return ok.lib()


@pytest.fixture(scope="module")
def dec4(built_lib):
    return ok.Filter.load(golden_path("filters", "fs128_fs16_dec4"))


def _tunes(nus):
    t = (ok.Tune * len(nus))()
    for x, nu in zip(t, nus):
        x.nu = nu
    return t


def _flat(ntaps):
    return [1.0 / ntaps] * ntaps


# ---- interface --------------------------------------------------------------------------------------------

def test_new_form_constant(built_lib, tmp_path):
    src = tmp_path / "forms.c"
    src.write_text('#include <stdio.h>\n#include "ookiedokie_amd.h"\n'
                   'int main(void) { printf("OOKD_SURVEY_TUNED_MULTI_FIR2 == %d\\n%d %d", OOKD_SURVEY_TUNED_MULTI_FIR2,\n'
                   '  OOKD_SURVEY_TUNED_MULTI, OOKD_RX_TUNED_FIR2); return 0; }\n')
    exe = tmp_path / "forms"
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o",
                        str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = subprocess.run([str(exe)], capture_output=True, text=True).stdout.split("\n")
    assert out[0] == "OOKD_SURVEY_TUNED_MULTI_FIR2 == 5"
    assert [int(x) for x in out[1].split()] == [4, ok.RX_TUNED_FIR2]
    assert ok.SURVEY_TUNED_MULTI_FIR2 == 5


def test_create_with_the_flag_needs_no_gpu_to_check_its_arguments(built_lib, dec4):
    L = built_lib
    F2 = ok.RX_TUNED_FIR2
    fs32 = ok.Filter.load(golden_path("filters", "fs32_fs4"))
    two = _tunes([0.2, -0.3])
    mk = ok.Filter.from_stages

    def reaches_the_device(filt, flags, stride):
        h = L.ookd_survey_create_carriers(-1, filt._h, flags, 1, None, two, 2, stride)
        assert not h and "no CPU fallback" in ok.last_error(), (flags, stride, ok.last_error())

    def refused(filt, flags, stride, word):
        h = L.ookd_survey_create_carriers(-1, filt._h, flags, 1, None, two, 2, stride)
        assert not h
        err = ok.last_error()
        assert WHO in err and word in err, (word, err)
        assert "no CPU fallback" not in err, err            # refused on its arguments, before any HIP call

    for stride in (1, 8, 64):
        reaches_the_device(dec4, F2, stride)
    reaches_the_device(dec4, F2 | ok.RX_SAMPLES_CS8, 8)
    reaches_the_device(dec4, F2 | ok.RX_SAMPLES_CU8, 64)
    reaches_the_device(fs32, F2, 8)                         # no effect: the one-stage multi form
    reaches_the_device(mk([(2, _flat(15)), (2, _flat(31))]), F2, 2)
    reaches_the_device(mk([(2, _flat(1)), (2, _flat(1))]), F2, 2)
    # shapes beside the fused one: the flag has no effect and the stride is refused as before
    refused(mk([(2, _flat(17)), (2, _flat(32))]), F2, 2, "stride")
    refused(mk([(2, _flat(16)), (2, _flat(33))]), F2, 2, "stride")
    refused(mk([(1, _flat(257))]), F2, 2, "stride")
    refused(mk([(2, _flat(16)), (4, _flat(32))]), F2, 2, "stride")
    refused(mk([(2, _flat(16)), (2, _flat(32)), (2, _flat(8))]), F2, 2, "stride")
    refused(mk([(2, _flat(15))]), F2, 2, "stride")
    refused(dec4, F2 | ok.RX_EXACT_FIR, 8, "stride")
    refused(dec4, 0, 8, "stride")                           # without the flag nothing changes
    refused(dec4, F2 | ok.RX_KEEP_FIR, 1, "flags")
    refused(dec4, F2 | ok.RX_SAMPLES_CS8 | ok.RX_SAMPLES_CU8, 1, "flags")
    # at stride 1 those shapes, flagged, still reach the device (the generic form)
    reaches_the_device(mk([(2, _flat(17)), (2, _flat(32))]), F2, 1)
    reaches_the_device(dec4, F2 | ok.RX_EXACT_FIR, 1)


def test_tuned_fir2_needs_carriers():
    f = object()
    with pytest.raises(ValueError):
        ok.Survey(f, tune=0.1, tuned_fir2=True)
    with pytest.raises(ValueError):
        ok.Survey(f, tuned_fir2=True)


# ---- the reason for the feature, on the numpy contract and the oracle alone ---------------------------------

@pytest.mark.parametrize("seed", [2, 3])
def test_strided_survey_through_the_default_filter_finds_each_threshold(built_lib, oracle, dec4, seed):
    iq, (b1, g1), (b2, g2) = two_transmitters(seed)
    for hz, base, g, npay in ((600e3, b1, g1, 3), (-900e3, b2, g2, 2)):
        nu = hz / RATE
        od = oracle_device(oracle, g["device"], decimation=4)
        _, ref_pay, ref_es = decode(oracle, od, base, lib_stages(dec4, 0.0), 0.1)
        assert len(ref_pay) == npay and len(ref_es) == 0
        # untuned, the carrier lies outside the filter: nothing is decoded
        _, pay0, _ = decode(oracle, od, iq, lib_stages(dec4, 0.0), 0.1)
        assert len(pay0) == 0
        stages = lib_stages(dec4, nu)
        with np.errstate(over="ignore", invalid="ignore"):
            p = contract_power(iq, stages)                  # once: every stride is a slice of it
        assert p.size == (iq.size // 2) // 4
        for S in (1, 8, 64):
            h = np_hist(p[::S])
            assert int(h.sum()) == -(-p.size // S)
            s = ok.suggest_threshold(h)
            print(seed, hz, S, s["threshold"], s["off_bin"], s["on_bin"])
            assert s["found"] == 1
            _, pay, es = decode(oracle, od, iq, stages, s["threshold"])
            assert [bytes(x) for x in pay] == [bytes(x) for x in ref_pay] and len(es) == 0, (seed, hz, S)


# ---- the C program ------------------------------------------------------------------------------------------

def test_scan_example_still_compiles_and_prints_usage(built_lib, tmp_path):
    exe = build_scan(tmp_path)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode != 0 and "usage" in r.stderr and "--survey-stride" in r.stderr and r.stdout == ""
