"""Host side of the frequency-tuned front end: the tap rule (ookd_filter_tuned_taps), the numpy restatement of the
contract the GPU tests compare against (at nu = 0 it must be the CPU oracle, bits and floats), the C example."""
import json
import os
import subprocess

import numpy as np
import pytest

import ookiedokie_amd as ok
from ookiedokie_amd import build as okbuild
from tests.helpers import ROOT, golden_path
from tests.tuned_contract import RATE, SPB, THR, contract_rx, golden_capture, taps_rule


@pytest.fixture(scope="module")
def built_lib():
    okbuild.build()
    return ok.lib()


def _filter(tmp_path, name):
    if name != "taps257":
        return ok.Filter.load(golden_path("filters", name))
    h = np.random.default_rng(257).normal(0, 1, 257)
    p = tmp_path / "taps257.json"
    p.write_text(json.dumps({"filter": {"stages": [{"decimation": 1, "taps": [float(t) for t in h / np.abs(h).sum()]}]}}))
    return ok.Filter.load(str(p))


def _ulps(got, want64):
    """distance of float32 `got` from the double `want64` in float32 ulps of want64's binade"""
    w = np.abs(want64)
    ulp = np.spacing(np.maximum(w, np.finfo(np.float32).tiny).astype(np.float32)).astype(np.float64)
    return np.abs(got.astype(np.float64) - want64) / ulp


NUS = [0.2, -0.3, 1.0 / 3000.0, 0.5, -0.5, 0.25, 600e3 / 3e6, -900e3 / 3e6]


@pytest.mark.parametrize("name", ["fs32_fs4", "fs128_fs16_dec4", "taps257"])
def test_tuned_taps_follow_the_rule(built_lib, tmp_path, name):
    f = _filter(tmp_path, name)
    before = 1
    for s in range(f.num_stages):
        D, h = f.stage(s)
        for nu in NUS:
            re, im = f.tuned_taps(nu, s)
            assert re.dtype == np.float32 and re.size == h.size == im.size
            wr, wi = taps_rule(h, nu, before)           # stage 1 of the decimating filter: 2 nu
            assert _ulps(re, wr).max() <= 1.0, (name, s, nu)
            assert _ulps(im, wi).max() <= 1.0, (name, s, nu)
            # -nu: the same re, the bitwise negated im
            re_n, im_n = f.tuned_taps(-nu, s)
            assert (re_n.view(np.uint32) == re.view(np.uint32)).all(), (name, s, nu)
            assert (im_n.view(np.uint32) == (im.view(np.uint32) ^ np.uint32(0x80000000))).all(), (name, s, nu)
        # nu = 0: re == h bitwise, im == +0
        re, im = f.tuned_taps(0.0, s)
        assert (re.view(np.uint32) == h.view(np.uint32)).all()
        assert (im.view(np.uint32) == 0).all()
        before *= D
    if name == "fs128_fs16_dec4":
        assert f.num_stages == 2 and f.stage(0)[0] == 2
        # the second stage turns twice as fast as the first
        _, im1 = f.tuned_taps(0.05, 1)
        want = f.stage(1)[1].astype(np.float64) * np.sin(2 * np.pi * 0.1 * np.arange(im1.size))
        assert np.abs(im1 - want).max() < 1e-6


def test_tuned_taps_refusals(built_lib):
    f = ok.Filter.load(golden_path("filters", "fs32_fs4"))
    n = f.stage(0)[1].size
    re, im = np.zeros(n, np.float32), np.zeros(n, np.float32)
    L = ok.lib()
    assert L.ookd_filter_tuned_taps(f._h, 0.2, 0, re.ctypes.data, im.ctypes.data) == 0
    for nu in (float("nan"), 0.500001, -0.6, float("inf")):
        assert L.ookd_filter_tuned_taps(f._h, nu, 0, re.ctypes.data, im.ctypes.data) == -1, nu
    assert L.ookd_filter_tuned_taps(f._h, 0.2, 1, re.ctypes.data, im.ctypes.data) == -1         # no such stage
    assert L.ookd_filter_tuned_taps(None, 0.2, 0, re.ctypes.data, im.ctypes.data) == -1
    assert L.ookd_filter_tuned_taps(f._h, 0.2, 0, None, im.ctypes.data) == -1
    assert L.ookd_filter_tuned_taps(f._h, 0.2, 0, re.ctypes.data, None) == -1
    with pytest.raises(ok.OokdError):
        f.tuned_taps(0.2, 3)


def test_receiver_tune_arguments():
    """both ways of saying the offset at once, or half of the second one, is an error before anything is created"""
    f = object()
    with pytest.raises(ValueError):
        ok.Receiver(f, None, max_samples=1, tune=0.1, tune_hz=1e5, sample_rate=3e6)
    with pytest.raises(ValueError):
        ok.Receiver(f, None, max_samples=1, tune_hz=1e5)
    with pytest.raises(ValueError):
        ok.Receiver(f, None, max_samples=1, sample_rate=3e6)
    assert (ok.FRONT_TUNED_GENERIC, ok.FRONT_TUNED_FIR1) == (12, 13)


@pytest.mark.parametrize("name", ["G1", "G2"])
def test_contract_at_nu_0_is_the_oracle(built_lib, oracle, name):
    """the yardstick of the GPU tests: the restatement, fed the library's taps for nu = 0, gives the oracle's bits
    and floats bit for bit"""
    iq, g = golden_capture(name)
    rng = np.random.default_rng(7)
    iq = (iq + rng.integers(-40, 41, size=iq.size)).astype(np.int16)
    for fname in ("fs32_fs4", "fs128_fs16_dec4"):
        f = ok.Filter.load(golden_path("filters", fname))
        of = oracle.load_filter_json(golden_path("filters", fname))
        stages = [(f.stage(s)[0],) + tuple(f.tuned_taps(0.0, s)) for s in range(f.num_stages)]
        bits, y = contract_rx(iq, stages, THR, SPB)
        want = oracle.rx(iq, of, THR, None, SPB, want_bits=True, want_fir=True)
        assert bits.size == want.bits.size
        assert (bits == want.bits).all(), fname
        assert (y.view(np.uint32) == want.fir.view(np.uint32)).all(), fname
        assert want.bits.any()


def test_c_example_compiles_and_refuses_auto_with_tune(built_lib, tmp_path):
    exe = tmp_path / "ookd_rx"
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "examples", "ookd_rx.c"), "-o", str(exe),
                        "-L" + os.path.dirname(ok.LIB_PATH), "-lookiedokie_amd",
                        "-Wl,-rpath," + os.path.dirname(ok.LIB_PATH)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    args = ["capture.sc16q11", golden_path("devices", "p3l-nexa2012"), golden_path("filters", "fs32_fs4"), str(RATE)]
    r = subprocess.run([str(exe), "--threshold", "auto", "--tune", "600000"] + args, capture_output=True, text=True)
    assert r.returncode != 0
    assert "--tune" in r.stderr and "auto" in r.stderr
    r = subprocess.run([str(exe), "--tune"], capture_output=True, text=True)       # no value
    assert r.returncode != 0 and "usage" in r.stderr
