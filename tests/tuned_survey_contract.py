"""The tuned envelope survey's contract (include/ookiedokie_amd.h, at ookd_survey_create_tuned) restated in numpy:
the histogram is np_hist of the power of contract_stage chained over the capture's own n samples, unpadded.  Built
from tests/tuned_contract.py (the four statements) and tests/test_survey_host.py (the bin rule).  Shared by
test_tuned_survey_host.py and test_gpu_tuned_survey.py."""
import numpy as np

from tests.helpers import golden_path
from tests.test_survey_host import np_hist
from tests.tuned_contract import RATE, SPB, contract_rx, contract_stage

DC = 400.0 * (1 + 0.5j)
NOISE = 40


def unpack(iq):
    iq = np.asarray(iq, dtype=np.int16).reshape(-1)
    s = np.float32(1.0 / 2048.0)
    return iq[0::2].astype(np.float32) * s, iq[1::2].astype(np.float32) * s


def contract_power(iq, stages):
    """stages: [(decimation, re, im)] float32 taps -> float32 power of the first floor(n / D) outputs from zero
    history; no input at or beyond n exists"""
    xr, xi = unpack(iq)
    for D, re, im in stages:
        xr, xi = contract_stage(xr, xi, np.asarray(re, np.float32), np.asarray(im, np.float32), int(D))
    with np.errstate(over="ignore", invalid="ignore"):
        rr = xr * xr
        ii = xi * xi
        p = rr + ii
    assert p.dtype == np.float32
    return p


def contract_hist(iq, stages):
    """(histogram uint64[256], samples)"""
    with np.errstate(over="ignore", invalid="ignore"):
        p = contract_power(iq, stages)
    return np_hist(p), int(p.size)


def decode(oracle, odev, iq, stages, threshold, spb=SPB):
    """contract_rx's bits at `threshold` through the oracle's state machine: (msg samples, payloads, err samples)"""
    bits, _ = contract_rx(iq, stages, threshold, spb)
    return oracle.sm_stream(odev, bits, spb)


def oracle_device(oracle, name, decimation=1):
    od, _ = oracle.load_device_json(golden_path("devices", name), RATE // decimation)
    return od
