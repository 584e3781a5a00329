"""The carriers survey's contract (include/ookiedokie_amd.h, at ookd_survey_create_carriers) restated in numpy: one
carrier's histogram is the tuned survey's (tests/tuned_survey_contract.py) over the outputs with index 0 (mod S).
Shared by test_survey_carriers_host.py and test_gpu_survey_carriers.py."""
import numpy as np

from tests.test_survey_host import np_hist
from tests.tuned_survey_contract import contract_power


def contract_hist_strided(iq, stages, S):
    """(histogram uint64[256], samples = ceil(floor(n / D) / S))"""
    with np.errstate(over="ignore", invalid="ignore"):
        p = contract_power(iq, stages)[::S]
    return np_hist(p), int(p.size)
