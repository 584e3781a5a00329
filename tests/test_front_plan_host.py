"""plan_front (csrc/front_plan.cpp) is a pure function of a context's creation arguments: every band, bound, weight,
tap image and form number it gives equals, bit for bit, what tests/golden/front_plan.json holds
(tools/front_plan_golden.py regenerates the file).  The file was computed from plan_front itself when it was
introduced, not recorded from contexts of the commit before it, so it pins the plan from
then on; tests/test_gpu_front_bounds.py::test_live_context_reports_what_the_plan_recorded and the oracle comparisons
of the gpu suite are what tie it to the kernels' behaviour.  No GPU."""
import json

import pytest

import ookiedokie_amd as ok
from tests import front_plan_cases as P

CASES = P.cases()


@pytest.fixture(scope="module")
def golden():
    with open(P.GOLDEN_FILE) as f:
        return json.load(f)


@pytest.fixture(autouse=True)
def _no_overrides(monkeypatch):
    for v in ("OOKD_FIR_VALU", "OOKD_MFMA_G", "OOKD_MFMA_XCD"):
        monkeypatch.delenv(v, raising=False)


def test_the_file_holds_exactly_the_case_list(golden):
    assert sorted(golden) == sorted(CASES)


@pytest.mark.parametrize("cid", sorted(CASES))
def test_plan_reproduces_the_recorded_front_end(cid, golden):
    case = CASES[cid]
    got = P.digest_entry(P.plan_digest(case, P.make_filter(case["filter"])))
    assert got == golden[cid]


# why a filter stays off the matrix cores, from the arguments alone (not in the file)
@pytest.mark.parametrize("cid, why", [
    ("fs32_fs4-none-thr0.1", "taken"), ("fs128_fs16_dec4-none-thr0.1", "taken"), ("rand256-none-thr0.1", "taken"),
    ("none-none-thr0.1", "not_considered"), ("fs32_fs4-exact_fir-thr0.1", "not_considered"),
    ("fs32_fs4-none-thr0.1-nu0.25", "not_considered"), ("fs32_fs4-none-thr0.1-car2", "not_considered"),
    ("fs32_fs4-fir_valu-thr0.1", "valu_asked"), ("fs128_fs16_dec4-fir_valu-thr1e20", "valu_asked"),
    ("rand257-none-thr0.1", "shape"), ("stages3-none-thr0.1", "shape"), ("dec3-none-thr0.1", "shape"),
])
def test_why_the_matrix_cores_are_not_used(cid, why):
    case = CASES[cid]
    d = P.plan_digest(case, P.make_filter(case["filter"]))
    assert P.MFMA_USE[d.mfma_use] == why
    mfma_forms = (ok.FRONT_FIR1_MFMA, ok.FRONT_FIR2_MFMA, ok.FRONT_FIR1_MFMA_8, ok.FRONT_FIR2_MFMA_8)
    assert (d.form in mfma_forms) == (why == "taken")
    assert (d.image_fnv[1] != 0xcbf29ce484222325) == (why == "taken")         # an A-fragment image only when taken


@pytest.mark.parametrize("thr", ["thr1e-20", "thr1e20"])
@pytest.mark.parametrize("filt", ["fs32_fs4", "fs128_fs16_dec4"])
def test_far_thresholds_refuse_the_matrix_cores(filt, thr):
    """1e-20 / 1e20: p_star = 1e-40 / 1e40 lies outside [2^-100, 2^100] ~ [8e-31, 1.3e30], so the band scaling or the
    range test refuses"""
    case = CASES["%s-none-%s" % (filt, thr)]
    d = P.plan_digest(case, P.make_filter(case["filter"]))
    assert P.MFMA_USE[d.mfma_use] in ("band_scale", "threshold_range")
    assert d.form in (ok.FRONT_FIR1_VALU, ok.FRONT_FIR2_VALU) and d.image_fnv[1] == 0xcbf29ce484222325


def test_refused_arguments_keep_their_error_texts():
    f = P.make_filter("fs32_fs4")
    bad = [(dict(flags=0, nu=0.6, filter=f), "nu must be within [-0.5, 0.5]"),
           (dict(flags=0, nu=0.1, filter=None), "nu != 0 needs a filter"),
           (dict(flags=0, nu=None, carriers=[(0.1, 0.1)], filter=None), "ookd_rx_create_carriers needs a filter"),
           (dict(flags=ok.RX_SAMPLES_CS8 | ok.RX_SAMPLES_CU8, nu=None, filter=f), "are both set"),
           (dict(flags=0, nu=None, filter=ok.Filter.from_stages([(1, [1.0])] * 9)), "filter has 9 stages")]
    for kw, text in bad:
        case = dict(threshold=0.1, carriers=None)
        case.update(kw)
        filt = case.pop("filter")
        with pytest.raises(AssertionError) as e:
            P.plan_digest(case, filt)
        assert text in str(e.value)


# ---- filters the generic kernels' smallest tile does not hold --------------------------------------------------------
# (kernels.hip generic_tile: len_s = D_s (len_{s+1} - 1) + T_s from len_S = 64; (max even + max odd + 2) * 8 B <= 160 KiB)

def _plan_of(stages, **kw):
    case = dict(flags=0, threshold=0.1, nu=None, carriers=None)
    case.update(kw)
    return P.plan_digest(case, ok.Filter.from_stages([(d, [1.0 / t] * t) for d, t in stages]))


@pytest.mark.parametrize("kw, form", [({}, ok.FRONT_GENERIC), (dict(nu=0.2), ok.FRONT_TUNED_GENERIC),
                                      (dict(carriers=[(0.2, 0.1), (-0.31, 0.05)]), ok.FRONT_TUNED_GENERIC)],
                         ids=["untuned", "tuned", "carriers"])
def test_a_filter_that_fits_no_generic_tile_is_refused_by_the_plan(kw, form):
    """the context, the tuned context and the carrier context refuse where they are created, with the total
    decimation, the tap counts and the limit in the text; what fits a smaller tile than 1024 is accepted"""
    for stages, dec, taps, need in (([(4096, 8)], 4096, "[8]", (63 * 4096 + 8 + 2) * 8),
                                    ([(326, 1)], 326, "[1]", (63 * 326 + 1 + 2) * 8),
                                    ([(325, 4)], 325, "[4]", (63 * 325 + 4 + 2) * 8),
                                    # two stages: levels 0 and 1 lie in different buffers
                                    ([(16, 16), (20, 5)], 320, "[16, 5]", (16 * (63 * 20 + 5 - 1) + 16 + 63 * 20 + 5 + 2) * 8)):
        assert need > 160 * 1024
        with pytest.raises(AssertionError) as e:
            _plan_of(stages, **kw)
        text = str(e.value)
        assert ("ookd_rx_create_carriers:" if "carriers" in kw else "ookd_rx_create_tuned:" if "nu" in kw
                else "ookd_rx_create:") in text, text
        assert "total decimation %d " % dec in text and "tap counts %s" % taps in text, text
        assert "%d bytes" % need in text and "163840 bytes" in text and "64 outputs" in text, text
    for stages in ([(64, 64)], [(19, 64)], [(20, 19)], [(325, 3)], [(2, 8)] * 4, [(3, 21), (2, 9), (5, 40)],
                   [(16, 16), (19, 5)]):
        assert _plan_of(stages, **kw).form == form, stages


def test_the_generic_kernels_tile_per_shape():
    """the largest power of two in [64, 1024] whose level buffers fit, worked out by hand in
    tests/front_shapes_inputs.py: the GPU tests of the smaller tiles run the tiles they name"""
    from tests import front_shapes_inputs as S
    for name, shape in dict(S.GENERIC_SHAPES, **S.LARGE_SHAPES).items():
        for kw in ({}, dict(nu=0.2), dict(carriers=[(0.2, 0.1), (-0.31, 0.05)])):
            assert _plan_of(shape, **kw).gen_tile == S.TILES[name], (name, kw)
    assert sorted(set(S.TILES.values())) == [64, 128, 256, 512, 1024]
    assert _plan_of([(1, 256)]).gen_tile == 0 and _plan_of([(325, 3)]).gen_tile == 64


def test_the_fused_shapes_are_never_refused():
    """(their kernels do not build levels in LDS: the limit is the generic kernels' alone)"""
    assert _plan_of([(1, 256)]).form == ok.FRONT_FIR1_MFMA
    assert _plan_of([(2, 16), (2, 32)]).form == ok.FRONT_FIR2_MFMA
