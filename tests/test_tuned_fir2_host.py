"""Host side of the fused tuned two-stage front end (OOKD_RX_TUNED_FIR2 -> OOKD_FRONT_TUNED_FIR2): what plan_front
decides with the flag, that every other context keeps the plan it has without it, the documented quiet rule for two
stages checked against the contract in numpy, and the new constants in the header.  No GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import ookiedokie_amd as ok
from ookiedokie_amd import build as okbuild
from tests import front_plan_cases as P
from tests import tuned_fir2_inputs as T2
from tests.helpers import ROOT, golden_path
from tests.tuned_bounds_inputs import rand_taps
from tests.tuned_contract import SPB, THR, contract_rx, lib_stages

CARRIERS2 = [(0.2, 0.1), (-0.3, 0.05)]


@pytest.fixture(scope="module")
def dec4():
    okbuild.build()
    ok.lib()
    return ok.Filter.load(golden_path("filters", "fs128_fs16_dec4"))


def _digest(filt, flags=0, nu=None, carriers=None, threshold=THR):
    return P.plan_digest(dict(flags=flags, threshold=threshold, nu=nu, carriers=carriers), filt)


def _f32_bits(x):
    return int(np.float32(x).view(np.uint32))


# ---------------------------------------------------------------------------- the plan with the flag ----

@pytest.mark.parametrize("kw", [dict(nu=0.2), dict(carriers=CARRIERS2)], ids=["tuned", "carriers"])
def test_the_flag_selects_the_fused_form(dec4, kw):
    d = _digest(dec4, ok.RX_TUNED_FIR2, **kw)
    base = _digest(dec4, 0, **kw)
    assert base.form == ok.FRONT_TUNED_GENERIC and base.tile_bits == 0 and base.sparse_capable == 0
    assert d.form == ok.FRONT_TUNED_FIR2 == 15 and d.tile_bits == 256 and d.sparse_capable == 1 and d.quiet_lsb == 1
    assert d.gen_tile == 0 and base.gen_tile != 0
    entries = kw.get("carriers") or [(kw["nu"], THR)]
    assert d.num_records == base.num_records == len(entries)
    for k, (nu, thr) in enumerate(entries):
        # finite weights, bit for bit the documented rule recomputed in double and rounded upwards
        qa, qb = T2.quiet_weights(lib_stages(dec4, nu), thr)
        assert np.isfinite(qa) and np.isfinite(qb)
        assert list(d.quiet_bits[k]) == [_f32_bits(qa), _f32_bits(qb)], k
        assert [np.uint32(q).view(np.float32) for q in base.quiet_bits[k]] == [np.inf, np.inf]
        # bands and the bound they come from: those of the plan without the flag
        a, b = P.info_entry(d.info[k]), P.info_entry(base.info[k])
        assert a.pop("form") == 15 and b.pop("form") == 12
        assert a == b
        assert d.info[k].err_valu > 0 and d.info[k].p_lo < d.info[k].p_star < d.info[k].p_hi
    # the same taps; the carrier table differs by the weights alone
    assert list(d.image_fnv)[:3] == list(base.image_fnv)[:3]


def test_no_quiet_skip_refuses_the_weights(dec4):
    d = _digest(dec4, ok.RX_TUNED_FIR2 | ok.RX_NO_QUIET_SKIP, nu=0.2)
    assert d.form == ok.FRONT_TUNED_FIR2 and d.tile_bits == 256 and d.sparse_capable == 0 and d.quiet_lsb == 0
    assert [np.uint32(q).view(np.float32) for q in d.quiet_bits[0]] == [np.inf, np.inf]
    # beyond 1e30: a threshold so small that the weights leave the floats' useful range
    d = _digest(dec4, ok.RX_TUNED_FIR2, nu=0.2, threshold=1e-36)
    assert d.form == ok.FRONT_TUNED_FIR2 and d.quiet_lsb == 0 and d.sparse_capable == 0
    # keep_fir: no sparse output, the weights stay
    d = _digest(dec4, ok.RX_TUNED_FIR2 | ok.RX_KEEP_FIR, nu=0.2)
    assert d.form == ok.FRONT_TUNED_FIR2 and d.quiet_lsb == 1 and d.sparse_capable == 0


# ---------------------------------------------------------------- everything else keeps its plan ----

def _two(n1, n2, d1=2, d2=2):
    return ok.Filter.from_stages([(d1, rand_taps(n1, 100 + n1)), (d2, rand_taps(n2, 200 + n2))])


STAY = {
    "exact_fir": (lambda f: f, ok.RX_EXACT_FIR),
    "taps17_32": (lambda f: _two(17, 32), 0),
    "taps16_33": (lambda f: _two(16, 33), 0),
    "dec2_4": (lambda f: _two(16, 32, 2, 4), 0),
    "one_stage": (lambda f: ok.Filter.from_stages([(2, rand_taps(16, 3))]), 0),
}


@pytest.mark.parametrize("kw", [dict(nu=0.2), dict(carriers=CARRIERS2)], ids=["tuned", "carriers"])
@pytest.mark.parametrize("name", sorted(STAY))
def test_contexts_that_stay_on_the_generic_form(dec4, name, kw):
    make, extra = STAY[name]
    filt = make(dec4)
    with_flag = _digest(filt, ok.RX_TUNED_FIR2 | extra, **kw)
    without = _digest(filt, extra, **kw)
    assert with_flag.form == ok.FRONT_TUNED_GENERIC == 12
    assert P.digest_entry(with_flag) == P.digest_entry(without)
    assert with_flag.gen_tile == without.gen_tile != 0


def test_shapes_at_the_limit_take_the_fused_form(dec4):
    for n1, n2 in ((16, 32), (15, 31), (1, 1), (16, 1), (1, 32)):
        assert _digest(_two(n1, n2), ok.RX_TUNED_FIR2, nu=-0.37).form == ok.FRONT_TUNED_FIR2, (n1, n2)


@pytest.mark.parametrize("nu", [None, 0.0, -0.0])
def test_untuned_contexts_ignore_the_flag(dec4, nu):
    for filt in (dec4, ok.Filter.load(golden_path("filters", "fs32_fs4")), None):
        for extra in (0, ok.RX_FIR_VALU, ok.RX_EXACT_FIR):
            a, b = _digest(filt, ok.RX_TUNED_FIR2 | extra, nu=nu), _digest(filt, extra, nu=nu)
            assert P.digest_entry(a) == P.digest_entry(b)
            assert a.form not in (ok.FRONT_TUNED_FIR2, ok.FRONT_TUNED_GENERIC, ok.FRONT_TUNED_FIR1)


def test_the_one_stage_tuned_plans_ignore_the_flag():
    fs32 = ok.Filter.load(golden_path("filters", "fs32_fs4"))
    for kw, form in ((dict(nu=0.25), ok.FRONT_TUNED_FIR1), (dict(carriers=CARRIERS2), ok.FRONT_TUNED_MULTI)):
        a, b = _digest(fs32, ok.RX_TUNED_FIR2, **kw), _digest(fs32, 0, **kw)
        assert a.form == form and P.digest_entry(a) == P.digest_entry(b)


def test_plans_without_the_flag_are_the_recorded_ones():
    """every case of tests/golden/front_plan.json on fs128_fs16_dec4, as recorded"""
    import json
    with open(P.GOLDEN_FILE) as f:
        golden = json.load(f)
    cases = {cid: c for cid, c in P.cases().items() if c["filter"] == "fs128_fs16_dec4"}
    assert len(cases) > 30
    for cid, case in cases.items():
        assert P.digest_entry(P.plan_digest(case, P.make_filter(case["filter"]))) == golden[cid], cid


# ------------------------------------------------------------------------- the rule itself ----

# interior tiles, tiles the rule takes, tiles whose contract bits are all zero (nu = 0.2, -0.3 and 0.5 alike: the
# spread term decides, and the noise is that of the capture's name and nu)
CENSUS = {"G1": (1191, 893, 911), "G2": (410, 176, 184)}


@pytest.mark.parametrize("nu", T2.NUS, ids=T2.NU_IDS)
@pytest.mark.parametrize("cap", ["G1", "G2"])
def test_the_documented_rule_takes_no_tile_that_holds_a_one(dec4, record_property, cap, nu):
    _, iq, _ = T2.moved_golden(cap, nu)
    stages = lib_stages(dec4, nu)
    bits, _ = contract_rx(iq, stages, THR, SPB)
    c = T2.quiet_census(iq, stages, THR, bits)
    A, G, e = T2.rule_terms(stages)
    record_property("census", c)
    print(cap, nu, c, "A %.4f G %.3g e %.3g" % (A, G, e))
    assert c["bad"] == 0
    assert abs(A - 1.378) < 1e-3 and e < 2e-5
    if nu == 1.0 / 3000.0:
        # the DC term sits in the pass band: the offset alone is loud, the rule takes nothing and (nearly) every
        # output is a one
        assert abs(G - 0.9997) < 1e-4 and c["taken"] == 0 and c["zero"] == 0 and c["interior"] == CENSUS[cap][0]
        assert bits[T2.F:].mean() > 0.98
    else:
        assert G < 1e-5
        assert (c["interior"], c["taken"], c["zero"]) == CENSUS[cap]
        # the float32 form the kernel evaluates decides these windows alike: none lies within rounding of the edge
        assert c["taken32"] == c["taken"]


# ------------------------------------------------------------------------------- constants ----

def test_the_header_constants_equal_the_python_mirror(dec4, tmp_path):
    src = tmp_path / "fir2.c"
    src.write_text('#include <stdio.h>\n#include "ookiedokie_amd.h"\n'
                   'int main(void) {\n'
                   '  printf("%u %d %d %d %d\\n", (unsigned) OOKD_RX_TUNED_FIR2, OOKD_FRONT_TUNED_FIR2,\n'
                   '         OOKD_FRONT_TUNED_GENERIC, (int) sizeof(ookd_rx_config), (int) sizeof(ookd_front_info));\n'
                   '  return 0; }\n')
    exe = tmp_path / "fir2"
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True).stdout.split()]
    assert out == [ok.RX_TUNED_FIR2, ok.FRONT_TUNED_FIR2, ok.FRONT_TUNED_GENERIC, C.sizeof(ok.RxConfig), C.sizeof(ok.FrontInfo)]
    assert (ok.RX_TUNED_FIR2, ok.FRONT_TUNED_FIR2) == (1 << 12, 15)
    flags = [getattr(ok, n) for n in dir(ok) if n.startswith("RX_") and n not in ("RX_MAX_CARRIERS", "RX_FMT_PRETTY", "RX_FMT_CSV")]
    assert len(set(flags)) == len(flags)                # no flag bit is used twice


def test_receiver_takes_the_keyword():
    import inspect
    assert inspect.signature(ok.Receiver.__init__).parameters["tuned_fir2"].default is False
