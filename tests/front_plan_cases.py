"""The case list of tests/golden/front_plan.json and the decoding of ookd_front_plan_digest's result, shared by
tests/test_front_plan_host.py, the live-context test in tests/test_gpu_front_bounds.py and tools/front_plan_golden.py."""
import ctypes as C
import json
import os
import struct

import numpy as np

import ookiedokie_amd as ok
from tests.helpers import GOLDEN, golden_path
from tests.tuned_bounds_inputs import rand_taps

GOLDEN_FILE = os.path.join(GOLDEN, "front_plan.json")

FLAGS = {"none": 0, "fir_valu": ok.RX_FIR_VALU, "exact_fir": ok.RX_EXACT_FIR, "no_quiet_skip": ok.RX_NO_QUIET_SKIP,
         "keep_fir": ok.RX_KEEP_FIR, "cs8": ok.RX_SAMPLES_CS8, "cu8": ok.RX_SAMPLES_CU8}
# (1e-20 / 1e20: the band scaling or the 2^+-100 test keeps the filter off the matrix cores)
THRESHOLDS = {"thr0.1": 0.1, "thr0": 0.0, "thrnan": float("nan"), "thr1e-20": 1e-20, "thr1e20": 1e20}
TUNES = {"nu0": 0.0, "nu3000th": 1.0 / 3000.0, "nu0.25": 0.25, "nu-0.5": -0.5}
_NUS16 = [(-0.45 + 0.06 * k, (0.1, 0.02, 0.5, 3.0)[k % 4]) for k in range(16)]
CARRIERS = {"car1": [(0.2, 0.1)],
            "car2": [(0.25, 0.1), (-0.125, 0.0)],            # threshold 0: no quiet test, infinite weights
            "car16": _NUS16[:5] + [(0.0, 0.0)] + _NUS16[6:]}


def _stages(name):
    if name == "none":
        return None
    if name.startswith("rand"):                 # 1 stage, decimation 1, that many taps
        n = int(name[4:])
        return [(1, rand_taps(n, 1000 + n))]
    if name in ("big_tap", "tiny_tap"):
        h = rand_taps(48, 7)
        h[5] = 1e15 if name == "big_tap" else 1e-15
        return [(1, h)]
    if name == "stages3":
        return [(2, rand_taps(12, 11)), (1, rand_taps(33, 12)), (2, rand_taps(20, 13))]
    if name == "dec3":
        return [(3, rand_taps(40, 14))]
    raise KeyError(name)


FILTERS = ["none", "unity1", "unity16", "fs32_fs4", "fs128_fs16_dec4", "rand64", "rand255", "rand256", "rand257",
           "big_tap", "tiny_tap", "stages3", "dec3"]


def make_filter(name):
    if name in ("unity1", "unity16", "fs32_fs4", "fs128_fs16_dec4"):
        return ok.Filter.load(golden_path("filters", name))
    st = _stages(name)
    return None if st is None else ok.Filter.from_stages(st)


def cases():
    """case id -> dict(filter, flags, threshold, nu, carriers): every filter at the default flags; every flag and
    every threshold on fs32_fs4 and fs128_fs16_dec4; the tuned and carrier cases on fs32_fs4, the 255-tap filter and
    the 3-stage filter"""
    out = {}

    def add(filt, flag="none", thr="thr0.1", nu=None, car=None):
        cid = "-".join([filt, flag, thr] + ([nu] if nu else []) + ([car] if car else []))
        out[cid] = dict(filter=filt, flags=FLAGS[flag], threshold=THRESHOLDS[thr], nu=TUNES[nu] if nu else None,
                        carriers=CARRIERS[car] if car else None)

    for f in FILTERS:
        add(f)
    add("none", "cs8")          # (the one form number the lists below do not reach: OOKD_FRONT_NO_FILTER_8)
    for f in ("fs32_fs4", "fs128_fs16_dec4"):
        for flag in FLAGS:
            for thr in THRESHOLDS:
                add(f, flag, thr)
    for f in ("fs32_fs4", "rand255", "stages3"):
        for nu in TUNES:
            add(f, nu=nu)
        for car in CARRIERS:
            add(f, car=car)
        add(f, "exact_fir", nu="nu0.25")
        add(f, "no_quiet_skip", car="car2")
    return out


class PlanDigest(C.Structure):
    _fields_ = [("num_records", C.c_uint32), ("form", C.c_uint32), ("tile_bits", C.c_uint32),
                ("sparse_capable", C.c_uint32), ("mfma_g", C.c_uint32), ("mfma_xcd", C.c_uint32),
                ("quiet_lsb", C.c_int32), ("mfma_use", C.c_uint32), ("band_bits", C.c_uint32 * 4),
                ("image_fnv", C.c_uint64 * 4), ("info", ok.FrontInfo * ok.RX_MAX_CARRIERS),
                ("quiet_bits", (C.c_uint32 * 2) * ok.RX_MAX_CARRIERS), ("gen_tile", C.c_uint32)]


MFMA_USE = ("taken", "not_considered", "valu_asked", "shape", "band_scale", "threshold_range")


def carrier_array(carriers):
    arr = (ok.RxCarrier * max(len(carriers or ()), 1))()
    for k, (nu, thr) in enumerate(carriers or ()):
        arr[k].nu, arr[k].threshold = nu, thr
    return arr


def plan_digest(case, filt):
    """ookd_front_plan_digest (a test aid of the library, not in the public header) for one case"""
    fn = ok.lib().ookd_front_plan_digest
    fn.restype = C.c_int
    fn.argtypes = [C.c_uint32, C.c_float, C.c_void_p, C.c_double, C.c_void_p, C.c_uint32, C.POINTER(PlanDigest)]
    out = PlanDigest()
    car = case["carriers"] or []
    rc = fn(case["flags"], case["threshold"], filt._h if filt else None, case["nu"] or 0.0, carrier_array(car),
            len(car), C.byref(out))
    assert rc == 0, ok.last_error()
    return out


def _f32(x):
    return "0x%08x" % struct.unpack("<I", struct.pack("<f", x))[0]


def _f64(x):
    return "0x%016x" % struct.unpack("<Q", struct.pack("<d", x))[0]


def info_entry(f):
    """a FrontInfo (or Receiver.front_info()'s dict) as the file holds it: floats as bit patterns"""
    g = f if isinstance(f, dict) else {n: getattr(f, n) for n, _ in ok.FrontInfo._fields_}
    e = {"form": int(g["form"]), "mfma_ksteps": int(g["mfma_ksteps"])}
    e.update({n: _f32(g[n]) for n in ("p_star", "p_lo", "p_hi", "mfma_c")})
    e.update({n: _f64(g[n]) for n in ("err_nominal", "err_wide", "err_valu", "mfma_delta")})
    return e


def digest_entry(d):
    """a PlanDigest as the file holds it (mfma_use is not in the file: test_front_plan_host.py reasons about it)"""
    n = d.num_records
    return {"form": d.form, "tile_bits": d.tile_bits, "sparse_capable": d.sparse_capable, "mfma_g": d.mfma_g,
            "mfma_xcd": d.mfma_xcd, "quiet_lsb": d.quiet_lsb, "bands": ["0x%08x" % b for b in d.band_bits],
            "images": ["0x%016x" % h for h in d.image_fnv], "info": [info_entry(d.info[k]) for k in range(n)],
            "quiet": [["0x%08x" % q for q in d.quiet_bits[k]] for k in range(n)]}


def receiver_kwargs(case):
    """Receiver keywords of a case (the flags as its booleans)"""
    fl = case["flags"]
    kw = dict(threshold=case["threshold"], fir_valu=bool(fl & ok.RX_FIR_VALU), exact_fir=bool(fl & ok.RX_EXACT_FIR),
              quiet_skip=not fl & ok.RX_NO_QUIET_SKIP, keep_fir=bool(fl & ok.RX_KEEP_FIR),
              sample_format="cs8" if fl & ok.RX_SAMPLES_CS8 else "cu8" if fl & ok.RX_SAMPLES_CU8 else "sc16q11")
    if case["carriers"]:
        kw["carriers"] = case["carriers"]
    elif case["nu"] is not None:
        kw["tune"] = case["nu"]
    return kw
