"""Host side of the carrier contexts (ookd_rx_create_carriers): the new declarations compile as C99 against the header
and the library, the argument refusals happen before any HIP call, Receiver's `carriers` argument, and
examples/ookd_scan.c -- which now decodes through a carrier context -- still builds."""
import ctypes as C
import os
import subprocess

import pytest

import ookiedokie_amd as ok
from ookiedokie_amd import build as okbuild
from tests.helpers import ROOT, golden_path
from tests.test_tuned_survey_host import build_scan


@pytest.fixture(scope="module")
def built_lib():
    okbuild.build()
    return ok.lib()


@pytest.fixture(scope="module")
def fs32(built_lib):
    return ok.Filter.load(golden_path("filters", "fs32_fs4"))


def _create(L, filt, entries, *, reserved=0, max_captures=0, null=False, count=None, hip_device=0):
    cfg = ok.RxConfig()
    cfg.hip_device = hip_device
    cfg.threshold = 0.1
    cfg.samples_per_buffer = 8192
    cfg.max_samples = 8192
    cfg.max_captures = max_captures
    arr = (ok.RxCarrier * max(len(entries), 1))()
    for k, (nu, thr) in enumerate(entries):
        arr[k].nu, arr[k].threshold = nu, thr
        arr[k].reserved[4] = reserved
    h = L.ookd_rx_create_carriers(C.byref(cfg), filt, None, None if null else arr,
                                  len(entries) if count is None else count)
    return h, ok.last_error()


def test_new_declarations_compile_and_link(built_lib, tmp_path):
    for name in ("ookd_rx_create_carriers", "ookd_rx_num_carriers", "ookd_rx_get_carrier",
                 "ookd_rx_get_carrier_front_info"):
        assert hasattr(built_lib, name), name
    src = tmp_path / "carriers.c"
    src.write_text('#include <stdio.h>\n#include <string.h>\n#include "ookiedokie_amd.h"\n'
                   'int main(void) {\n'
                   '  ookd_rx_carrier c[2]; ookd_rx_carrier back; ookd_front_info info; ookd_rx_config cfg;\n'
                   '  memset(c, 0, sizeof(c)); memset(&cfg, 0, sizeof(cfg));\n'
                   '  c[0].nu = 0.2; c[0].threshold = 0.1f; c[1].nu = -0.3; c[1].threshold = 0.05f;\n'
                   '  cfg.samples_per_buffer = 8192; cfg.max_samples = 8192;\n'
                   '  ookd_rx *rx = ookd_rx_create_carriers(&cfg, NULL, NULL, c, 2);       /* no filter: refused */\n'
                   '  printf("%d %d %d %d %u %d %d\\n", OOKD_FRONT_TUNED_MULTI, OOKD_RX_MAX_CARRIERS, (int) sizeof(c[0]),\n'
                   '         rx == NULL, ookd_rx_num_carriers(NULL), ookd_rx_get_carrier(NULL, 0, &back) != 0,\n'
                   '         ookd_rx_get_carrier_front_info(NULL, 0, &info) != 0);\n'
                   '  puts(ookd_last_error());\n'
                   '  return 0; }\n')
    exe = tmp_path / "carriers"
    lib_dir = os.path.dirname(ok.LIB_PATH)
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o",
                        str(exe), "-L" + lib_dir, "-lookiedokie_amd", "-Wl,-rpath," + lib_dir],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = subprocess.run([str(exe)], capture_output=True, text=True).stdout.split("\n")
    assert [int(x) for x in out[0].split()] == [14, 16, 32, 1, 0, 1, 1]
    assert "bad argument" in out[1]
    assert (ok.FRONT_TUNED_MULTI, ok.RX_MAX_CARRIERS, C.sizeof(ok.RxCarrier)) == (14, 16, 32)


def test_create_refusals_need_no_gpu(built_lib, fs32):
    L = built_lib

    def refused(*words, filt=fs32._h, **kw):
        entries = kw.pop("entries", [(0.2, 0.1)])
        h, err = _create(L, filt, entries, **kw)
        assert not h
        for w in words:
            assert w in err, (w, err)
        assert "no CPU fallback" not in err, err         # refused on its arguments, before any HIP call

    refused("ookd_rx_create_carriers", "1 to 16", entries=[])
    refused("1 to 16", "17", entries=[(0.01 * k, 0.1) for k in range(17)])
    refused("NULL", null=True)
    refused("carrier 1", "[-0.5, 0.5]", entries=[(0.2, 0.1), (float("nan"), 0.1)])
    refused("carrier 0", "[-0.5, 0.5]", entries=[(0.51, 0.1)])
    refused("carrier 0", "[-0.5, 0.5]", entries=[(-0.500001, 0.1)])
    refused("needs a filter", filt=None)
    refused("carrier 0", "reserved", entries=[(0.2, 0.1), (0.2, 0.2)], reserved=7)
    refused("one capture per run", max_captures=2)
    # valid arguments reach the device check: without a HIP device (or with device -1) that is said loudly
    for entries in ([(0.2, 0.1)], [(0.0, 0.1), (0.2, 0.1), (0.2, 0.05), (-0.5, 0.1)]):
        h, err = _create(L, fs32._h, entries, hip_device=-1, max_captures=1)
        assert not h and ("no CPU fallback" in err or "out of range" in err), err


def test_without_a_hip_device_create_fails_loudly(built_lib, fs32):
    import torch
    if torch.cuda.is_available():
        rx = ok.Receiver(fs32, None, max_samples=1 << 16, carriers=[0.2, (-0.3, 0.05)])
        assert rx.num_carriers == 2
        rx.close()
    else:
        with pytest.raises(ok.OokdError, match="no CPU fallback"):
            ok.Receiver(fs32, None, max_samples=1 << 16, carriers=[0.2, (-0.3, 0.05)])


def test_receiver_carrier_arguments(fs32):
    for kw in ({"tune": 0.1}, {"tune": 0.0}, {"tune_hz": 1e5, "sample_rate": 3e6}):
        with pytest.raises(ValueError, match="mutually exclusive"):
            ok.Receiver(fs32, None, max_samples=64, carriers=[0.2], **kw)
    with pytest.raises(ValueError):
        ok.Receiver(fs32, None, max_samples=64, carriers=[0.2], sample_format="cf32")
    with pytest.raises((TypeError, ValueError)):
        ok.Receiver(fs32, None, max_samples=64, carriers=[(0.2, 0.1, 3)])
    # the library's refusals come through as OokdError with its message
    with pytest.raises(ok.OokdError, match="1 to 16"):
        ok.Receiver(fs32, None, max_samples=64, carriers=[])
    with pytest.raises(ok.OokdError, match="carrier 1"):
        ok.Receiver(fs32, None, max_samples=64, carriers=[0.1, 0.7])


def test_scan_example_still_builds(built_lib, tmp_path):
    exe = build_scan(tmp_path)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode != 0 and "usage" in r.stderr and r.stdout == ""
    with open(os.path.join(ROOT, "examples", "ookd_scan.c")) as f:
        assert "ookd_rx_create_carriers" in f.read()
