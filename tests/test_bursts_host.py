"""CPU-side tests of burst extraction: the new symbols and layouts, ookd_find_bursts against its restatement
(tests/bursts_contract.py) on designed and random edge lists, its refusals, and the round trip the feature is for --
the golden captures cut by the host rule and decoded again by the reference decoder, which pins the margins the GPU
test uses before the GPU is asked."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests.bursts_contract import (FIELDS, RATE, SPB, THR, assert_table, bursts_of, cut_of, designed_cases, mapped_samples,
                                   margins, random_case, total_of)
from tests.helpers import golden_path
from tests.pulse_contract import golden_iq, oracle_edges

import ookiedokie_amd as ok
from ookiedokie_amd import build as okbuild

INCLUDE = os.path.dirname(ok.HEADER_PATH)
FILTERS = ("fs32_fs4", "fs128_fs16_dec4")


@pytest.fixture(scope="session", autouse=True)
def built_lib():
    okbuild.build()
    return ok.lib()


# ---- interface --------------------------------------------------------------------------------------------

def test_new_symbols_are_exported(built_lib):
    for name in ("ookd_find_bursts", "ookd_rx_bursts", "ookd_rx_get_burst_info", "ookd_rx_get_bursts",
                 "ookd_rx_copy_bursts_device", "ookd_rx_copy_bursts_host", "ookd_rx_bursts_kernel_ms",
                 "ookd_rx_burst_copy_kernel_ms"):
        assert hasattr(built_lib, name), name
    assert hasattr(ok, "find_bursts") and hasattr(ok, "Burst") and hasattr(ok, "BurstInfo") and ok.BURSTS_CLEAN == 1
    for name in ("bursts", "burst_samples", "burst_samples_device", "message_bursts", "bursts_kernel_ms",
                 "burst_copy_kernel_ms"):
        assert hasattr(ok.Receiver, name), name
    assert built_lib.ookd_rx_bursts_kernel_ms(None) == 0.0 and built_lib.ookd_rx_burst_copy_kernel_ms(None) == 0.0
    assert built_lib.ookd_api_version() == 1                    # symbols were added, nothing else


def test_null_context_needs_no_gpu(built_lib):
    info = ok.BurstInfo()
    n = C.c_uint64(7)
    assert built_lib.ookd_rx_bursts(None, 1, 1, 2, 0) == -1 and "NULL" in ok.last_error()
    assert built_lib.ookd_rx_get_burst_info(None, 0, C.byref(info)) == -1 and "NULL" in ok.last_error()
    assert built_lib.ookd_rx_get_bursts(None, 0, None, 0, C.byref(n)) == -1
    assert built_lib.ookd_rx_copy_bursts_device(None, 0, None, 0) == -1
    assert built_lib.ookd_rx_copy_bursts_host(None, 0, None, 0) == -1


def test_header_is_c99_and_the_layouts_match(tmp_path):
    src = tmp_path / "b.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ookiedokie_amd.h"\n'
                   'int main(void) {\n'
                   '  uint64_t nb = 9, total = 9;\n'
                   '  if (ookd_rx_bursts(NULL, 0, 0, 0, 0) != OOKD_ERR_ARG || ookd_rx_get_burst_info(NULL, 0, NULL) != OOKD_ERR_ARG\n'
                   '      || ookd_rx_get_bursts(NULL, 0, NULL, 0, NULL) != OOKD_ERR_ARG\n'
                   '      || ookd_rx_copy_bursts_device(NULL, 0, NULL, 0) != OOKD_ERR_ARG\n'
                   '      || ookd_rx_copy_bursts_host(NULL, 0, NULL, 0) != OOKD_ERR_ARG\n'
                   '      || ookd_rx_bursts_kernel_ms(NULL) != 0.0f || ookd_rx_burst_copy_kernel_ms(NULL) != 0.0f\n'
                   '      || ookd_find_bursts(NULL, 0, 10, 1, 10, 1, 1, 2, NULL, 0, &nb, &total) != OOKD_OK || nb || total) return 1;\n'
                   '  printf("%d %d %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu", OOKD_API_VERSION, OOKD_BURSTS_CLEAN,\n'
                   '    sizeof(ookd_burst), offsetof(ookd_burst, first_sample), offsetof(ookd_burst, num_samples),\n'
                   '    offsetof(ookd_burst, offset), offsetof(ookd_burst, first_run), offsetof(ookd_burst, num_runs),\n'
                   '    sizeof(ookd_burst_info), offsetof(ookd_burst_info, max_gap), offsetof(ookd_burst_info, flags),\n'
                   '    offsetof(ookd_burst_info, sample_bytes), offsetof(ookd_burst_info, tile_edges),\n'
                   '    offsetof(ookd_burst_info, decimation));\n'
                   '  return 0; }\n')
    exe = tmp_path / "b"
    libdir = os.path.dirname(ok.LIB_PATH)
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", INCLUDE, str(src), "-o", str(exe),
                        "-L", libdir, "-lookiedokie_amd", "-Wl,-rpath," + libdir], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    got = [int(x) for x in out.stdout.split()]
    B, I = ok.Burst, ok.BurstInfo
    assert got == [1, 1, C.sizeof(B), B.first_sample.offset, B.num_samples.offset, B.offset.offset, B.first_run.offset,
                   B.num_runs.offset, C.sizeof(I), I.max_gap.offset, I.flags.offset, I.sample_bytes.offset,
                   I.tile_edges.offset, I.decimation.offset]
    assert C.sizeof(B) == 40 and C.sizeof(I) == 64


# ---- the rule ---------------------------------------------------------------------------------------------

def _check_case(case):
    name, e, n_out, D, n, pre, post, max_gap = case
    want = bursts_of(e, n_out, D, n, pre, post, max_gap)
    got = ok.find_bursts(e, n_out, D, n, pre, post, max_gap)
    assert_table(got, want, (name, e))
    return want


@pytest.mark.parametrize("case", designed_cases(), ids=[c[0] for c in designed_cases()])
def test_designed_lists(case):
    want = _check_case(case)
    name = case[0]
    # each case is what its name says
    if name == "E=0":
        assert want == []
    if name in ("E=1 open", "odd E, open last run"):
        assert want[-1]["hi"] == case[2]
    if name == "gap of exactly max_gap joins":
        assert len(want) == 1 and want[0]["burst_runs"] == 2
    if name == "gap of max_gap + 1 splits":
        assert len(want) == 2
    if name in ("pre beyond the first rise", "rise at 0"):
        assert want[0]["lo"] == 0 and want[0]["first_sample"] == 0
    if name == "post beyond n_out":
        assert want[-1]["hi"] == case[2]
    if name == "n_out D > n: clipped at n":
        assert want[-1]["first_sample"] + want[-1]["num_samples"] == case[4] < want[-1]["hi"] * case[3]
    if name == "a burst wholly in the padding":
        assert len(want) == 2 and want[1]["num_samples"] == 0 and want[1]["first_sample"] == case[4]
    if name == "two bursts in the padding":
        assert [b["num_samples"] for b in want[1:]] == [0, 0] and want[2]["offset"] == want[1]["offset"] == total_of(want)
    if name == "every run its own burst":
        assert len(want) == 9 and all(b["burst_runs"] == 1 for b in want)
    if name == "all runs one burst":
        assert len(want) == 1 and want[0]["burst_runs"] == 9
    # bursts never overlap, and the offsets are the running sum
    for a, b in zip(want, want[1:]):
        assert a["hi"] <= b["lo"] and a["first_sample"] + a["num_samples"] <= b["first_sample"]
        assert b["offset"] == a["offset"] + a["num_samples"]


def test_random_lists():
    rng = np.random.default_rng(2024)
    seen = set()
    for _ in range(400):
        case = random_case(rng)
        want = _check_case(case)
        seen.add(min(len(want), 3))
        if any(b["num_samples"] == 0 for b in want):
            seen.add("empty")
        if len(case[1]) % 2:
            seen.add("open")
    assert seen >= {0, 1, 2, 3, "empty", "open"}


def test_capacity_convention():
    e = np.array([10, 20, 100, 120, 300, 310], dtype=np.uint64)
    table = np.full((2, 5), 77, dtype=np.uint64)
    nb, total = C.c_uint64(0), C.c_uint64(0)
    f = ok.lib().ookd_find_bursts
    assert f(e.ctypes.data, 6, 1000, 1, 1000, 1, 2, 3, table.ctypes.data, 1, C.byref(nb), C.byref(total)) == 0
    assert nb.value == 3 and total.value == 13 + 23 + 13
    assert table[0].tolist() == [9, 13, 0, 0, 1] and table[1].tolist() == [77] * 5      # one entry stored, no more
    assert f(e.ctypes.data, 6, 1000, 1, 1000, 1, 2, 3, None, 5, C.byref(nb), None) == 0 and nb.value == 3
    assert f(e.ctypes.data, 6, 1000, 1, 1000, 1, 2, 3, None, 0, None, None) == 0


def test_refusals():
    e = np.array([10, 20], dtype=np.uint64)
    nb = C.c_uint64(0)
    f = ok.lib().ookd_find_bursts
    assert f(e.ctypes.data, 2, 100, 1, 100, 3, 4, 6, None, 0, C.byref(nb), None) == -1 and "max_gap" in ok.last_error()
    assert f(e.ctypes.data, 2, 100, 1, 100, 2 ** 64 - 1, 2, 2 ** 64 - 1, None, 0, C.byref(nb), None) == -1      # (pre + post wraps)
    assert f(e.ctypes.data, 2, 100, 1, 100, 3, 4, 7, None, 0, C.byref(nb), None) == 0
    assert f(None, 2, 100, 1, 100, 3, 4, 7, None, 0, C.byref(nb), None) == -1 and "NULL" in ok.last_error()
    assert f(None, 0, 100, 1, 100, 3, 4, 7, None, 0, C.byref(nb), None) == 0 and nb.value == 0
    assert f(e.ctypes.data, 2, 100, 0, 100, 3, 4, 7, None, 0, C.byref(nb), None) == -1 and "decimation" in ok.last_error()
    with pytest.raises(ok.OokdError) as err:
        ok.find_bursts(e, 100, 1, 100, 3, 4, 6)
    assert err.value.code == -1


# ---- the round trip through the reference decoder --------------------------------------------------------

@pytest.mark.parametrize("filt", FILTERS)
@pytest.mark.parametrize("name", ["G1", "G2"])
def test_cut_decodes_like_the_whole_capture(oracle, vectors, name, filt):
    g = vectors[name]
    iq = golden_iq(vectors, name)
    n = iq.size // 2
    fir = oracle.load_filter_json(golden_path("filters", filt))
    D = fir.total_decimation
    fsm, _ = oracle.load_device_json(golden_path("devices", g["device"]), RATE // D)
    whole = oracle.rx(iq, fir, THR, fsm, SPB)
    assert len(whole.msg_samples) >= 1
    e, n_out = oracle_edges(oracle, iq, filt)
    pre, post, max_gap = margins(D)
    want = bursts_of(e, n_out, D, n, pre, post, max_gap)
    got = ok.find_bursts(e, n_out, D, n, pre, post, max_gap)
    assert_table(got, want, (name, filt))
    assert 1 <= len(want) and total_of(want) < n                # something was left out
    cut = cut_of(iq, want).reshape(-1)
    again = oracle.rx(cut, fir, THR, fsm, SPB)
    assert again.payloads.tolist() == whole.payloads.tolist()
    mapped, which = mapped_samples(whole.msg_samples, want, D)
    assert again.msg_samples.tolist() == mapped, (which, whole.msg_samples.tolist())
    assert again.err_samples.size == whole.err_samples.size
