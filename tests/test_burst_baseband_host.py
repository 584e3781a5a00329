"""CPU-side tests of the burst basebands: the new symbols and layouts, the table rule ookd_baseband_bursts and the
contract on the host ookd_baseband_of against their restatement (tests/burst_baseband_contract.py), the refusals, and
the round trip the feature is for -- the reference's filter output of the golden captures cut by the table, quantised
to SC16Q11 and decoded again by the reference decoder without a filter at the decimated rate, which pins on the
reference what the GPU test then asks of the kernel."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests.burst_baseband_contract import (FIELDS, assert_table, baseband_cut_of, baseband_table_of, q16, rows_of, same_bits,
                                           tiles_filtered_of, total_of, turn_of)
from tests.bursts_contract import RATE, SPB, THR, bursts_of, designed_cases, mapped_samples, margins, random_case, table_of
from tests.helpers import edges_of, golden_path
from tests.pulse_contract import golden_iq

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
    for name in ("ookd_baseband_bursts", "ookd_baseband_of", "ookd_rx_get_baseband_info", "ookd_rx_get_baseband_bursts",
                 "ookd_rx_burst_baseband_device", "ookd_rx_burst_baseband_host", "ookd_rx_baseband_kernel_ms"):
        assert hasattr(built_lib, name), name
    assert hasattr(ok, "baseband_bursts") and hasattr(ok, "baseband_of") and hasattr(ok, "BasebandBurst") and hasattr(ok, "BasebandInfo")
    assert ok.BASEBAND_CF32 == 0 and ok.BASEBAND_SC16Q11 == 1
    for name in ("burst_baseband", "burst_baseband_device", "baseband_info", "baseband_kernel_ms"):
        assert hasattr(ok.Receiver, name), name
    assert built_lib.ookd_rx_baseband_kernel_ms(None) == 0.0
    assert built_lib.ookd_api_version() == 1                    # symbols were added, nothing else


def test_null_context_needs_no_gpu(built_lib):
    info = ok.BasebandInfo()
    n = C.c_uint64(7)
    assert built_lib.ookd_rx_get_baseband_info(None, 0, C.byref(info)) == -1 and "NULL" in ok.last_error()
    assert built_lib.ookd_rx_get_baseband_bursts(None, 0, None, 0, C.byref(n)) == -1 and "NULL" in ok.last_error()
    for fmt in (0, 1):
        assert built_lib.ookd_rx_burst_baseband_device(None, 0, fmt, None, 0) == -1 and "NULL" in ok.last_error()
        assert built_lib.ookd_rx_burst_baseband_host(None, 0, fmt, None, 0) == -1 and "NULL" in ok.last_error()


def test_header_is_c99_and_the_layouts_match(tmp_path):
    src = tmp_path / "b.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ookiedokie_amd.h"\n'
                   'int main(void) {\n'
                   '  uint64_t total = 9;\n'
                   '  if (ookd_rx_get_baseband_info(NULL, 0, NULL) != OOKD_ERR_ARG\n'
                   '      || ookd_rx_get_baseband_bursts(NULL, 0, NULL, 0, NULL) != OOKD_ERR_ARG\n'
                   '      || ookd_rx_burst_baseband_device(NULL, 0, OOKD_BASEBAND_CF32, NULL, 0) != OOKD_ERR_ARG\n'
                   '      || ookd_rx_burst_baseband_host(NULL, 0, OOKD_BASEBAND_SC16Q11, NULL, 0) != OOKD_ERR_ARG\n'
                   '      || ookd_rx_baseband_kernel_ms(NULL) != 0.0f\n'
                   '      || ookd_baseband_of(NULL, 0, NULL, 0, OOKD_BASEBAND_CF32, NULL, 0) != OOKD_OK\n'
                   '      || ookd_baseband_bursts(NULL, 0, 4, NULL, 0, &total) != OOKD_OK || total) return 1;\n'
                   '  printf("%d %d %d %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu", OOKD_API_VERSION, OOKD_BASEBAND_CF32,\n'
                   '    OOKD_BASEBAND_SC16Q11, sizeof(ookd_baseband_burst), offsetof(ookd_baseband_burst, first_output),\n'
                   '    offsetof(ookd_baseband_burst, num_outputs), offsetof(ookd_baseband_burst, offset),\n'
                   '    sizeof(ookd_baseband_info), offsetof(ookd_baseband_info, num_bursts),\n'
                   '    offsetof(ookd_baseband_info, total_outputs), offsetof(ookd_baseband_info, tiles_total),\n'
                   '    offsetof(ookd_baseband_info, tiles_filtered), offsetof(ookd_baseband_info, tile_outputs),\n'
                   '    offsetof(ookd_baseband_info, decimation), offsetof(ookd_baseband_info, nu),\n'
                   '    offsetof(ookd_baseband_info, turn));\n'
                   '  return 0; }\n')
    exe = tmp_path / "b"
    libdir = os.path.dirname(ok.LIB_PATH)
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", INCLUDE, str(src), "-o", str(exe),
                        "-L", libdir, "-lookiedokie_amd", "-Wl,-rpath," + libdir], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    got = [int(x) for x in out.stdout.split()]
    B, I = ok.BasebandBurst, ok.BasebandInfo
    assert got == [1, 0, 1, C.sizeof(B), B.first_output.offset, B.num_outputs.offset, B.offset.offset, C.sizeof(I),
                   I.num_bursts.offset, I.total_outputs.offset, I.tiles_total.offset, I.tiles_filtered.offset,
                   I.tile_outputs.offset, I.decimation.offset, I.nu.offset, I.turn.offset]
    assert C.sizeof(B) == 24 and C.sizeof(I) == 56


def test_c_example_still_compiles_and_names_the_option(tmp_path):
    from tests.test_host import _build_c_example
    exe = _build_c_example(tmp_path)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "usage" in r.stderr.lower() and "[--baseband <file" in r.stderr
    # an extension that names no format is refused before anything is opened
    r = subprocess.run([exe, "--baseband", str(tmp_path / "cut.bin"), "nothing.sc16q11", "nothing.json", "none", str(RATE)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and ".cf32" in r.stderr and ".sc16q11" in r.stderr


# ---- the table rule ---------------------------------------------------------------------------------------

def _check_case(case):
    name, e, n_out, D, n, pre, post, max_gap = case
    bursts = bursts_of(e, n_out, D, n, pre, post, max_gap)
    want = baseband_table_of(bursts, n_out, D, n)
    got = ok.baseband_bursts(table_of(bursts), D)
    assert_table(got, want, (name, e))
    assert_table(ok.baseband_bursts(ok.find_bursts(e, n_out, D, n, pre, post, max_gap), D), want, (name, e))
    # what the header says of the table, and what the kernel's search relies on
    m = min(n_out, -(-n // D))
    for raw, b in zip(bursts, want):
        assert b["first_output"] + b["num_outputs"] <= m
        if b["num_outputs"]:
            assert b["offset"] == -(-raw["offset"] // D), (name, raw, b)
        else:
            assert b["first_output"] == -(-n // D) and raw["num_samples"] == 0, (name, raw, b)
        assert (raw["num_samples"] == 0) == (b["num_outputs"] == 0)
    for a, b in zip(want, want[1:]):
        assert a["first_output"] + a["num_outputs"] <= b["first_output"]
    return bursts, want


# (the burst rule's designed lists, and what they lack: a capture whose length is no multiple of D)
DESIGNED = designed_cases() + [
    ("n no multiple of D: the last output has one input", [40, 50, 900, 960], 1000, 4, 3701, 3, 20, 30),
    ("n no multiple of D, a burst in the padding", [40, 50, 950, 960], 1000, 4, 3703, 3, 4, 10),
    ("one output between two bursts", [10, 20, 28, 30], 1000, 3, 3000, 3, 4, 7),
]


@pytest.mark.parametrize("case", DESIGNED, ids=[c[0] for c in DESIGNED])
def test_designed_tables(case):
    bursts, want = _check_case(case)
    name = case[0]
    if name == "E=0":
        assert want == []
    if name == "n_out D > n: clipped at n":
        assert want[-1]["first_output"] + want[-1]["num_outputs"] == case[4] // case[3] < bursts[-1]["hi"]
    if name.startswith("n no multiple of D: the last output"):
        assert want[-1]["first_output"] + want[-1]["num_outputs"] == 926 == case[4] // case[3] + 1
    if name == "n no multiple of D, a burst in the padding":
        assert [b["num_outputs"] for b in want] == [17, 0] and want[1]["first_output"] == 926
    if name == "a burst wholly in the padding":
        assert [b["num_outputs"] for b in want] == [7 + 10, 0] and want[1]["offset"] == 17
    if name == "two bursts in the padding":
        assert [b["num_outputs"] for b in want[1:]] == [0, 0]
    if name == "one output between two bursts":                 # the nearest the rule lets two bursts come
        assert want[0]["first_output"] + want[0]["num_outputs"] + 1 == want[1]["first_output"]


def test_random_tables():
    rng = np.random.default_rng(20260)
    seen = set()
    for _ in range(2000):
        case = random_case(rng)
        bursts, want = _check_case(case)
        D, n = case[3], case[4]
        if n % D:
            seen.add("n not a multiple of D")
        if any(b["num_samples"] == 0 for b in bursts):
            seen.add("a burst in the padding")
        if any(b["num_samples"] and b["first_sample"] + b["num_samples"] == n < b["hi"] * D for b in bursts):
            seen.add("clipped at n")
        if any(a["first_output"] + a["num_outputs"] + 1 == b["first_output"] and b["num_outputs"] for a, b in zip(want, want[1:])):
            seen.add("one output apart")
    assert seen == {"n not a multiple of D", "a burst in the padding", "clipped at n", "one output apart"}


def test_table_capacity_convention():
    t = np.array([[8, 8, 0, 0, 1], [40, 9, 8, 1, 1], [100, 3, 17, 2, 2]], dtype=np.uint64)
    out = np.full((2, 3), 77, dtype=np.uint64)
    total = C.c_uint64(0)
    f = ok.lib().ookd_baseband_bursts
    assert f(t.ctypes.data, 3, 4, out.ctypes.data, 1, C.byref(total)) == 0
    assert total.value == 2 + 3 + 1 and out[0].tolist() == [2, 2, 0] and out[1].tolist() == [77] * 3
    assert f(t.ctypes.data, 3, 4, None, 3, C.byref(total)) == 0 and total.value == 6
    assert f(t.ctypes.data, 3, 4, None, 0, None) == 0
    assert f(t.ctypes.data, 3, 0, None, 0, None) == -1 and "decimation" in ok.last_error()
    assert f(None, 3, 4, None, 0, None) == -1 and "NULL" in ok.last_error()
    assert f(None, 0, 4, None, 0, C.byref(total)) == 0 and total.value == 0


# ---- the cut, given y -------------------------------------------------------------------------------------

def _special_y(rng, n_out):
    y = rng.normal(0.0, 0.4, size=(n_out, 2)).astype(np.float32)
    lsb = 1.0 / 2048.0
    special = [0.0, -0.0, 16.0, -16.0, 15.99951171875, -15.99951171875, 16.0 - lsb / 2, 17.0, -17.0, 1e30, -1e30,
               np.nan, np.inf, -np.inf, np.float32(1e-45), 3.0e-5]
    special += [(k + 0.5) * lsb for k in (-32769, -32768, -3, -2, -1, 0, 1, 2, 3, 100, 101, 32766, 32767)]
    at = rng.choice(n_out, size=2 * len(special), replace=False)
    for i, v in enumerate(special):
        y[at[2 * i], 0] = v
        y[at[2 * i + 1], 1] = v
    return y, at


def test_q16_is_what_the_contract_says():
    lsb = 1.0 / 2048.0
    v = np.array([0.0, -0.0, 0.5 * lsb, 1.5 * lsb, 2.5 * lsb, -0.5 * lsb, -1.5 * lsb, 16.0, -16.0, -17.0, 15.9999, np.nan, np.inf,
                  -np.inf, 1.0], dtype=np.float32)
    assert q16(v).tolist() == [0, 0, 0, 2, 2, 0, -2, 32767, -32768, -32768, 32767, 0, 32767, -32768, 2048]


@pytest.mark.parametrize("fmt", ["cf32", "sc16q11"])
def test_baseband_of_agrees_with_the_restatement(fmt):
    rng = np.random.default_rng(31)
    n_out = 5000
    y, at = _special_y(rng, n_out)
    # every output in one burst; then bursts that touch, an empty one in the middle of the list's tail, the last to n_out
    tables = [[dict(first_output=0, num_outputs=n_out, offset=0)]]
    t, pos, off = [], 3, 0
    for k in range(60):
        length = int(rng.integers(1, 150))
        if pos + length > n_out:
            break
        t.append(dict(first_output=pos, num_outputs=length, offset=off))
        off += length
        pos += length + (0 if k % 5 == 0 else int(rng.integers(1, 40)))
    t.append(dict(first_output=n_out - 7, num_outputs=7, offset=off))
    t.append(dict(first_output=n_out, num_outputs=0, offset=off + 7))
    tables.append(t)
    for table in tables:
        want = baseband_cut_of(y, table, fmt)
        got = ok.baseband_of(y, rows_of(table), fmt)
        same_bits(got, want, fmt)
        assert got.shape[0] == total_of(table)
        got = ok.baseband_of(y.view(np.complex64).reshape(-1), {k: np.array([b[k] for b in table], np.uint64) for k in FIELDS}, fmt)
        same_bits(got, want, fmt)
    whole = ok.baseband_of(y, rows_of(tables[0]), fmt)
    if fmt == "cf32":
        assert whole.view(np.uint32).tolist() == y.view(np.uint32).reshape(-1).tolist()      # -0, NaN and inf keep their bits
    else:
        assert whole[at[::2], 0].tolist() == q16(y[at[::2], 0]).tolist()
        assert {-32768, 32767, 0, 2, -2} <= set(whole.reshape(-1).tolist())


def test_baseband_of_refusals():
    y = np.zeros((100, 2), dtype=np.float32)
    out = np.full((100, 2), 7, dtype=np.int16)
    f = ok.lib().ookd_baseband_of
    t = np.array([[10, 20, 0], [40, 60, 20]], dtype=np.uint64)
    assert f(y.ctypes.data, 100, t.ctypes.data, 2, 1, out.ctypes.data, 80) == 0 and not out[:80].any() and (out[80:] == 7).all()
    out[:] = 7
    assert f(y.ctypes.data, 100, t.ctypes.data, 2, 2, out.ctypes.data, 80) == -1 and "format" in ok.last_error()
    assert f(y.ctypes.data, 100, t.ctypes.data, 2, 1, out.ctypes.data, 79) == -5 and (out == 7).all()
    t[1, 1] = 61
    assert f(y.ctypes.data, 100, t.ctypes.data, 2, 1, out.ctypes.data, 100) == -1 and "beyond n_out" in ok.last_error()
    t[1] = [101, 0, 20]
    assert f(y.ctypes.data, 100, t.ctypes.data, 2, 0, out.ctypes.data, 100) == -1 and "beyond n_out" in ok.last_error()
    t[1] = [2 ** 64 - 1, 2, 20]                                 # (first + count wraps)
    assert f(y.ctypes.data, 100, t.ctypes.data, 2, 0, out.ctypes.data, 100) == -1
    t[1] = [100, 0, 20]                                         # an empty burst at n_out is inside
    assert f(y.ctypes.data, 100, t.ctypes.data, 2, 0, out.ctypes.data, 100) == 0
    out[:] = 7
    assert f(None, 100, t.ctypes.data, 2, 0, out.ctypes.data, 100) == -1 and "NULL" in ok.last_error()
    assert f(y.ctypes.data, 100, None, 2, 0, out.ctypes.data, 100) == -1 and "NULL" in ok.last_error()
    assert f(y.ctypes.data, 100, t.ctypes.data, 2, 0, None, 100) == -1 and "NULL" in ok.last_error()
    assert (out == 7).all()
    with pytest.raises(KeyError):
        ok.baseband_of(y, t, "cs8")


def test_tiles_and_turn_of_the_restatement():
    t = [dict(first_output=1000, num_outputs=48, offset=0), dict(first_output=4096, num_outputs=1, offset=48),
         dict(first_output=9000, num_outputs=0, offset=49)]
    assert tiles_filtered_of(t, 9000, 1024) == 3 and tiles_filtered_of(t, 9000, 8) == 6 + 1
    assert turn_of(0.2, 4) == pytest.approx(-0.2) and turn_of(0.0, 4) == 0.0 and turn_of(0.2, 1) == pytest.approx(0.2)


# ---- the round trip through the reference decoder --------------------------------------------------------

def _round_trip(oracle, iq, device, filt, what):
    n = iq.size // 2
    fir = oracle.load_filter_json(golden_path("filters", filt))
    D = fir.total_decimation
    fsm, _ = oracle.load_device_json(golden_path("devices", device), RATE // D)
    whole = oracle.rx(iq, fir, THR, fsm, SPB, want_bits=True, want_fir=True)
    e, n_out = edges_of(whole.bits).astype(np.uint64), whole.decimated
    pre, post, max_gap = margins(D)
    bursts = bursts_of(e, n_out, D, n, pre, post, max_gap)
    table = baseband_table_of(bursts, n_out, D, n)
    assert_table(ok.baseband_bursts(ok.find_bursts(e, n_out, D, n, pre, post, max_gap), D), table, what)
    cut = baseband_cut_of(whole.fir, table, "sc16q11")
    same_bits(ok.baseband_of(whole.fir, rows_of(table), "sc16q11"), cut, "sc16q11", what)
    assert np.abs(whole.fir).max() < 16.0                        # nothing was clamped
    again = oracle.rx(cut.reshape(-1), None, THR, fsm, SPB, want_bits=True)
    total = total_of(table)
    bits = np.concatenate([whole.bits[b["first_output"]:b["first_output"] + b["num_outputs"]] for b in table])
    assert bits.size == total and int(np.count_nonzero(again.bits[:total] != bits)) == 0, what
    assert not again.bits[total:].any(), what                   # (the padding of the cut to whole buffers)
    assert again.payloads.tolist() == whole.payloads.tolist(), what
    assert again.err_samples.size == whole.err_samples.size, what
    mapped, which = mapped_samples(whole.msg_samples, bursts, D)
    assert again.msg_samples.tolist() == mapped, (what, which, whole.msg_samples.tolist())
    return whole, bursts, table, n_out


@pytest.mark.parametrize("noise", [None, 1], ids=["clean", "noise"])
@pytest.mark.parametrize("filt", FILTERS)
@pytest.mark.parametrize("name", ["G1", "G2"])
def test_quantised_cut_decodes_like_the_whole_capture(oracle, vectors, name, filt, noise):
    iq = golden_iq(vectors, name, noise_seed=noise)
    whole, bursts, table, n_out = _round_trip(oracle, iq, vectors[name]["device"], filt, (name, filt, noise))
    assert len(whole.msg_samples) >= 2 and 1 <= len(table) and 0 < total_of(table) < n_out


@pytest.mark.parametrize("filt", FILTERS)
def test_silence_then_two_levels(oracle, vectors, filt):
    """silence, G1, silence, G1 at a quarter of its level: two transmissions, and most of the capture left out"""
    g = golden_iq(vectors, "G1", noise_seed=3)
    quiet = np.random.default_rng(4).integers(-40, 41, size=2 * g.size).astype(np.int16)
    iq = np.concatenate([quiet, g, quiet, (g.astype(np.int32) // 4).astype(np.int16)])
    whole, bursts, table, n_out = _round_trip(oracle, iq, vectors["G1"]["device"], filt, filt)
    assert len(table) >= 2 and 0 < 2 * total_of(table) < n_out
    half = 3 * g.size // 2 // whole_decimation(oracle, filt)     # outputs in front of the second silence
    first = int(np.count_nonzero(whole.msg_samples < half))
    assert first >= 2 and len(whole.msg_samples) == 2 * first    # the quiet transmitter decodes like the loud one


def whole_decimation(oracle, filt):
    return oracle.load_filter_json(golden_path("filters", filt)).total_decimation
