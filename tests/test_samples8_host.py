"""CPU-side tests of the 8-bit sample formats (CS8, CU8): the public constants and symbols, the widening rule
against the oracle's unpack, and the 8-bit fixtures the GPU tests decode (tests/test_gpu_samples8.py imports the
fixture builders below)."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

from tests.helpers import GOLDEN, golden_path, iq_from_rle

import ookiedokie_amd as ok
from ookiedokie_amd import build as okbuild

RATE = 3000000
FORMATS = ("cs8", "cu8")


# ---- 8-bit fixtures ---------------------------------------------------------------------------------------

def cut8(iq16):
    """an SC16Q11 capture cut to 8 bits (arithmetic shift: floor), as int8 values"""
    return (np.asarray(iq16, dtype=np.int16) >> 4).astype(np.int8)


def as_format(v8, fmt):
    """int8 values -> the array a context of that format takes (cs8: int8; cu8: uint8 around 128)"""
    v8 = np.asarray(v8, dtype=np.int8)
    return v8 if fmt == "cs8" else (v8.astype(np.int16) + 128).astype(np.uint8)


def widen(x, fmt):
    """the SC16Q11 capture an 8-bit capture stands for: CS8 v -> 16 v, CU8 u -> 16 (u - 128)"""
    x = np.asarray(x)
    assert x.dtype == (np.int8 if fmt == "cs8" else np.uint8)
    v = x.astype(np.int16) - (0 if fmt == "cs8" else 128)
    return (v * 16).astype(np.int16)


def golden8(vectors, name, noise_seed=None):
    """golden capture G1 / G2 cut to 8 bits, clean or with +-60 LSB of uniform noise added before the cut"""
    g = vectors[name]
    iq = iq_from_rle(g["i_rle"], g["num_samples"])
    if noise_seed is not None:
        rng = np.random.default_rng(noise_seed)
        iq = (iq + rng.integers(-60, 61, size=iq.size)).astype(np.int16)
    return g, cut8(iq)


@pytest.fixture(scope="session", autouse=True)
def built_lib():
    okbuild.build()
    return ok.lib()


# ---- interface --------------------------------------------------------------------------------------------

def test_constants_match_header_and_layouts_are_unchanged(tmp_path):
    src = tmp_path / "c8.c"
    src.write_text('#include <stdio.h>\n#include "ookiedokie_amd.h"\n'
                   'int main(void) { printf("%u %u %d %d %d %d %zu %zu %zu", (unsigned)OOKD_RX_SAMPLES_CS8,\n'
                   '  (unsigned)OOKD_RX_SAMPLES_CU8, OOKD_FRONT_NO_FILTER_8, OOKD_FRONT_FIR1_MFMA_8, OOKD_FRONT_FIR2_MFMA_8,\n'
                   '  OOKD_API_VERSION, sizeof(ookd_rx_config), sizeof(ookd_rx_stats), sizeof(ookd_front_info));\n'
                   '  return 0; }\n')
    exe = tmp_path / "c8"
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.dirname(ok.HEADER_PATH), str(src), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True).stdout.split()]
    assert got[:5] == [ok.RX_SAMPLES_CS8, ok.RX_SAMPLES_CU8, ok.FRONT_NO_FILTER_8, ok.FRONT_FIR1_MFMA_8,
                       ok.FRONT_FIR2_MFMA_8] == [1 << 10, 1 << 11, 9, 10, 11]
    assert got[5] == 1 == ok.lib().ookd_api_version()
    # what they were before the formats: no member added
    assert got[6:] == [C.sizeof(ok.RxConfig), C.sizeof(ok.RxStats), C.sizeof(ok.FrontInfo)] == [80, 104, 56]
    assert ok.RX_SCAN_TABLES < ok.RX_SAMPLES_CS8 < ok.RX_SAMPLES_CU8
    assert ok.FRONT_FIR2_MFMA == 8


def test_new_symbols_are_exported(built_lib):
    assert hasattr(built_lib, "ookd_rx_sample_bytes")
    assert hasattr(built_lib, "sdr_hip_file_sample_flags")
    assert built_lib.ookd_rx_sample_bytes(None) == 0
    assert built_lib.sdr_hip_file_sample_flags(None) == 0
    assert set(ok.SAMPLE_FORMATS) == {"sc16q11", "cs8", "cu8"}
    with pytest.raises(ValueError):
        ok.Receiver(None, None, max_samples=16, sample_format="cf32")


# ---- the widening rule ------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", FORMATS)
def test_widening_rule_is_the_oracles_unpack(oracle, fmt):
    """all 256 values of the format: unpack(widened int16) == v / 128 as float32, bit for bit"""
    if fmt == "cs8":
        x = np.arange(-128, 128, dtype=np.int16).astype(np.int8)
        v = x.astype(np.float32)
    else:
        x = np.arange(0, 256, dtype=np.int16).astype(np.uint8)
        v = x.astype(np.float32) - np.float32(128.0)
    pairs = np.stack([x, x[::-1]], axis=1).reshape(-1)          # every value on both rails
    w = widen(pairs, fmt)
    assert w.min() == -2048 and w.max() == 2032                 # every 8-bit sample is a nominal SC16Q11 one
    got = oracle.unpack(w)
    want = np.stack([v, v[::-1]], axis=1) / np.float32(128.0)
    assert got.dtype == np.float32 and (got.view(np.uint32) == want.astype(np.float32).view(np.uint32)).all()
    assert (as_format(x.astype(np.int16) - (0 if fmt == "cs8" else 128), fmt) == x).all()


# ---- the fixtures decode ----------------------------------------------------------------------------------

@pytest.mark.parametrize("noise_seed", [None, 7])
@pytest.mark.parametrize("name,nmsg,nbits", [("G1", 3, 36), ("G2", 2, 32)])
def test_8bit_golden_captures_decode_on_the_oracle(oracle, vectors, name, nmsg, nbits, noise_seed):
    g, v8 = golden8(vectors, name, noise_seed)
    for fmt in FORMATS:
        iq = widen(as_format(v8, fmt), fmt)
        assert (iq == v8.astype(np.int16) * 16).all()
        of = oracle.load_filter_json(golden_path("filters", g["filter"]))
        od, _ = oracle.load_device_json(golden_path("devices", g["device"]), RATE)
        want = oracle.rx(iq, of, 0.1, od, g["spb"])
        assert len(want.msg_samples) == nmsg
        assert all(want.payload_bits(i, nbits) == g["survey"]["payload_bits"] for i in range(nmsg))
        if noise_seed is None:
            assert list(want.msg_samples) == g["survey"]["msg_samples"]
