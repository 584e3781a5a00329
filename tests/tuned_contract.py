"""The tuned front end's contract (include/ookiedokie_amd.h, at ookd_filter_tuned_taps) restated in numpy, and the
captures the tuned tests decode.  Shared by test_tuned_host.py and test_gpu_tuned.py; float32 throughout, every
product and every sum rounded on its own."""
import json
import os

import numpy as np

from tests.helpers import GOLDEN, iq_from_rle

RATE, SPB, THR = 3000000, 8192, 0.1


def taps_rule(h, nu, before):
    """the header's tap rule in double: h float32 taps of a stage, `before` = product of the decimations in front"""
    k = np.arange(h.size, dtype=np.float64)
    t = abs(nu) * (before * k)
    r = t - np.rint(t)
    s = np.sin(2.0 * np.pi * r)
    if nu < 0:
        s = -s
    return h.astype(np.float64) * np.cos(2.0 * np.pi * r), h.astype(np.float64) * s


def contract_stage(xr, xi, re, im, D):
    """one stage from zero history: output j sits on input D (j + 1) - 1, tap 0 multiplies the newest sample; the
    four statements of the contract per tap, in order"""
    T = re.size
    n_out = xr.size // D
    pr = np.concatenate([np.zeros(T - 1, np.float32), xr])
    pi = np.concatenate([np.zeros(T - 1, np.float32), xi])
    newest = D * (np.arange(n_out) + 1) - 1 + (T - 1)
    ar = np.zeros(n_out, np.float32)
    ai = np.zeros(n_out, np.float32)
    for k in range(T):
        a, b = pr[newest - k], pi[newest - k]
        ar = ar + re[k] * a
        ar = ar - im[k] * b
        ai = ai + re[k] * b
        ai = ai + im[k] * a
    assert ar.dtype == np.float32 and ai.dtype == np.float32
    return ar, ai


def contract_rx(iq, stages, thr, spb=SPB):
    """stages: [(decimation, re, im)] float32 taps.  -> (bits uint8, floats [n, 2] float32) of the capture zero
    padded to whole buffers, as an rx context runs it"""
    iq = np.asarray(iq, dtype=np.int16).reshape(-1)
    n = iq.size // 2
    n_in = -(-n // spb) * spb
    xr = np.zeros(n_in, np.float32)
    xi = np.zeros(n_in, np.float32)
    xr[:n] = iq[0::2].astype(np.float32) * np.float32(1.0 / 2048.0)
    xi[:n] = iq[1::2].astype(np.float32) * np.float32(1.0 / 2048.0)
    for D, re, im in stages:
        xr, xi = contract_stage(xr, xi, np.asarray(re, np.float32), np.asarray(im, np.float32), int(D))
    p = xr * xr + xi * xi
    with np.errstate(invalid="ignore"):
        bits = (np.sqrt(p) >= np.float32(thr)).astype(np.uint8)        # ookiedokie.c:171-179
    return bits, np.stack([xr, xi], axis=1)


def lib_stages(flt, nu):
    """the library's own taps for a context tuned to nu: [(decimation, re, im)]"""
    return [(flt.stage(s)[0],) + tuple(flt.tuned_taps(nu, s)) for s in range(flt.num_stages)]


def golden_capture(name):
    with open(os.path.join(GOLDEN, "vectors.json")) as f:
        g = json.load(f)[name]
    return iq_from_rle(g["i_rle"], g["num_samples"]), g


def moved(iq, nu, dc=0j, noise=0, seed=0, scale=1.0):
    """z e^{j 2 pi nu n} + dc + uniform noise of +-noise LSB on both rails, rounded and clipped to int16"""
    iq = np.asarray(iq, dtype=np.int16).reshape(-1)
    z = (iq[0::2].astype(np.float64) + 1j * iq[1::2].astype(np.float64)) * scale
    n = np.arange(z.size, dtype=np.float64)
    z = z * np.exp(2j * np.pi * ((nu * n) % 1.0)) + dc
    rng = np.random.default_rng(seed)
    if noise:
        z = z + rng.integers(-noise, noise + 1, size=z.size) + 1j * rng.integers(-noise, noise + 1, size=z.size)
    out = np.empty(2 * z.size, np.int16)
    out[0::2] = np.clip(np.rint(z.real), -32768, 32767)
    out[1::2] = np.clip(np.rint(z.imag), -32768, 32767)
    return out


def to_8bit(iq, fmt):
    """the capture scaled by 1/20 and clipped to the byte range, as `fmt` samples and as the SC16Q11 capture of
    the same values (16 v)"""
    v = np.clip(np.rint(np.asarray(iq, np.float64) / 20.0), -128, 127).astype(np.int16)
    raw = v.astype(np.int8) if fmt == "cs8" else (v + 128).astype(np.uint8)
    return raw, (v * 16).astype(np.int16)
