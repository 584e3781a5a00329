"""The pulse moments' contract (include/ookiedokie_amd.h, "Pulse moments") restated in numpy, independent of the
library: the filter's complex output + edge list -> three int64 sums per on-run, and mean power, carrier and coherence
per message.  y comes from oracle.unpack / oracle.fir_run (untuned) or tests.tuned_contract.contract_rx's floats
(tuned), both over the capture zero padded to whole buffers.  Shared by tests/test_run_moments_host.py and
tests/test_gpu_run_moments.py."""
import math

import numpy as np

from tests.run_levels_contract import RATE, SPB, THR, padded, runs_of

LIMIT = np.float32(2.0 ** 32)
ONE = 2.0 ** 30


def q(v):
    """llrint((double)v 2^30), ties to even, v clamped to [-2^32, 2^32] first, a NaN -> 0; int64"""
    v = np.atleast_1d(np.asarray(v, dtype=np.float32)).copy()
    v[np.isnan(v)] = np.float32(0.0)
    v = np.clip(v, -LIMIT, LIMIT)
    return np.rint(v.astype(np.float64) * ONE).astype(np.int64)


def wrapped_sum(terms):
    """the sum of int64 terms modulo 2^64, as int64"""
    total = 0
    for t in np.asarray(terms, dtype=np.int64).tolist():
        total += t
    total &= (1 << 64) - 1
    return total - (1 << 64) if total >= 1 << 63 else total


def oracle_y(oracle, fir, iq):
    """the oracle's filter output (the unpacked samples when fir is None), float32 [n_out, 2]"""
    y = oracle.unpack(iq)
    if fir is not None:
        y = oracle.fir_run(fir, y)
    return np.ascontiguousarray(y, dtype=np.float32).reshape(-1, 2)


def terms_of(y):
    """per output: q(p_j), q(zr_j), q(zi_j) -- the lag terms of output 0 are 0 and never summed"""
    y = np.ascontiguousarray(y, dtype=np.float32).reshape(-1, 2)
    re, im = y[:, 0], y[:, 1]
    with np.errstate(over="ignore", invalid="ignore"):
        rr = re * re
        ii = im * im
        p = rr + ii
        zr = np.zeros_like(re)
        zi = np.zeros_like(re)
        a = re[1:] * re[:-1]
        b = im[1:] * im[:-1]
        c = im[1:] * re[:-1]
        d = re[1:] * im[:-1]
        zr[1:] = a + b
        zi[1:] = c - d
    assert p.dtype == zr.dtype == zi.dtype == np.float32
    return q(p), q(zr), q(zi)


def moments_of(y, edges, n_out):
    """-> int64 [R, 3]: power, lag_re, lag_im of every on-run"""
    y = np.ascontiguousarray(y, dtype=np.float32).reshape(-1, 2)
    assert y.shape[0] == n_out, (y.shape, n_out)
    qp, qr, qi = terms_of(y)
    runs = runs_of(edges, n_out)
    out = np.zeros((len(runs), 3), dtype=np.int64)
    for r, (a, f) in enumerate(runs):
        out[r] = (wrapped_sum(qp[a:f]), wrapped_sum(qr[a + 1:f]), wrapped_sum(qi[a + 1:f]))
    return out


def message_carriers_of(edges, moments, msg_samples, pulses, decimation, nu, n_out):
    """message m: the on-runs rising at or below msg_samples[m] and above msg_samples[m - 1], the last `pulses` of
    them; -> [(carrier, mean_power, coherence, outputs)]"""
    runs = runs_of(edges, n_out)
    if isinstance(moments, dict):
        moments = np.stack([moments[k] for k in ("power", "lag_re", "lag_im")], axis=1)
    mo = np.asarray(moments, dtype=np.int64).reshape(-1, 3)
    assert mo.shape[0] == len(runs)
    out, prev = [], -1
    for s in (int(x) for x in msg_samples):
        mine = [r for r, (a, _) in enumerate(runs) if prev < a <= s][-pulses:]
        P = Zr = Zi = 0.0
        outputs = 0
        for r in mine:
            P += float(mo[r, 0])
            Zr += float(mo[r, 1])
            Zi += float(mo[r, 2])
            outputs += runs[r][1] - runs[r][0]
        carrier, coherence = float(nu), 0.0
        if Zr != 0.0 or Zi != 0.0:
            x = math.atan2(Zi, Zr) / (2.0 * math.pi) - nu * decimation
            carrier = nu + (x - math.floor(x + 0.5)) / decimation
            coherence = math.hypot(Zr, Zi) / P if P != 0.0 else 0.0
        out.append((carrier, P / ONE / outputs if outputs else 0.0, coherence, outputs))
        prev = s
    return out


# ---- T3: two transmitters 6 kHz apart, one at a quarter of the other's level ----------------------------------------

TWO_NU = (600e3 / RATE, 606e3 / RATE)       # the transmitters
TWO_TUNE = 603e3 / RATE                     # the context between them
TWO_DC = 300 + 200j
TWO_NOISE = 40


def two_carrier_capture(vectors):
    """golden G1 moved to +600 kHz at nominal level, then G1 moved to +606 kHz at 1/4 level, both with the DC term and
    +-40 LSB of noise (seeds 1 and 2) -> (golden entry, capture, samples of the first half)"""
    from tests.helpers import iq_from_rle
    from tests.tuned_contract import moved
    g = vectors["G1"]
    iq = iq_from_rle(g["i_rle"], g["num_samples"])
    a = moved(iq, TWO_NU[0], TWO_DC, TWO_NOISE, seed=1, scale=1.0)
    # the second transmitter's phase goes on counting from its own first sample: a carrier does not know the capture
    b = moved(iq, TWO_NU[1], TWO_DC, TWO_NOISE, seed=2, scale=0.25)
    return g, np.concatenate([a, b]), a.size // 2


# ---- the seam captures behind a filter, built on the reference ------------------------------------------------------

SLOW_NU = 1.0 / 9973.0              # a turn in 9973 input samples: inside every filter's pass band here
_moved = {}


def moved_seam(oracle, shape, which):
    """FILTERED_TARGETS[which] of tests/run_level_seams_inputs.py behind `shape`, shifted onto the seams by
    filtered_capture, the pulses turning at SLOW_NU so that both lag sums hold something -> (capture, samples, samples
    per buffer, targets)"""
    from tests import run_level_seams_inputs as S
    from tests.run_levels_contract import oracle_fir, ref_edges
    from tests.tuned_contract import moved
    if (shape, which) not in _moved:
        D = S.SHAPE_D[shape]
        n, spb = S.FILTERED_OUT * D, 500 * D
        fir = oracle_fir(oracle, shape)
        iq = S.filtered_capture(lambda x: ref_edges(oracle, fir, x, spb), n, D, S.FILTERED_PULSE, S.FILTERED_TARGETS[which],
                                move=lambda x: moved(x, SLOW_NU))
        _moved[shape, which] = (iq, n, spb, S.FILTERED_TARGETS[which])
    return _moved[shape, which]
