"""What the tests of the fused tuned two-stage front end (OOKD_FRONT_TUNED_FIR2; test_tuned_fir2_host.py,
test_gpu_tuned_fir2.py) share, numpy only: the tile geometry of fir2_tuned_kernel, the documented quiet rule for two
stages and its weights as the plan folds them.  Expected bits and floats come from
tests/tuned_contract.py; nothing here knows what the kernel computes."""
import math
import zlib

import numpy as np

from tests.tuned_contract import golden_capture, moved

F, T1, T2 = 256, 16, 32                         # final outputs per tile, padded tap counts of the two stages
L1 = 64 * ((2 * (F - 1) + T2 + 63) // 64)       # level-1 outputs a tile computes
L0 = 2 * (L1 - 1) + T1                          # input samples of a tile's window: 1166
A0 = 2 * (1 - (T2 - 1)) + 1 - (T1 - 1)          # first window sample of tile 0: -74
DC = 400.0 * (1 + 0.5j)
NOISE = 40
NUS = [0.2, -0.3, 1.0 / 3000.0, 0.5]
NU_IDS = ["p0.2", "m0.3", "1_3000", "0.5"]
U = 2.0 ** -24
SQRT2 = 1.41421356237309515


def moved_golden(cap, nu):
    """golden capture `cap` moved to nu with DC and noise (the parity inputs of test_gpu_tuned.py) -> base, moved, g"""
    base, g = golden_capture(cap)
    return base, moved(base, nu, DC, NOISE, seed=zlib.crc32(("%s/%g" % (cap, nu)).encode())), g


def rule_terms(stages):
    """A = A1 A2, G = |C1| |C2| + 1e-12 S, e = 1.01 (2 T1 + 1 + 2 T2 + 1) u S, S = prod max(sum(|re| + |im|), 1) over
    the float32 taps [(decimation, re, im)], summed in double tap by tap"""
    A = G = S = 1.0
    T = 0.0
    for _, re, im in stages:
        a = s = gr = gi = 0.0
        for r, i in zip(np.asarray(re, np.float32), np.asarray(im, np.float32)):
            r, i = float(r), float(i)
            a += math.hypot(r, i)
            s += abs(r) + abs(i)
            gr += r
            gi += i
        A *= a
        G *= math.hypot(gr, gi)
        S *= max(s, 1.0)
        T += 2.0 * len(re) + 1.0
    return A, G + 1e-12 * S, 1.01 * T * U * S


def quiet_weights(stages, thr):
    """(quiet_a, quiet_b) as float32: the rule folded as the plan folds it, rounded upwards"""
    A, G, e = rule_terms(stages)
    scale = SQRT2 / (2.0 * 2048.0) / (0.999 * float(np.float32(thr)))
    up = lambda v: np.nextafter(np.float32(v), np.float32(np.inf))
    return up((A + e) * scale), up((G + e) * scale)


def interior_tiles(n):
    """first final outputs of the tiles whose whole input window holds capture samples"""
    return [J0 for J0 in range(0, -(-n // 4), F) if 4 * J0 + A0 >= 0 and 4 * J0 + A0 + L0 <= n]


def window_ab(iq, J0):
    """a = the larger component range, b = the larger |min + max| of tile J0's input window, raw LSB"""
    w = np.asarray(iq).reshape(-1, 2)[4 * J0 + A0:4 * J0 + A0 + L0].astype(np.int64)
    mx, mn = w.max(axis=0), w.min(axis=0)
    return int((mx - mn).max()), int(np.abs(mx + mn).max())


def documented_lhs(stages, a, b):
    A, G, e = rule_terms(stages)
    return SQRT2 / (2.0 * 2048.0) * ((A + e) * a + (G + e) * b)


def kernel_takes(a, b, qa, qb):
    """the test as the kernel evaluates it: float32, two products and one sum, each rounded"""
    return bool(np.float32(a) * np.float32(qa) + np.float32(b) * np.float32(qb) < np.float32(1.0))


def quiet_census(iq, stages, thr, bits):
    """-> interior tiles, tiles the documented rule takes, tiles whose contract bits are all zero, tiles the rule takes
    that hold a one, tiles the float32 form of the test takes, tiles whose left-hand side is below thr / 2"""
    n = np.asarray(iq).size // 2
    qa, qb = quiet_weights(stages, thr)
    tiles = interior_tiles(n)
    taken = zero = bad = taken32 = half = 0
    for J0 in tiles:
        a, b = window_ab(iq, J0)
        lhs = documented_lhs(stages, a, b)
        z = not bits[J0:J0 + F].any()
        zero += z
        t = lhs < 0.999 * float(np.float32(thr))
        taken += t
        bad += t and not z
        taken32 += kernel_takes(a, b, qa, qb)
        half += lhs < 0.5 * float(np.float32(thr))
    return dict(interior=len(tiles), taken=int(taken), zero=int(zero), bad=int(bad), taken32=int(taken32), half=int(half))
