"""Input builders for the front ends' shape sweeps (test_gpu_front_shapes.py; checked on the CPU by
test_front_shapes_host.py), numpy only: the stage shapes, their taps, the capture every shape decodes and what the
oracle's result must look like before a GPU result is compared with it.  Nothing here knows what the kernels
compute."""
import zlib

import numpy as np

THR = 0.1                       # 204.8 LSB
SPB = 8192
NOISE = 40                      # +-LSB on both components
ON, AT, OFF, WIDE = 300, 205, 150, 20000    # on; at the threshold (the noise toggles it: the band sees it); off but
                                            # above quiet_lsb (145 LSB at unit gain): loud, not quiet; a wide burst
IN_BAND = 64
TILE = 1024                     # final outputs per tile of the generic kernels where the level buffers allow it

# two decimate-by-2 stages, (n1, n2) taps: the corners, odd sizes and one below each limit of the (16, 32) family
FIR2_SHAPES = [(1, 1), (1, 32), (16, 1), (2, 3), (3, 5), (7, 9), (9, 17), (15, 31), (16, 31), (15, 32), (16, 32)]

# (decimation, taps) per stage.  Generic-kernel shapes whose level buffers hold a 1024-output tile ...
GENERIC_SHAPES = {
    "d3t40": [(3, 40)],
    "d2d1d2": [(2, 12), (1, 33), (2, 20)],
    "d5t3": [(5, 3)],                                   # fewer taps than D
    "d7t1": [(7, 1)],                                   # a pure decimation: y[o] = h0 x[7 o + 6]
    "d1t300": [(1, 300)],
    "eight": [(1, k) for k in range(1, 9)],             # kMaxStages
    "d19t64": [(19, 64)],                               # the largest single decimation that still fits 1024
}
# ... and those that need a smaller one
LARGE_SHAPES = {
    "d20t19": [(20, 19)],                               # the first single stage that does not fit
    "d32t64": [(32, 64)],
    "d64t64": [(64, 64)],
    "d4d4t30": [(4, 30), (4, 30)],
    "d2x4": [(2, 8)] * 4,
    "d3d2d5": [(3, 21), (2, 9), (5, 40)],
    # tiles of 128 and 64 outputs, below the 256 lanes of a workgroup: waves that own no bit word.  One stage and two
    # (both level buffers in use) at each
    "d101t8": [(101, 8)],
    "d9d11t8": [(9, 8), (11, 8)],
    "d300t4": [(300, 4)],
    "d15d20": [(15, 6), (20, 5)],
}
# the tile generic_tile gives each shape above (level s of a tile of L outputs: len_s = D_s (len_{s+1} - 1) + T_s, the
# largest power of two L with max even len + max odd len <= 20478) -- test_front_plan_host.py holds the plan to it
TILES = dict({name: 1024 for name in GENERIC_SHAPES}, d20t19=512, d32t64=512, d4d4t30=512, d2x4=512, d64t64=256,
             d3d2d5=256, d101t8=128, d9d11t8=128, d300t4=64, d15d20=64)
# final outputs of a sweep capture: three tiles and 37 where that stays within 250 000 samples, else as many of the
# shape's smaller tiles as do -- never a multiple of the tile
SWEEP_OUTPUTS = {"101x8": 16 * 128 + 37, "9x8_11x8": 16 * 128 + 37, "300x4": 12 * 64 + 37, "15x6_20x5": 12 * 64 + 37}


def fir2_shape(n1, n2):
    return [(2, n1), (2, n2)]


def shape_id(shape):
    return "_".join("%dx%d" % (d, t) for d, t in shape)


def taps(rng, n):
    """|normal| + 0.05, sum 1: a DC gain of 1, so a level decides a bit"""
    h = np.abs(rng.normal(0, 1, n)) + 0.05
    return (h / h.sum()).astype(np.float32)


def stages(shape):
    """[(decimation, float32 taps)] of a shape, the same taps wherever the shape is used"""
    rng = np.random.default_rng(zlib.crc32(shape_id(shape).encode()))
    return [(int(d), taps(rng, int(t))) for d, t in shape]


def total_decimation(shape):
    return int(np.prod([d for d, _ in shape], dtype=np.int64))


def sweep_len(shape):
    """no multiple of a tile or of a buffer, nor of a total decimation that does not divide 3; ends inside a tile"""
    return total_decimation(shape) * SWEEP_OUTPUTS.get(shape_id(shape), 3 * TILE + 37) + 3


def capture_seed(shape):
    """(+ 1: the 300-tap filter smooths the AT stretch of its 3112-sample capture into a handful of toggles; with these
    seeds the oracle's result has at least 16 edges for every shape above -- test_front_shapes_host.py)"""
    return zlib.crc32(shape_id(shape).encode()) + 1


def capture(n, seed=0):
    """noise of +-NOISE LSB on both components; on I, stretches of n/8 samples at ON, AT and OFF and n/16 samples at
    WIDE, noise between them; IN_BAND samples just below the threshold behind the burst"""
    rng = np.random.default_rng(seed)
    i = rng.integers(-NOISE, NOISE + 1, size=n).astype(np.int64)
    q = rng.integers(-NOISE, NOISE + 1, size=n).astype(np.int64)
    for k, (level, length) in enumerate(((ON, n // 8), (AT, n // 8), (OFF, n // 8), (WIDE, n // 16))):
        start = n // 16 + k * (3 * n // 16)
        i[start:start + length] += level
    # Right behind the burst, IN_BAND samples at (204, 18) exactly: |x|^2 = 41940 LSB^2 beside the threshold's 41943.04.
    # A filter of one unit tap per stage hands the slicer the samples themselves, and no integer pair reaches the band
    # of a nominal tile (41942 .. 41944 are no sums of two squares): only this run, in the windows the burst makes
    # wide, puts such a filter's outputs into a band.
    end = n // 16 + 3 * (3 * n // 16) + n // 16
    i[end:end + IN_BAND] = 204
    q[end:end + IN_BAND] = 18
    iq = np.empty(2 * n, np.int16)
    iq[0::2], iq[1::2] = i, q
    return iq


def to_cs8(iq):
    """the capture in units of 16 LSB, rounded and clipped to the byte range -- ON stays on (19), AT stays at the
    threshold (13 = 208 LSB beside 204.8, the noise of +-2.5 toggles it) -- as CS8 samples and as the SC16Q11 capture of
    the same values"""
    v = np.clip(np.rint(np.asarray(iq, np.float64) / 16.0), -128, 127).astype(np.int16)
    return v.astype(np.int8), (v * 16).astype(np.int16)


def two_carrier_capture(shape, nus, scale2=0.5):
    """the shape's capture moved to nus[0], plus another capture of the same kind at half the level moved to nus[1]
    (its ON 150 and AT 102.5 LSB sit around a threshold of 0.05 as the first one's sit around 0.1)"""
    from tests.tuned_contract import moved
    n = sweep_len(shape)
    a = moved(capture(n, seed=capture_seed(shape)), nus[0]).astype(np.int32)
    b = moved(capture(n, seed=capture_seed(shape) + 7), nus[1], scale=scale2).astype(np.int32)
    return np.clip(a + b, -32768, 32767).astype(np.int16)


def check_oracle_result(bits, n, dec):
    """what a case asserts on the oracle's bits alone, before it looks at the GPU's: the ones are between 1/16 and
    15/16 of the floor(n / dec) outputs, and there are at least 16 edges"""
    n_out = n // dec
    ones = int(np.count_nonzero(bits[:n_out]))
    edges = int(np.count_nonzero(np.diff(np.concatenate([[0], bits.astype(np.int8)]))))
    assert n_out // 16 <= ones <= 15 * n_out // 16, (ones, n_out)
    assert edges >= 16, edges
    return ones / max(n_out, 1), edges


def edge_lengths(dec):
    """lengths around the decimation edge and the edge of a 1024-output tile"""
    return [0, 1, dec - 1, dec, dec + 1, TILE * dec - 1, TILE * dec, TILE * dec + 1]
