"""Captures laid against the seams of the pulse moments' kernel (run_moments.hip), for
tests/test_gpu_run_moments.py; what each is laid for is proved on the reference alone by
tests/test_run_moments_host.py.  The layouts and the seam catalogue are those of tests/run_level_seams_inputs.py (W = 64
lanes, P = 256 outputs of one pass of the workgroup, the tile, B = 4096, the 64-tile chunk, the capture's end); the
amplitudes are new.  A sum shows a lost or doubled term only if the terms differ, so without a filter every on sample
has its own I and Q, a hash of its index, each rail at least MIN_RAIL in magnitude: on at THR whatever the signs.

S1 .. S10 of the moments' seams, by the layout that holds them:
  S1  a run across a tile seam (the pair (j0 - 1, j0) counted once)     seams-across
  S2  a run rising exactly at j0 (that pair not counted)                 seams-starts
  S3  a one-output run at j0 - 1 with j0 off; a run falling at j0        seams-singles_before, seams-ends
  S4  a run rising at j0 - 1                                             seams-pair
  S5  output 0 on: an edge at 0 and no extra output                      seams-starts, seams-singles_on (s = 0)
  S6  a run across a 4096 block seam and across a 64-tile chunk seam     seams-across (s = B, 2 B, C)
  S7  a run open through the padding to n_out, n no multiple of a buffer open_pad_capture (behind a filter)
  S8  capture c ends on, capture c + 1 begins on                          parity cases, batched
  S9  one on, one off across a whole wave and a whole tile               dense-even, dense-odd
  S10 a run longer than 64 tiles                                         long_run"""
import numpy as np

from tests import run_level_seams_inputs as S

MIN_RAIL, SPAN = 300, 1700          # |I|, |Q| in 300 .. 1999 LSB: |x| >= 0.207 > THR
MIN_RAIL8, SPAN8 = 16, 105          # CS8 / CU8 values 16 .. 120 (x 16 LSB): |x| >= 0.176


def _hash(j, salt):
    """a 32-bit mix of the index (xorshift-multiply): neighbours differ in every bit position"""
    x = (np.asarray(j, dtype=np.uint64) + np.uint64(salt)) * np.uint64(0x9E3779B97F4A7C15)
    x ^= x >> np.uint64(29)
    x *= np.uint64(0xBF58476D1CE4E5B9)
    x ^= x >> np.uint64(32)
    return (x & np.uint64(0xFFFFFFFF)).astype(np.int64)


def lay_hashed(case, lo=MIN_RAIL, span=SPAN, dtype=np.int16):
    """the capture of a Case of run_level_seams_inputs: every on sample its own I and Q"""
    j = np.arange(case.n)
    on = np.zeros(case.n, dtype=bool)
    for a, f, _ in case.runs:
        assert 0 <= a < f <= case.n
        on[a:f] = True
    with np.errstate(over="ignore"):
        hi, hq = _hash(j, 1), _hash(j, 2)
    i = (lo + hi % span) * np.where(hi >> 20 & 1, -1, 1)
    qq = (lo + hq % span) * np.where(hq >> 20 & 1, -1, 1)
    iq = np.zeros(2 * case.n, dtype)
    iq[0::2] = np.where(on, i, 0)
    iq[1::2] = np.where(on, qq, 0)
    return iq


def seam_cases():
    """one capture per layout (the "first" variant: where the levels' largest output sat says nothing here)"""
    return [c for c in S.seam_cases() if c.name.endswith("-first")]


def dense_cases():
    return S.dense_cases()[:3]


def long_run_case():
    return S.long_run_cases()[0]


# S7: behind fs32_fs4 (decimation 1, 32 taps) a pulse that lasts to the capture's last sample is still on PAD outputs
# later, in the zero padding: the window then still holds 32 - PAD of its samples
PAD = 5
OPEN_PAD_SPB = 500
OPEN_PAD_N = 4 * S.T + 404 - PAD            # n_out = 4500: a partial last tile, and n no multiple of a buffer


def open_pad_capture():
    """-> (capture, samples, samples per buffer): a pulse across a tile seam and a pulse from 4200 to the end, both with
    +-100 LSB of noise on both rails"""
    n = OPEN_PAD_N
    rng = np.random.default_rng(12)
    i = np.zeros(n, np.int64)
    qq = np.zeros(n, np.int64)
    for a, f in ((900, 1300), (4200, n)):
        i[a:f] = 1500 + rng.integers(-100, 101, size=f - a)
        qq[a:f] = -700 + rng.integers(-100, 101, size=f - a)
    iq = np.zeros(2 * n, np.int16)
    iq[0::2] = i
    iq[1::2] = qq
    return iq, n, OPEN_PAD_SPB
