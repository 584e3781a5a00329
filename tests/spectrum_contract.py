"""The carrier survey's contract (include/ookiedokie_amd.h, at ookd_spectrum_* and ookd_suggest_carriers) restated
in numpy: the Welch spectrum in float64, the error bound B[k], the suggestion rule, and the captures the spectrum
tests use.  Shared by test_spectrum_host.py and test_gpu_spectrum.py."""
import numpy as np

from tests.tuned_contract import golden_capture, moved

N = 1024
EPS = 12.0 * 10.0 / 16777216.0          # OOKD_SPECTRUM_EPS
MIN_RATIO, MIN_SPACING = 64.0, 32       # OOKD_CARRIER_MIN_RATIO, OOKD_CARRIER_MIN_SPACING
RATE = 3000000
DC = 400.0 * (1 + 0.5j)
NOISE = 40
# golden capture, messages in it, carrier offset in Hz, the bin the issue's CPU check found
MOVES = [(cap, nmsg, hz, b) for cap, nmsg in (("G1", 3), ("G2", 2)) for hz, b in ((600e3, 205), (-900e3, -307))]


def window():
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(N, dtype=np.float64) / N)


def np_spectrum(iq):
    """SC16Q11 capture (int16 I,Q pairs) -> (frames, S[1024] float64): whole 1024-sample periodic-Hann frames,
    sum over frames of |FFT|^2"""
    iq = np.asarray(iq, dtype=np.int16).reshape(-1)
    frames = (iq.size // 2) // N
    S = np.zeros(N, dtype=np.float64)
    if frames == 0:
        return 0, S
    w = window()
    chunk = 4096                        # frames per FFT call: bounds the memory of the large captures
    for f0 in range(0, frames, chunk):
        part = iq[2 * N * f0:2 * N * min(frames, f0 + chunk)].astype(np.float64)
        z = (part[0::2] + 1j * part[1::2]) / 2048.0
        X = np.fft.fft(z.reshape(-1, N) * w, axis=1)
        S += (X.real * X.real + X.imag * X.imag).sum(axis=0)
    return frames, S


def bound(S):
    """B[k] = 2 EPS sqrt(S[k] E) + EPS^2 E + EPS S[k], E = sum_k S[k]"""
    E = S.sum()
    return 2.0 * EPS * np.sqrt(S * E) + EPS * EPS * E + EPS * S


def worst_over_bound(power, S):
    """max_k |power[k] - S[k]| / B[k]; 0 for a spectrum that is all zero on both sides"""
    B = bound(S)
    err = np.abs(np.asarray(power, dtype=np.float64) - S)
    if not B.any():
        return 0.0 if not err.any() else float("inf")
    return float((err / np.where(B > 0, B, np.finfo(np.float64).tiny)).max())


def bin_nu(k):
    k %= N
    return (k if k < N // 2 else k - N) / N


def py_suggest(power, frames=1, min_ratio=0.0, min_spacing=0, capacity=16):
    """the header's rule: ([(bin, at_dc, power, ratio)], floor)"""
    p = [float(x) for x in power]
    assert len(p) == N
    min_ratio = min_ratio or MIN_RATIO
    min_spacing = min_spacing or MIN_SPACING
    srt = sorted(p)
    floor = (srt[N // 2 - 1] + srt[N // 2]) / 2.0
    out = []
    if frames == 0:
        return out, floor
    live = [True] * N
    while len(out) < capacity:
        best = None
        for k in range(N):
            if live[k] and (best is None or p[k] > p[best]):
                best = k
        if best is None or not p[best] > 0.0 or p[best] < min_ratio * floor:
            break
        b = best if best < N // 2 else best - N
        with np.errstate(divide="ignore"):
            ratio = float(np.float64(p[best]) / np.float64(floor))
        out.append((b, abs(b) <= 1, p[best], ratio))
        for k in range(N):
            d = abs(k - best)
            if min(d, N - d) <= min_spacing:
                live[k] = False
    return out, floor


def as_tuples(carriers):
    return [(c.bin, c.at_dc, c.power, c.ratio) for c in carriers]


def moved_golden(cap, hz, scale=1.0, seed=0):
    """a golden capture moved to hz at 3 MHz, with the DC term and +-40 LSB of noise
    -> (capture, base, vectors entry)"""
    base, g = golden_capture(cap)
    return moved(base, hz / RATE, DC, NOISE, seed=seed, scale=scale), base, g


def two_transmitters(seed=0):
    """G1 at half level and +600 kHz plus G2 at half level and -900 kHz, DC and noise once.  G2 is the longer
    capture; G1 is padded with silence."""
    b1, g1 = golden_capture("G1")
    b2, g2 = golden_capture("G2")
    n = max(b1.size, b2.size)
    b1 = np.concatenate([b1, np.zeros(n - b1.size, np.int16)])
    b2 = np.concatenate([b2, np.zeros(n - b2.size, np.int16)])
    a = moved(b1, 600e3 / RATE, 0j, 0, scale=0.5).astype(np.int32)
    b = moved(b2, -900e3 / RATE, DC, NOISE, seed=seed, scale=0.5).astype(np.int32)
    return np.clip(a + b, -32768, 32767).astype(np.int16), (b1, g1), (b2, g2)
