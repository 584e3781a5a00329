"""Input builders for the tuned / carrier front ends' bound tests (test_gpu_tuned_bounds.py; checked on the CPU by
test_tuned_bounds_host.py), numpy only: filters written as JSON, the captures of the tap sweep, the windows that push
the fused chain towards its error bound, and the windows planted around the quiet shortcut's decision.  Nothing here
knows what the kernels compute: every expected value comes from tests/tuned_contract.py."""
import json

import numpy as np

WINDOW = 512                    # outputs per wave tile with the quiet shortcut (R = 8); 1024 without it (R = 16)
TAP_PAD = 32                    # tap counts are padded to a multiple of this (ntaps_pad)
DC = 400.0 * (1 + 0.5j)


def write_filter(tmp_path, name, stages):
    p = tmp_path / (name + ".json")
    p.write_text(json.dumps({"filter": {"stages": [{"decimation": int(d), "taps": [float(t) for t in taps]}
                                                   for d, taps in stages]}}))
    return str(p)


def rand_taps(n, seed, total=1.3):
    h = np.random.default_rng(seed).normal(0, 1, n)
    return (h / np.abs(h).sum() * total).astype(np.float32)


def tight(re, im, A, n_win, rng, cancel):
    """windows whose products all have one sign in the real component (partial sums up to sum(|re| + |im|) A), or
    whose second half cancels the first to a few per cent; one sample of each window moves by a few LSB so the
    outputs spread over a few ulp around one magnitude.  -> capture, output indices of the windows"""
    T = re.size
    sr = np.where(re >= 0, 1, -1)
    si = np.where(im >= 0, -1, 1)
    w = np.abs(re.astype(np.float64)) + np.abs(im.astype(np.float64))
    if cancel:
        flip = np.cumsum(w) / w.sum() > 0.52
        sr, si = np.where(flip, -sr, sr), np.where(flip, -si, si)
    n = (n_win + 1) * (T + 1)
    xr = rng.integers(-A // 4, A // 4 + 1, size=n)
    xi = rng.integers(-A // 4, A // 4 + 1, size=n)
    # the tap at which one LSB moves the output by about two float32 ulp of its magnitude
    mag0 = np.hypot(np.sum(re * sr - im * si), np.sum(re * si + im * sr)) * A / 2048.0
    kp = int(np.argmin(np.abs(w - 2048.0 * 2.0 ** -22 * mag0)))
    outs = []
    for i in range(n_win):
        e = (i + 1) * (T + 1) - 1
        k = np.arange(T)
        xr[e - k] = sr * A
        xi[e - k] = si * A
        xr[e - kp] = sr[kp] * (A - 8) + rng.integers(-8, 9)
        outs.append(e)
    iq = np.empty(2 * n, np.int16)
    iq[0::2], iq[1::2] = xr, xi
    return iq, np.array(outs)


def ntaps_pad(ntaps):
    return -(-ntaps // TAP_PAD) * TAP_PAD


def interleave(z):
    """complex samples (integer valued) -> int16 I,Q"""
    out = np.empty(2 * z.size, np.int16)
    re, im = np.rint(z.real), np.rint(z.imag)
    assert re.min() >= -32768 and re.max() <= 32767 and im.min() >= -32768 and im.max() <= 32767
    out[0::2], out[1::2] = re, im
    return out


def as_complex(iq):
    iq = np.asarray(iq).reshape(-1)
    return iq[0::2].astype(np.float64) + 1j * iq[1::2].astype(np.float64)


def sum64(iq, re, im, spb):
    """float64 sum_k (re[k] + j im[k]) x[n - k] / 2048 over the float32 taps and the int16 samples, zero history, the
    capture zero padded to whole buffers as contract_rx pads it: [n_padded, 2]"""
    x = as_complex(iq)
    n = -(-x.size // spb) * spb
    c = np.asarray(re, np.float64) + 1j * np.asarray(im, np.float64)
    y = np.convolve(np.concatenate([x, np.zeros(n - x.size)]), c)[:n] / 2048.0
    return np.stack([y.real, y.imag], axis=1)


def unaligned_view(iq):
    """the same samples behind a pointer one sample (4 bytes) past a 16-byte boundary: a view into a copy"""
    iq = np.asarray(iq, np.int16).reshape(-1)
    store = np.zeros(iq.size + 16, np.int16)
    off = (-(store.ctypes.data // 2) % 8 + 2) % 8           # int16 index of a 16-byte boundary, plus one sample
    v = store[off:off + iq.size]
    v[:] = iq
    return v


# ------------------------------------------------------------------- 1. tap-count sweep ----

SWEEP_SPB = 4096
SWEEP_N = 3 * SWEEP_SPB + 257
SWEEP_STRETCHES = ((1700, 3100), (5800, 7200), (9900, 11300))
# 1 .. 256 run the fused forms, every ntaps_pad from 32 to 256 occurs (161 / 192: 192, which no other count gives)
SWEEP_TAPS = [1, 15, 16, 17, 32, 33, 48, 64, 65, 96, 128, 129, 161, 192, 224, 240, 241, 255, 256]


def sweep_capture(seed=1):
    """uniform +-1500 LSB with three stretches of +-30 LSB, each long enough to hold a whole R = 8 window (256
    samples of history and 512 outputs) at any alignment"""
    rng = np.random.default_rng(seed)
    x = rng.integers(-1500, 1501, size=2 * SWEEP_N)
    for lo, hi in SWEEP_STRETCHES:
        x[2 * lo:2 * hi] = rng.integers(-30, 31, size=2 * (hi - lo))
    return x.astype(np.int16)


# --------------------------------------------------------------- 2. distance to the bound ----

MARGIN_SEG = 4096
MARGIN_SEGMENTS = ("aligned", "cancel", "tones", "noise")


def margin_capture(re, im, nu, A, rng):
    """four segments of MARGIN_SEG outputs: sign-aligned windows (tight, cancel=False), cancelling windows, a
    full-scale tone at nu beside a tone at -nu, full-scale noise.  With A = 32767 the planted windows of the
    second half of the aligned segment and some noise samples sit at -32768.  -> capture, aligned output indices"""
    T = re.size
    n_win = MARGIN_SEG // (T + 1) - 1
    segs = []
    for cancel in (False, True):
        iq, outs = tight(re, im, A, n_win, rng, cancel)
        rest = rng.integers(-A // 4, A // 4 + 1, size=2 * MARGIN_SEG - iq.size)
        seg = np.concatenate([iq, rest.astype(np.int16)])
        if not cancel:
            aligned_outs = outs
            if A == 32767:
                late = seg[MARGIN_SEG:]                     # (I,Q interleaved: the second half of the segment)
                late[late == -32767] = -32768
        segs.append(seg)
    t = np.arange(MARGIN_SEG, dtype=np.float64)
    ph = 2.0 * np.pi * ((nu * t) % 1.0)
    z = np.rint(0.7 * A * np.exp(1j * ph)) + np.rint(0.3 * A * np.exp(-1j * ph))
    z = np.clip(z.real, -A, A) + 1j * np.clip(z.imag, -A, A)
    segs.append(interleave(z))
    lo = -32768 if A == 32767 else -A
    nz = rng.integers(lo, A + 1, size=2 * MARGIN_SEG)
    if A == 32767:
        nz[rng.integers(0, nz.size, size=64)] = -32768
    segs.append(nz.astype(np.int16))
    return np.concatenate(segs), aligned_outs


# ------------------------------------------------------------------ 3. tap magnitudes ----

SCALES = [1e-15, 1e-6, 1e-3, 1.0, 37.5, 1e6, 1e15]
SCALE_N = 2 * 8192 + 300
SCALE_STRETCH = (6000, 8000)


def scale_capture(seed=3):
    """noise of +-1500 LSB with one stretch of +-10 LSB"""
    rng = np.random.default_rng(seed)
    x = rng.integers(-1500, 1501, size=2 * SCALE_N)
    lo, hi = SCALE_STRETCH
    x[2 * lo:2 * hi] = rng.integers(-10, 11, size=2 * (hi - lo))
    return x.astype(np.int16)


# ------------------------------------------------------- 4. the quiet shortcut's decision ----

QUIET_FACTORS = (0.25, 0.5, 0.75, 1.0, 1.5, 2.0, 4.0)
QUIET_DS = (0j, DC, 12000 + 0j)
QUIET_DC_LEVELS = (0, 100, 1000, 5000, 15000, 30000)
SQRT2 = 1.41421356237309515


def tap_sums(re, im):
    """A = sum |c[k]|, G = |sum c[k]| of the float32 taps, in double"""
    c = np.asarray(re, np.float64) + 1j * np.asarray(im, np.float64)
    return float(np.abs(c).sum()), float(abs(c.sum()))


def spike_offsets(ntaps):
    """offsets of the lone spike relative to its tile's first output (b); -ntaps and anything before it weigh in
    none of the tile's outputs"""
    Tp = ntaps_pad(ntaps)
    offs = [-(ntaps - 1), -(ntaps - 2), -ntaps, -1, 0, 1, 3, 4, 255, 256, WINDOW - 4, WINDOW - 1, -Tp]
    out = []
    for o in offs:
        if o not in out:
            out.append(o)
    return out


def documented_lhs(iq, re, im, t0, Tp, tile=WINDOW):
    """the left-hand side of the documented quiet inequality, sqrt(2) / (2 2048) (A a + G b), for the window of the
    tile whose first output is t0: samples t0 - Tp .. t0 + tile - 1, a = the larger component range, b = the larger
    |min + max|"""
    A, G = tap_sums(re, im)
    w = np.asarray(iq).reshape(-1)[2 * (t0 - Tp):2 * (t0 + tile)].astype(np.int64)
    i, q = w[0::2], w[1::2]
    a = max(i.max() - i.min(), q.max() - q.min())
    b = max(abs(i.max() + i.min()), abs(q.max() + q.min()))
    return SQRT2 / 4096.0 * (A * a + G * b)


def interior_tiles(n, Tp, tile=WINDOW):
    """first outputs of the tiles whose window holds capture samples only"""
    return [t0 for t0 in range(0, n, tile) if t0 >= Tp and t0 + tile <= n]


def quiet_count_bounds(iq, re, im, thr, bits, Tp, tile=WINDOW):
    """(at least, at most) windows a sound shortcut built on the documented inequality takes: interior windows whose
    left-hand side is below half the threshold; interior windows whose contract bits are all zero"""
    n = np.asarray(iq).size // 2
    lo = hi = 0
    for t0 in interior_tiles(n, Tp, tile):
        lo += documented_lhs(iq, re, im, t0, Tp, tile) < 0.5 * thr
        hi += not bits[t0:t0 + tile].any()
    return int(lo), int(hi)


def quiet_capture(re, im, thr, seed=4):
    """One feature per interior R = 8 tile, every other tile (a feature owns the tile before it too, so a window's
    history is the feature's own level), from the library's taps (re, im) of one nu and one threshold:
      a  worst-case spread windows x = d + (a/2) (sgn re[k], -sgn im[k]) laid on the taps of the tile's first,
         middle and last output, a = QUIET_FACTORS times the value where the documented inequality is an equality,
         d in QUIET_DS
      b  one lone spike of 8 thr 2048 / max|c| (clipped to the sample range) over DC, at spike_offsets
      c  a window holding both -32768 and 32767
      d  DC-only windows, |d| in QUIET_DC_LEVELS
      e  +-3 LSB of noise around 0
    -> capture, [(kind, first output of the tile, detail)]"""
    rng = np.random.default_rng(seed)
    T = re.size
    A, G = tap_sums(re, im)
    sr = np.where(np.asarray(re) >= 0, 1.0, -1.0)
    si = np.where(np.asarray(im) >= 0, -1.0, 1.0)
    cmax = float(np.hypot(np.asarray(re, np.float64), np.asarray(im, np.float64)).max())
    plan = []
    for d in QUIET_DS:
        b = 2.0 * max(abs(d.real), abs(d.imag))
        a_eq = (thr * 4096.0 / SQRT2 - G * b) / A
        if a_eq < 2.0:                                      # the offset alone is loud: the spread of d = 0
            a_eq = thr * 4096.0 / SQRT2 / A
        for f in QUIET_FACTORS:
            half = min(max(1, int(np.rint(0.5 * f * a_eq))), 20000)
            for pos in (0, WINDOW // 2, WINDOW - 1):
                plan.append(("spread", d, (half, pos, f)))
    height = int(min(np.rint(8.0 * thr * 2048.0 / cmax), 32767 - abs(DC.real)))
    for off in spike_offsets(T):
        plan.append(("spike", DC, (height, off)))
    plan.append(("extremes", 0j, None))
    for lvl in QUIET_DC_LEVELS:
        plan.append(("dc", complex(lvl), lvl))
    for _ in range(4):
        plan.append(("hush", 0j, None))
    n = WINDOW * (2 * len(plan) + 2) + 77
    z = np.zeros(n, np.complex128)
    feats = []
    for i, (kind, d, detail) in enumerate(plan):
        t0 = WINDOW * (2 * i + 2)
        z[t0 - WINDOW:t0 + WINDOW] = d
        if kind == "spread":
            half, pos, _ = detail
            k = np.arange(T)
            z[t0 + pos - k] = d + half * (sr + 1j * si)
        elif kind == "spike":
            height, off = detail
            z[t0 + off] = d + height
        elif kind == "extremes":
            z[t0 + 100] = -32768 - 32768j
            z[t0 + 101] = 32767 + 32767j
        elif kind == "hush":
            m = 2 * WINDOW
            z[t0 - WINDOW:t0 + WINDOW] = rng.integers(-3, 4, size=m) + 1j * rng.integers(-3, 4, size=m)
        feats.append((kind, t0, detail))
    return interleave(z), feats


def loud_capture(n, seed=5):
    """full-band noise of +-6000 LSB: what a context runs before the planted capture, so that words a quiet window
    leaves behind are ones"""
    return np.random.default_rng(seed).integers(-6000, 6001, size=2 * n).astype(np.int16)


# ------------------------------------------------------------------- 5. split launches ----

SPLIT_N = 5 * 65536 + 777


def tiled(iq, n):
    """the capture repeated to n samples"""
    iq = np.asarray(iq, np.int16).reshape(-1)
    reps = -(-2 * n // iq.size)
    return np.tile(iq, reps)[:2 * n]
