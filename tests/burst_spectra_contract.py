"""The burst spectra's contract (include/ookiedokie_amd.h, "Burst spectra") restated in numpy float64: the spectrum of
one burst, its summary, the keyed spectrum, the span rule and the host rule ookd_suggest_burst_carriers.  Shared by
test_burst_spectra_host.py and test_gpu_burst_spectra.py."""
import numpy as np

from tests.spectrum_contract import N, bin_nu, bound, np_spectrum, worst_over_bound

MIN_SHARE, MIN_SPACING = 0.125, 32      # OOKD_BURST_MIN_SHARE, OOKD_CARRIER_MIN_SPACING
MIN_SPAN, MAX_ROWS = 32, 8192           # OOKD_BURST_SPECTRA_MIN_SPAN, OOKD_BURST_SPECTRA_MAX_ROWS
FIELDS = ("frames", "total_power", "dc_power", "peak_power", "peak_bin")


def np_burst_spectrum(iq16, first_sample, num_samples):
    """SC16Q11 capture [n, 2] or flat, one burst -> (F_b, S_b[1024]): the whole frames inside the burst alone"""
    iq = np.asarray(iq16, dtype=np.int16).reshape(-1, 2)
    F = int(num_samples) // N
    return np_spectrum(iq[int(first_sample):int(first_sample) + N * F].reshape(-1))


def np_summary(S, frames):
    """the summary of a spectrum S of `frames` frames, as the header states it"""
    if frames == 0:
        return dict(frames=0, total_power=0.0, dc_power=0.0, peak_power=0.0, peak_bin=0)
    k = 2 + int(np.argmax(S[2:N - 1]))              # (argmax returns the lowest index among equals)
    return dict(frames=int(frames), total_power=float(S.sum()), dc_power=float((S[N - 1] + S[0]) + S[1]), peak_power=float(S[k]),
                peak_bin=k)


def assert_summary_of(entry, power, frames, what=""):
    """the exact relations between a summary and the 1024 doubles it was taken from"""
    power = np.asarray(power, dtype=np.float64)
    assert int(entry["frames"]) == frames, (what, entry, frames)
    if frames == 0:
        assert not power.any() and all(float(entry[k]) == 0.0 for k in FIELDS[1:]), (what, entry)
        return
    want = np_summary(power, frames)
    assert int(entry["peak_bin"]) == want["peak_bin"] and 2 <= want["peak_bin"] <= N - 2, (what, entry, want)
    assert float(entry["peak_power"]) == float(power[int(entry["peak_bin"])]), (what, entry)      # bit for bit
    assert float(entry["dc_power"]) == want["dc_power"], (what, entry, want)
    total = float(entry["total_power"])
    assert abs(total - want["total_power"]) <= N * 2.0 ** -53 * want["total_power"], (what, entry, want)


def peak_is_decided(S):
    """numpy's top two bins of 2 .. 1022 differ by more than twice their bounds: the library's peak_bin must agree"""
    B = bound(S)
    order = np.argsort(S[2:N - 1])[::-1] + 2
    a, b = int(order[0]), int(order[1])
    return S[a] - S[b] > 2.0 * (B[a] + B[b])


def spans_of(total, span):
    return -(-int(total) // (N * span))


def span_rule(total, span=0):
    """the span the library takes, or the name of the refusal"""
    if span and (span < MIN_SPAN or span & (span - 1)):
        return "arg"
    fit = MIN_SPAN
    while 2 * spans_of(total, fit) > MAX_ROWS:
        fit *= 2
    if span and span < fit:
        return "capacity"
    return span or fit


def py_suggest_burst_carriers(spectra, min_share=0.0, min_spacing=0, capacity=16):
    """the header's rule over a list of dicts (or a dict of arrays) -> ([(bin, bursts, frames, power)], carrier_of_burst)"""
    if isinstance(spectra, dict):
        spectra = [dict((k, spectra[k][b]) for k in FIELDS) for b in range(len(spectra["frames"]))]
    min_share = min_share or MIN_SHARE
    min_spacing = min_spacing or MIN_SPACING
    weight = [0.0] * N
    qualifies = []
    for s in spectra:
        rest = float(s["total_power"]) - float(s["dc_power"])
        q = int(s["frames"]) >= 1 and rest > 0.0 and float(s["peak_power"]) >= min_share * rest
        qualifies.append(q)
        if q:
            weight[int(s["peak_bin"])] += float(s["peak_power"])
    live = [True] * N
    owner = [-1] * N
    out = []
    while len(out) < capacity:
        best = None
        for k in range(N):
            if live[k] and (best is None or weight[k] > weight[best]):
                best = k
        if best is None or not weight[best] > 0.0:
            break
        for k in range(N):
            d = abs(k - best)
            if live[k] and min(d, N - d) <= min_spacing:
                owner[k] = len(out)
                live[k] = False
        out.append([best if best < N // 2 else best - N, 0, 0, 0.0])
    of = []
    for s, q in zip(spectra, qualifies):
        o = owner[int(s["peak_bin"])] if q else -1
        of.append(o)
        if o >= 0:
            out[o][1] += 1
            out[o][2] += int(s["frames"])
            out[o][3] += float(s["peak_power"])
    return [tuple(c) for c in out], of


def as_tuples(carriers):
    return [(c.bin, c.bursts, c.frames, c.power) for c in carriers]

