"""The pulse levels' contract (include/ookiedokie_amd.h, "Pulse levels") restated in numpy, independent of the
library: power + edge list -> the peak of every on-run, the tiles that hold an on output, and the level of a message.
The power comes from tests.test_survey_host.oracle_power (untuned) or tests.tuned_survey_contract.contract_power
(tuned), both over the capture zero padded to whole buffers.  Shared by tests/test_run_levels_host.py,
tests/test_gpu_run_levels.py and the two seam files (tests/test_run_level_seams_host.py,
tests/test_gpu_run_level_seams.py), whose captures behind a filter are built here, on the reference's edges."""
import numpy as np

RATE = 3000000
SPB = 8192
THR = 0.1


def nominal_power(scale=1.0):
    """(0.95 scale)^2: the on power of a golden capture at `scale` of its nominal level (device.c:675)"""
    return (0.95 * scale) ** 2


def padded(iq, spb=SPB):
    """the capture zero padded to whole buffers, as a run sees it"""
    iq = np.asarray(iq).reshape(-1)
    n = iq.size // 2
    out = np.zeros(2 * (-(-n // spb) * spb), dtype=iq.dtype)
    out[:iq.size] = iq
    return out


def ref_edges(oracle, fir, iq, spb=SPB, thr=THR):
    """the reference's edge list of a capture: its filter (None: the samples) and its threshold over the capture
    zero padded to whole buffers"""
    from tests.helpers import edges_of
    y = oracle.unpack(padded(iq, spb))
    if fir is not None:
        y = oracle.fir_run(fir, y)
    return edges_of(oracle.threshold(y, thr)).astype(np.uint64)


def runs_of(edges, n_out):
    """[(start, end)] of the on-runs: [e[2r], e[2r + 1]), the last one up to n_out when it is open"""
    e = [int(x) for x in np.asarray(edges, dtype=np.uint64)]
    assert all(a < b for a, b in zip(e, e[1:])) and (not e or e[-1] < n_out), "an edge list is strictly increasing, below n_out"
    return [(e[i], e[i + 1] if i + 1 < len(e) else int(n_out)) for i in range(0, len(e), 2)]


def peaks_of(power, edges, n_out):
    """peak[r] = the maximum of the power bit patterns over on-run r, as float32"""
    bits = np.ascontiguousarray(power, dtype=np.float32).view(np.uint32)
    assert bits.size == n_out
    out = np.zeros(len(runs_of(edges, n_out)), dtype=np.uint32)
    for r, (a, f) in enumerate(runs_of(edges, n_out)):
        out[r] = bits[a:f].max()
    return out.view(np.float32)


def tiles_filtered_of(edges, n_out, tile):
    """tiles [t tile, (t + 1) tile) with at least one output of an on-run"""
    hit = np.zeros(-(-int(n_out) // tile) + 1, dtype=bool)
    for a, f in runs_of(edges, n_out):
        hit[a // tile:(f - 1) // tile + 1] = True
    return int(hit.sum())


def message_levels_of(edges, peaks, msg_samples, pulses):
    """message m: the on-runs rising at or below msg_samples[m] and above msg_samples[m - 1], the last `pulses` of
    them, the lower median of their peaks; 0 without any"""
    e = [int(x) for x in np.asarray(edges, dtype=np.uint64)]
    rise = e[0::2]
    p = np.asarray(peaks, dtype=np.float32)
    assert p.size == len(rise)
    out = np.zeros(len(msg_samples), dtype=np.float32)
    prev = -1
    for m, s in enumerate(int(x) for x in msg_samples):
        mine = [r for r, a in enumerate(rise) if prev < a <= s][-pulses:]
        if mine:
            out[m] = np.sort(p[mine])[(len(mine) - 1) // 2]
        prev = s
    return out


def assert_same_bits(got, want, what=""):
    g = np.ascontiguousarray(got, dtype=np.float32).view(np.uint32)
    w = np.ascontiguousarray(want, dtype=np.float32).view(np.uint32)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    bad = np.nonzero(g != w)[0]
    assert bad.size == 0, (what, bad[:6].tolist(), g[bad[:6]].tolist(), w[bad[:6]].tolist())


def two_level_capture(vectors):
    """golden G1 at nominal level followed by G1 at 1/4 of it, +-40 LSB of noise (seeds 1 and 2)"""
    from tests.test_survey_host import scaled_golden
    g, a = scaled_golden(vectors, "G1", 1.0, noise_seed=1)
    _, b = scaled_golden(vectors, "G1", 0.25, noise_seed=2)
    return g, np.concatenate([a, b]), a.size // 2


# ---- the seam captures behind a filter (tests/run_level_seams_inputs.py), built on the reference --------------------

SEAM_NU = 600e3 / RATE              # the tuned seam cases' carrier


def oracle_fir(oracle, shape):
    """the reference's filter of a seam shape: a golden filter's name, "three", "narrow32", "narrow4" """
    from tests import run_level_seams_inputs as S
    from tests.helpers import golden_path
    if shape == "three":
        return oracle.make_fir(S.three_stages())
    if shape.startswith("narrow"):
        return oracle.make_fir(S.narrow_stages(int(shape[6:])))
    return oracle.load_filter_json(golden_path("filters", shape))


_built = {}


def seam_filtered(oracle, shape, which):
    """-> (capture, samples, samples per buffer, targets) of FILTERED_TARGETS[which] behind `shape`"""
    from tests import run_level_seams_inputs as S
    if (shape, which) not in _built:
        D = S.SHAPE_D[shape]
        n, spb = S.FILTERED_OUT * D, 500 * D
        fir = oracle_fir(oracle, shape)
        iq = S.filtered_capture(lambda x: ref_edges(oracle, fir, x, spb), n, D, S.FILTERED_PULSE, S.FILTERED_TARGETS[which])
        _built[shape, which] = (iq, n, spb, S.FILTERED_TARGETS[which])
    return _built[shape, which]


def seam_narrow(oracle, tile):
    """-> (capture, samples, samples per buffer, targets): NARROW_TARGETS behind the single stage whose tile is `tile`"""
    from tests import run_level_seams_inputs as S
    if ("narrow", tile) not in _built:
        fir = oracle_fir(oracle, "narrow%d" % tile)
        iq = S.filtered_capture(lambda x: ref_edges(oracle, fir, x), S.NARROW_N, 1, S.NARROW_PULSE, S.NARROW_TARGETS)
        _built["narrow", tile] = (iq, S.NARROW_N, SPB, S.NARROW_TARGETS)
    return _built["narrow", tile]


def seam_tuned(flt, which):
    """the fs32_fs4 seam capture with its pulses moved to SEAM_NU, laid on the contract of a context tuned there
    (flt: the library's filter, whose tuned taps the contract reads) -> (capture, samples, samples per buffer,
    targets, the contract's stages)"""
    from tests import run_level_seams_inputs as S
    from tests.helpers import edges_of
    from tests.tuned_contract import contract_rx, lib_stages, moved
    stages = lib_stages(flt, SEAM_NU)
    if ("tuned", which) not in _built:
        n, spb = S.FILTERED_OUT, 500
        iq = S.filtered_capture(lambda x: edges_of(contract_rx(x, stages, THR, spb)[0]), n, 1, S.FILTERED_PULSE,
                                S.FILTERED_TARGETS[which], move=lambda x: moved(x, SEAM_NU))
        _built["tuned", which] = (iq, n, spb, S.FILTERED_TARGETS[which])
    return _built["tuned", which] + (stages,)


def assert_targets(edges, n_out, targets, what=""):
    """every target is an edge of its kind ("open": the list ends on)"""
    e = [int(x) for x in edges]
    for kind, j in targets:
        if kind == "open":
            assert len(e) % 2 == 1 and j == n_out, (what, kind, j, len(e))
        else:
            assert j in e[0 if kind == "rise" else 1::2], (what, kind, j, e)
