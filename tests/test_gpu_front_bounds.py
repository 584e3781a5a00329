"""The front end's guard band, measured: which kernel a context runs (stats["front_form"] against the dispatch
rules of launch_front / plan_real_form), how close each kernel's floats come to the forward error bound its band
is built from, and bits at the inputs where that bound is tight -- sign-aligned full-scale windows, cancellation at
the threshold, wide samples placed around tile boundaries.  Every result is compared with the CPU oracle, the
reference-order float chain."""
import json
import zlib

import numpy as np
import pytest

from tests.helpers import edges_of, golden_path

pytestmark = pytest.mark.gpu

# The margin the bounds must keep: measured |y_kernel - y_ref| per component over the bound.  Above 1.0 a band is
# unsound; between 0.5 and 1.0 the bound's safety factor (mfma_error_bound*, guard_error) is what must grow.
MARGIN = 0.5
TILE_IN = 1024              # input samples per wave tile of both matrix-core kernels


@pytest.fixture(scope="module")
def ok():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from ookiedokie_amd import build as okbuild
    okbuild.build()
    import ookiedokie_amd as okm
    okm.lib()
    return okm


def _write(tmp_path, name, stages):
    p = tmp_path / (name + ".json")
    p.write_text(json.dumps({"filter": {"stages": [{"decimation": int(d), "taps": [float(t) for t in taps]}
                                                   for d, taps in stages]}}))
    return str(p)


def _golden_stages(oracle, name):
    of = oracle.load_filter_json(golden_path("filters", name))
    return [(int(of.decimation[s]), of.stage_taps(s).astype(np.float32)) for s in range(of.num_stages)]


def _taps(rng, n, kind, total=1.7):
    """float32 taps, sum|h| ~ total.  rand24: random, full 24-bit mantissas (the two fp16 pieces leave a residue);
    exact22: multiples of 2^-22 below 2^-1 (the pieces carry them exactly); mixed: every other tap 2^-30 smaller."""
    h = rng.normal(0, 1, n)
    if kind == "mixed":
        h[1::2] *= 2.0 ** -30
    h = h / np.abs(h).sum() * total
    if kind == "exact22":
        h = np.clip(np.round(h * 2.0 ** 22), -(2 ** 21) + 1, 2 ** 21 - 1) * 2.0 ** -22
        if not np.any(h):
            h[0] = 0.25
    return h.astype(np.float32)


def _folded(stages):
    """the filter as one: y[o] = sum_t g[t] x[D o + D - 1 - t] (a 1-stage filter: g = h, D = 1; two
    decimate-by-2 stages: g[2 k2 + k1] = h2[k2] h1[k1], D = 4 -- fir.c's countdown starts at D)"""
    if len(stages) == 1:
        return stages[0][1].astype(np.float64), 1
    (_, h1), (_, h2) = stages
    g = np.zeros(2 * (h2.size - 1) + h1.size)
    for k2 in range(h2.size):
        g[2 * k2:2 * k2 + h1.size] += float(h2[k2]) * h1.astype(np.float64)
    return g, 4


def _sum64(iq, g, D):
    """float64 sum_t g[t] x[D o + D - 1 - t] / 2048 (zero history): exact enough to place inputs by"""
    x = iq[0::2].astype(np.float64) + 1j * iq[1::2].astype(np.float64)
    y = np.convolve(x, g)[:x.size][D - 1::D] / 2048.0
    return y


def _iq(i, q):
    out = np.empty(2 * i.size, np.int16)
    out[0::2], out[1::2] = i, q
    return out


# ------------------------------------------------------------------ which kernel runs ----

def _front_forms(ok):
    return dict(none=ok.FRONT_NO_FILTER, generic=ok.FRONT_GENERIC, fir1=ok.FRONT_FIR1_VALU,
                fir1x=ok.FRONT_FIR1_VALU_EXACT, mfma1=ok.FRONT_FIR1_MFMA, fir2=ok.FRONT_FIR2_VALU,
                fir2x=ok.FRONT_FIR2_VALU_EXACT, mfma2=ok.FRONT_FIR2_MFMA)


# (filter, Receiver keywords, threshold, expected form), from the rules:
#   no stages                                                       -> none
#   1 stage, decimation 1, taps padded to 32 <= 256                 -> mfma1 when plan_real_form prepared the
#       matrix-core image (not exact, not fir_valu, mfma_prepare_taps took the taps, every band edge scales exactly
#       into accumulator units -- mfma_scale_band --, p_star 0 / NaN or within [2^-100, 2^100]), else fir1 / fir1x
#   2 stages of decimation 2, <= 16 and <= 32 taps                  -> mfma2 under the same conditions, else fir2 / fir2x
#   anything else (257 taps and more, ...)                          -> generic
# A shard of a capture hands the filter its history as a halo and keeps the origin at 0: the same kernel as a
# whole capture.
DISPATCH = [
    ("none", None, {}, 0.1, "none"),
    ("unity1", "unity1", {}, 0.1, "mfma1"),
    ("unity16", "unity16", {}, 0.1, "mfma1"),
] + [("taps%d" % n, "taps%d" % n, {}, 0.1, "mfma1" if n <= 256 else "generic")
     for n in (32, 33, 64, 65, 128, 129, 256, 257)] + [
    ("taps256_valu", "taps256", dict(fir_valu=True), 0.1, "fir1"),
    ("taps257_valu", "taps257", dict(fir_valu=True), 0.1, "generic"),
    ("taps257_exact", "taps257", dict(exact_fir=True), 0.1, "generic"),
    ("fs32_fs4", "fs32_fs4", {}, 0.1, "mfma1"),
    ("fs32_fs4_exact", "fs32_fs4", dict(exact_fir=True), 0.1, "fir1x"),
    ("fs32_fs4_valu", "fs32_fs4", dict(fir_valu=True), 0.1, "fir1"),
    ("dec4", "fs128_fs16_dec4", {}, 0.1, "mfma2"),
    ("dec4_valu", "fs128_fs16_dec4", dict(fir_valu=True), 0.1, "fir2"),
    ("dec4_exact", "fs128_fs16_dec4", dict(exact_fir=True), 0.1, "fir2x"),
    # threshold 0 / negative / NaN: p_star 0 or NaN, band edges = p_star, which scale exactly
    ("thr0", "fs32_fs4", {}, 0.0, "mfma1"),
    ("thr_neg", "fs32_fs4", {}, -1.0, "mfma1"),
    ("thr_nan", "fs32_fs4", {}, float("nan"), "mfma1"),
    ("dec4_thr0", "fs128_fs16_dec4", {}, 0.0, "mfma2"),
    # p_star below 2^-100 / above 2^100 (with 1e-31 and 1e16 the scaled edges leave the floats as well)
    ("thr_tiny", "fs32_fs4", {}, 1e-31, "fir1"),
    ("thr_huge", "fs32_fs4", {}, 1e16, "fir1"),
    ("dec4_thr_tiny", "fs128_fs16_dec4", {}, 1e-31, "fir2"),
    # taps of 2^-40: c = 2^-65, p_star = 2^-102 scales to 2^28 -- only the p_star range refuses
    ("tiny_taps_pstar", "tiny40", {}, 2.0 ** -51, "fir1"),
    # taps of 2^-60: c = 2^-85, p_star = 2^-40 is in range but scales to 2^130 -- mfma_scale_band refuses
    ("tiny_taps_scale", "tiny60", {}, 2.0 ** -20, "fir1"),
    # taps beyond 2^100 of scaling: mfma_prepare_taps refuses
    ("taps_1e-35", "tiny116", {}, 1e-30, "fir1"),
    # where the two-stage family ends: one tap more than (16, 32), any decimations but 2 x 2, any other stage count
    ("fir2_17x32", "st:2x17,2x32", {}, 0.1, "generic"),
    ("fir2_16x33", "st:2x16,2x33", {}, 0.1, "generic"),
    ("dec2x1", "st:2x16,1x32", {}, 0.1, "generic"),
    ("dec1x2", "st:1x16,2x32", {}, 0.1, "generic"),
    ("dec2x4", "st:2x16,4x32", {}, 0.1, "generic"),
    ("dec4_one_stage", "st:4x32", {}, 0.1, "generic"),
    ("dec2x2x2", "st:2x16,2x32,2x8", {}, 0.1, "generic"),
]


def _dispatch_filter(oracle, tmp_path, spec):
    if spec is None:
        return None
    if spec.startswith("st:"):              # "st:2x17,2x32": (decimation x taps) per stage
        shape = [tuple(int(v) for v in stage.split("x")) for stage in spec[3:].split(",")]
        rng = np.random.default_rng(sum(d * 100 + t for d, t in shape))
        return _write(tmp_path, spec[3:].replace(",", "_"), [(d, _taps(rng, t, "rand24", 1.2)) for d, t in shape])
    if spec.startswith("taps"):
        n = int(spec[4:])
        return _write(tmp_path, spec, [(1, _taps(np.random.default_rng(n), n, "rand24"))])
    if spec.startswith("tiny"):
        e = int(spec[4:])
        h = np.full(32, 2.0 ** -e, dtype=np.float32)
        h[1::3] *= -0.5
        return _write(tmp_path, spec, [(1, h)])
    return golden_path("filters", spec)


@pytest.mark.parametrize("spec,kw,thr,want", [c[1:] for c in DISPATCH], ids=[c[0] for c in DISPATCH])
def test_front_form_dispatch(ok, oracle, tmp_path, spec, kw, thr, want):
    forms = _front_forms(ok)
    path = _dispatch_filter(oracle, tmp_path, spec)
    f = ok.Filter.load(path) if path else None
    of = oracle.load_filter_json(path) if path else None
    rng = np.random.default_rng(3)
    n = 3 * 8192 + 100
    iq = rng.integers(-1500, 1501, size=2 * n).astype(np.int16)
    rx = ok.Receiver(f, None, max_samples=n, threshold=thr, edge_capacity=n + 64, **kw)
    assert rx.front_info()["form"] == forms[want]
    got = rx.rx(iq)
    assert got.stats["front_form"] == forms[want]
    want_r = oracle.rx(iq, of, thr, None, 8192, want_bits=True)
    assert (rx.bits() == want_r.bits).all()
    rx.close()


@pytest.mark.parametrize("name,want", [("fs32_fs4", "mfma1"), ("fs128_fs16_dec4", "mfma2")])
def test_front_form_batched_pipelined_sharded(ok, oracle, name, want):
    """the field is set by every kind of run: batched, pipelined in chunks, the shards of a capture"""
    import torch
    forms = _front_forms(ok)
    f = ok.Filter.load(golden_path("filters", name))
    of = oracle.load_filter_json(golden_path("filters", name))
    rng = np.random.default_rng(11)
    # batched
    n, caps = 40000, 3
    host = rng.integers(-1500, 1501, size=(caps, 2 * n)).astype(np.int16)
    dev_t = torch.from_numpy(host).cuda()
    rx = ok.Receiver(f, None, max_samples=n, max_captures=caps, edge_capacity=caps * n + 64)
    got = rx.rx_device(dev_t.data_ptr(), n, num_captures=caps)
    assert got.stats["front_form"] == forms[want]
    for c in range(caps):
        assert (rx.bits(c) == oracle.rx(host[c], of, 0.1, None, 8192, want_bits=True).bits).all(), c
    rx.close()
    # pipelined in chunks (a state machine behind the front end)
    dec = of.total_decimation
    d = ok.Device.load(golden_path("devices", "p3l-nexa2012"), 3000000 // dec)
    od = oracle.load_device_json(golden_path("devices", "p3l-nexa2012"), 3000000 // dec)[0]
    n = 64 * 8192
    iq = rng.integers(-1500, 1501, size=2 * n).astype(np.int16)
    rx = ok.Receiver(f, d, max_samples=n, pipeline_chunk_samples=4 * 8192)
    got = rx.rx(iq)
    want_r = oracle.rx(iq, of, 0.1, od, 8192, want_bits=True)
    assert got.stats["front_form"] == forms[want]
    assert (rx.bits() == want_r.bits).all()
    if got.stats["fsm_fallback_reason"] == 0:
        assert got.stats["pipeline_chunks"] >= 2
    rx.close()
    # shards: the second one starts from the first one's samples as its halo
    dev_t = torch.from_numpy(iq.copy()).cuda()
    half = n // 2
    for r, (lo, hi) in enumerate(((0, half), (half, n))):
        rx = ok.Receiver(f, None, max_samples=half, edge_capacity=half + 64)
        H = rx.halo_samples
        halo = iq[2 * (lo - H):2 * lo] if r else None
        res, _ = rx.shard_begin(dev_t.data_ptr() + 4 * lo, hi - lo, halo, r == 1, None)
        assert res.stats["front_form"] == forms[want], r
        b = rx.bits()
        assert (b == want_r.bits[lo // dec:lo // dec + b.size]).all(), r
        rx.close()


# -------------------------------------------------------------- distance to the bound ----

def _aligned(g, D, A, n_out, rng, cancel=False):
    """I: windows x[D o + D - 1 - t] = sign(g[t]) A for a stride of outputs o (every product of the window has the
    same sign, the partial sums run up to sum|g| A); cancel: the taps past the point where the running sum|g| passes
    ~52 % get the opposite sign -- full-scale partial sums, a small output.  Returns the samples and the outputs o."""
    T = g.size
    so = -(-T // D) + 1                         # outputs per window stride
    s = np.sign(g)
    s[s == 0] = 1
    if cancel:
        # the running sum reaches half the scale, the rest comes back down to ~4 % of it (for a symmetric filter the
        # halves cancel exactly: then taps of the second half keep their sign, largest first, until it is 4 %)
        a = np.abs(g)
        flip = np.cumsum(a) / a.sum() > 0.5
        s = np.where(flip, -s, s)
        need = (0.04 * a.sum() - float(np.sum(np.where(flip, -a, a)))) / 2.0
        for k in np.argsort(-a):
            if flip[k] and 0 < a[k] <= need:
                s[k], need = -s[k], need - a[k]
    x = np.zeros(n_out * D, np.int64)
    outs = []
    for o in range(so - 1, n_out, so):
        e = D * o + D - 1
        if e - (T - 1) < 0 or e >= x.size:
            continue
        x[e - np.arange(T)] = s * A
        outs.append(o)
    rest = np.ones(x.size, bool)
    for o in outs:
        rest[D * o + D - 1 - np.arange(T)] = False
    x[rest] = rng.integers(-A, A + 1, size=int(rest.sum()))
    return x, np.array(outs)


def _margin_capture(stages, A, rng, seg_out=4096):
    """four segments of seg_out outputs each: sign-aligned windows, cancelling windows, a full-scale alternating
    tone on I beside a stop-band tone on Q, random full-scale noise"""
    g, D = _folded(stages)
    a_i, _ = _aligned(g, D, A, seg_out, rng)
    c_i, _ = _aligned(g, D, A, seg_out, rng, cancel=True)
    t = np.arange(seg_out * D)
    alt_i = A * (1 - 2 * (t & 1))
    alt_q = np.round(A * np.cos(2 * np.pi * 0.4137 * t)).astype(np.int64)
    nz_i = rng.integers(-A, A + 1, size=seg_out * D)
    nz_q = rng.integers(-A, A + 1, size=seg_out * D)
    i = np.concatenate([a_i, c_i, alt_i, nz_i])
    q = np.concatenate([-a_i, rng.integers(-A, A + 1, size=seg_out * D), alt_q, nz_q])
    lim = 32767 if A > 2047 else 2047
    assert np.abs(i).max() <= lim and np.abs(q).max() <= lim
    return _iq(i.astype(np.int16), q.astype(np.int16)), ("aligned", "cancel", "tones", "noise"), seg_out


MARGIN_FILTERS = ["t32", "t64", "t128", "t256", "t255", "dec4", "dec4_3x5", "dec4_16x1", "dec4_1x32", "dec4_15x31"]


def _two_stage_taps(name):
    """(n1, n2) of a two-stage name: "dec4" is the family's largest shape, "dec4_3x5" has (3, 5) taps; None for any other name"""
    if not name.startswith("dec4"):
        return None
    return (16, 32) if name == "dec4" else tuple(int(v) for v in name[5:].split("x"))


def _margin_stages(name, kind, rng):
    if _two_stage_taps(name):
        n1, n2 = _two_stage_taps(name)
        return [(2, _taps(rng, n1, kind, 1.2)), (2, _taps(rng, n2, kind, 1.2))]
    return [(1, _taps(rng, int(name[1:]), kind))]


@pytest.mark.parametrize("kind", ["rand24", "exact22", "mixed"])
@pytest.mark.parametrize("name", MARGIN_FILTERS)
def test_error_bound_margin(ok, oracle, tmp_path, record_property, name, kind):
    """max |y_kernel - y_oracle| / bound per component over every output, matrix-core form (err_nominal for captures
    within [-2048, 2047], err_wide for captures whose every tile holds a wide sample) and packed-VALU form
    (err_valu), at sign-aligned, cancelling, tone and noise inputs: <= MARGIN"""
    forms = _front_forms(ok)
    rng = np.random.default_rng(zlib.crc32(("%s/%s" % (name, kind)).encode()))
    stages = _margin_stages(name, kind, rng)
    path = _write(tmp_path, "%s_%s" % (name, kind), stages)
    f = ok.Filter.load(path)
    of = oracle.load_filter_json(path)
    two = _two_stage_taps(name) is not None
    mfma = forms["mfma2"] if two else forms["mfma1"]
    valu = forms["fir2"] if two else forms["fir1"]
    worst = {}
    for amp, A in (("nominal", 2047), ("wide", 32767)):
        iq, segs, seg_out = _margin_capture(stages, A, rng)
        n = iq.size // 2
        want = oracle.rx(iq, of, 0.1, None, 8192, want_bits=True, want_fir=True)
        g, D = _folded(stages)
        if not two:
            # the construction does what it says: the aligned outputs reach sum|h| A
            y64 = _sum64(iq, g, D)
            assert np.abs(y64.real[:seg_out]).max() >= 0.999 * np.abs(g).sum() * A / 2048.0
        else:
            y64 = _sum64(iq, g, D)
            assert np.abs(y64.real[:seg_out]).max() >= 0.99 * np.abs(g).sum() * A / 2048.0
            assert np.abs(y64 - (want.fir[:, 0] + 1j * want.fir[:, 1])).max() <= 1e-4 * np.abs(g).sum() * A / 2048.0
        for valu_leg in (False, True):
            rx = ok.Receiver(f, None, max_samples=n, edge_capacity=n + 64, keep_fir=True, fir_valu=valu_leg)
            info = rx.front_info()
            got = rx.rx(iq)
            assert got.stats["front_form"] == (valu if valu_leg else mfma)
            assert (rx.bits() == want.bits).all(), (amp, valu_leg)
            err = info["err_valu"] if valu_leg else info["err_wide" if amp == "wide" else "err_nominal"]
            assert err > 0
            if not valu_leg and kind == "exact22" and not two:
                assert info["mfma_delta"] == 0.0
            if not valu_leg and kind == "rand24":
                assert info["mfma_delta"] > 0.0
            d = np.abs(rx.fir_output().astype(np.float64) - want.fir.astype(np.float64)) / err
            for k, seg in enumerate(segs):
                key = "%s_%s_%s" % ("valu" if valu_leg else "mfma", amp, seg)
                worst[key] = float(d[k * seg_out:(k + 1) * seg_out].max())
            rx.close()
    for key, r in sorted(worst.items()):
        record_property(key, r)
    print("worst |y - y_ref| / bound", name, kind, json.dumps(worst))
    bad = {k: r for k, r in worst.items() if r > 1.0}
    assert not bad, "error beyond the bound: the guard band is unsound %s" % bad
    thin = {k: r for k, r in worst.items() if r > MARGIN}
    assert not thin, "error within a factor %.1f of the bound %s" % (1.0 / MARGIN, thin)


# -------------------------------------------------------------- bits where it is tight ----

def _tight_capture(stages, err, A, n_out, rng):
    """cancelling windows (partial sums at full scale) whose outputs all land within ~err of one magnitude: the
    window sample at the smallest non-zero tap moves by a random few LSB.  Returns the capture and a threshold at
    the median of those outputs."""
    g, D = _folded(stages)
    x, outs = _aligned(g, D, A, n_out, rng, cancel=True)
    nz = np.nonzero(np.abs(g) > np.abs(g).max() * 2.0 ** -12)[0]
    kp = int(nz[np.argmin(np.abs(g[nz]))])
    step = abs(g[kp]) / 2048.0
    r = int(min(max(1, np.ceil(2.0 * err / step)), A // 8))
    x = x.copy()
    d = rng.integers(-r, r + 1, size=outs.size)
    idx = D * outs + D - 1 - kp
    x[idx] = np.sign(x[idx]) * (np.abs(x[idx]) - r) + d         # stays within [-A, A]
    q = np.zeros_like(x)
    iq = _iq(x.astype(np.int16), q.astype(np.int16))
    y = np.abs(_sum64(iq, g, D))[outs]
    return iq, float(np.float32(np.median(y))), y


@pytest.mark.parametrize("amp", ["nominal", "wide"])
@pytest.mark.parametrize("name", ["fs32_fs4", "sinc255", "fs128_fs16_dec4", "dec4_3x5", "dec4_1x32"])
def test_tight_bits_at_threshold(ok, oracle, tmp_path, name, amp):
    """Full-scale partial sums that cancel to an output at the threshold, thousands of times: bits and edges are the
    oracle's, the matrix-core form ran, and every output the bound cannot place went through the exact recompute --
    the band is as wide as the bound it is built from (the kernels' errors are far inside it, so a band built from a
    fraction of the bound could still give the right bits here, but not the right count)."""
    forms = _front_forms(ok)
    if name == "sinc255":
        k = np.arange(255) - 127
        h = np.sinc(k / 32.0) * np.hamming(255)
        stages = [(1, (h / h.sum()).astype(np.float32))]
        path = _write(tmp_path, name, stages)
    elif _two_stage_taps(name):
        stages = _margin_stages(name, "rand24", np.random.default_rng(sum(_two_stage_taps(name))))
        path = _write(tmp_path, name, stages)
    else:
        stages = _golden_stages(oracle, name)
        path = golden_path("filters", name)
    f = ok.Filter.load(path)
    of = oracle.load_filter_json(path)
    A = 32767 if amp == "wide" else 2047
    rng = np.random.default_rng(23)
    probe = ok.Receiver(f, None, max_samples=1, threshold=0.1)
    err = probe.front_info()["err_wide" if amp == "wide" else "err_nominal"]
    probe.close()
    g, D = _folded(stages)
    n_out = min(600000, 5000 * (-(-g.size // D) + 1))
    iq, thr, y = _tight_capture(stages, err, A, n_out, rng)
    assert (np.abs(y - thr) <= 3 * err).mean() > 0.5                 # the planted outputs sit inside the band
    n = iq.size // 2
    want = oracle.rx(iq, of, thr, None, 8192, want_bits=True, want_fir=True)
    assert 0.05 < want.bits.mean() < 0.95
    mag = np.hypot(want.fir[:, 0].astype(np.float64), want.fir[:, 1].astype(np.float64))
    for valu in ((False, True) if name == "fs32_fs4" and amp == "nominal" else (False,)):
        rx = ok.Receiver(f, None, max_samples=n, threshold=thr, edge_capacity=n + 64, fir_valu=valu)
        got = rx.rx(iq)
        mfma = forms["mfma2"] if D == 4 else forms["mfma1"]
        valu_form = forms["fir2"] if D == 4 else forms["fir1"]
        assert got.stats["front_form"] == (valu_form if valu else mfma)
        bits = rx.bits()
        diff = np.nonzero(bits != want.bits)[0]
        assert diff.size == 0, "first differing bits at %s (valu=%s)" % (diff[:5], valu)
        assert list(rx.edges()) == list(edges_of(want.bits))
        # an output within the bound of the threshold is inside the band [p_lo, p_hi) (which reaches ~1.5 x the bound
        # to either side in magnitude), whatever the kernel's error as long as it keeps the measured margin
        band_err = rx.front_info()["err_valu" if valu else ("err_wide" if amp == "wide" else "err_nominal")]
        must = int(np.count_nonzero(np.abs(mag - thr) <= band_err))
        assert must > 100
        assert got.stats["guard_recomputes"] >= must, (got.stats["guard_recomputes"], must)
        rx.close()


# ------------------------------------------------------------------ wide sample placement ----

def _spiky_taps(rng, n):
    """random taps with the first four large: a sample's weight in the outputs right after it is big enough that
    reading it as one fp16 number (off by up to 8 LSB) moves them far beyond the nominal band"""
    h = rng.normal(0, 1, n)
    h = h / np.abs(h).sum() * 0.5
    h[:4] = [0.5, -0.45, 0.4, -0.35]
    return h.astype(np.float32)


def _placements(n):
    b = 3 * TILE_IN
    return {"history_only_2": b - 2, "history_only_1": b - 1, "tile_first": b, "tile_last": b + TILE_IN - 1,
            "first_tile": 2, "last_partial_tile": n - 3}


@pytest.mark.parametrize("wide_value", [32760, -32760])
@pytest.mark.parametrize("name", ["t32", "t255", "fs128_fs16_dec4", "dec4_3x5"])
def test_wide_sample_placement(ok, oracle, tmp_path, name, wide_value):
    """One wide sample (beyond +-2048, low five bits non-zero) in an otherwise nominal loud capture, placed in the
    history of the next tile only, at a tile's first / last sample, in the first and in the last (partial) tile: the
    tiles whose window holds it take two sample pieces.  Floats within MARGIN of err_wide; bits of the outputs it
    weighs most in are the oracle's with the threshold just above and just below them."""
    forms = _front_forms(ok)
    rng = np.random.default_rng(abs(wide_value) + len(name))
    if name == "fs128_fs16_dec4":
        stages = _golden_stages(oracle, name)
        path = golden_path("filters", name)
        want_form = forms["mfma2"]
    elif _two_stage_taps(name):
        # (large leading taps in both stages, as _spiky_taps: the folded filter's first taps weigh a sample heavily)
        n1, n2 = _two_stage_taps(name)
        stages = [(2, _spiky_taps(rng, 4 + n1)[:n1]), (2, _spiky_taps(rng, 4 + n2)[:n2])]
        path = _write(tmp_path, name, stages)
        want_form = forms["mfma2"]
    else:
        stages = [(1, _spiky_taps(rng, int(name[1:])))]
        path = _write(tmp_path, name, stages)
        want_form = forms["mfma1"]
    f = ok.Filter.load(path)
    of = oracle.load_filter_json(path)
    g, D = _folded(stages)
    n = 6 * TILE_IN + 300
    base = rng.integers(-1500, 1501, size=2 * n).astype(np.int16)
    # what reading the sample as one fp16 number would make of it
    as_half = int(np.float16(wide_value))
    assert as_half != wide_value and wide_value & 31
    for where, p in _placements(n).items():
        iq = base.copy()
        iq[2 * p] = wide_value
        shadow = iq.copy()
        shadow[2 * p] = max(-32768, min(32767, as_half))
        y = _sum64(iq, g, D)
        moved = np.abs(_sum64(shadow, g, D)) - np.abs(y)
        o = int(np.argmax(np.abs(moved)))
        y_ref = oracle.rx(iq, of, 0.0, None, 8192, want_fir=True).fir
        mag = float(np.hypot(float(y_ref[o, 0]), float(y_ref[o, 1])))
        for sgn in (1, -1):
            thr = float(np.float32(mag + sgn * abs(moved[o]) / 2))
            want = oracle.rx(iq, of, thr, None, 8192, want_bits=True, want_fir=True)
            rx = ok.Receiver(f, None, max_samples=n, threshold=thr, edge_capacity=n + 64, keep_fir=True)
            got = rx.rx(iq)
            assert got.stats["front_form"] == want_form
            bits = rx.bits()
            diff = np.nonzero(bits != want.bits)[0]
            assert diff.size == 0, "%s: first differing bits at %s (wide sample at %d, output %d)" % (where, diff[:5], p, o)
            err = rx.front_info()["err_wide"]
            r = float(np.abs(rx.fir_output().astype(np.float64) - want.fir.astype(np.float64)).max()) / err
            assert r <= MARGIN, (where, r)
            rx.close()


# ---- a live context agrees with the host-side plan ----------------------------------------------------------------
# one case of tests/golden/front_plan.json per OOKD_FRONT_* number (and carrier lists of 2 and 16)
LIVE_PLAN_CASES = ["none-none-thr0.1", "stages3-none-thr0.1", "fs32_fs4-fir_valu-thr0.1", "fs32_fs4-exact_fir-thr0.1",
                   "fs32_fs4-none-thr0.1", "fs128_fs16_dec4-fir_valu-thr0.1", "fs128_fs16_dec4-exact_fir-thr0.1",
                   "fs128_fs16_dec4-none-thr0.1", "none-cs8-thr0.1", "fs32_fs4-cs8-thr0.1", "fs128_fs16_dec4-cu8-thr0.1",
                   "stages3-none-thr0.1-nu0.25", "fs32_fs4-none-thr0.1-nu3000th", "fs32_fs4-none-thr0.1-car2",
                   "rand255-none-thr0.1-car16"]


def test_live_context_reports_what_the_plan_recorded(ok):
    """What a context reports about its front end -- front_info(), carrier_front_info(k) for every carrier, and the
    form its run launched -- is the recorded plan's, bit for bit: the context holds no numbers of its own."""
    from tests import front_plan_cases as P
    with open(P.GOLDEN_FILE) as f:
        golden = json.load(f)
    cases = P.cases()
    n = 8192
    rng = np.random.default_rng(21)
    iq = rng.integers(-40, 41, size=2 * n).astype(np.int16)
    iq[2 * 3000:2 * 3600] = 32767               # one full-scale burst
    forms = set()
    for cid in LIVE_PLAN_CASES:
        case, want = cases[cid], golden[cid]
        kw = P.receiver_kwargs(case)
        rx = ok.Receiver(P.make_filter(case["filter"]), None, max_samples=n, samples_per_buffer=4096, **kw)
        x = iq if kw["sample_format"] == "sc16q11" else (iq >> 8).astype(np.int8)
        rx.rx(x if kw["sample_format"] != "cu8" else (x.astype(np.int16) + 128).astype(np.uint8))
        assert P.info_entry(rx.front_info()) == want["info"][0], cid
        for k in range(rx.num_carriers):
            assert P.info_entry(rx.carrier_front_info(k)) == want["info"][k], (cid, k)
        assert rx.num_carriers == (len(case["carriers"]) if case["carriers"] else 0)
        assert rx.stats()["front_form"] == want["form"] == want["info"][0]["form"], cid
        forms.add(want["form"])
        rx.close()
    assert forms == set(range(ok.FRONT_NO_FILTER, ok.FRONT_TUNED_MULTI + 1))
