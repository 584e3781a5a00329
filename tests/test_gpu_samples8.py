"""8-bit IQ captures (CS8, CU8) through the fused front ends, on the GPU.

The expected values always come from `oracle.rx` on the capture widened to int16 (CS8 v -> 16 v, CU8 u ->
16 (u - 128)); in addition the library's own 16-bit run on that widened capture must give the same bits, edges,
messages, error samples, guard_recomputes and quiet_waves: an 8-bit run IS the 16-bit run on the widened capture.
"""
import json

import numpy as np
import pytest

from tests.helpers import golden_path, edges_of
from tests.test_samples8_host import FORMATS, RATE, as_format, cut8, golden8, widen

pytestmark = pytest.mark.gpu

FIR_RTOL = 1e-5


@pytest.fixture(scope="module")
def ok():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from ookiedokie_amd import build as okbuild
    okbuild.build()
    import ookiedokie_amd as okm
    okm.lib()
    return okm


# ---- filters ----------------------------------------------------------------------------------------------

def _write(tmp_path, name, stages):
    p = tmp_path / (name + ".json")
    p.write_text(json.dumps({"filter": {"stages": [{"decimation": int(d), "taps": [float(t) for t in taps]}
                                                   for d, taps in stages]}}))
    return str(p)


def _sinc(n, cut):
    k = np.arange(n) - (n - 1) / 2.0
    h = np.sinc(k / cut) * np.hamming(n)
    return (h / h.sum()).astype(np.float32)


# shape -> (filter, Receiver keywords, front_form of an 8-bit context, of a 16-bit context)
SHAPES = {
    "fs32_fs4": ("fs32_fs4", {}, 10, 5),
    "sinc255": ([(1, _sinc(255, 32.0))], {}, 10, 5),
    "t17": ([(1, _sinc(17, 4.0))], {}, 10, 5),
    "dec4": ("fs128_fs16_dec4", {}, 11, 8),
    "none": (None, {}, 9, 1),
    "valu": ("fs32_fs4", {"fir_valu": True}, 3, 3),
    "exact": ("fs32_fs4", {"exact_fir": True}, 4, 4),
    "t257": ([(1, _sinc(257, 32.0))], {}, 2, 2),
    "three_stage": ([(2, _sinc(9, 2.0)), (1, _sinc(5, 2.0)), (2, _sinc(7, 2.0))], {}, 2, 2),
}
FUSED = ("fs32_fs4", "sinc255", "t17", "dec4", "none")


def _filter(ok, oracle, tmp_path, shape):
    spec = SHAPES[shape][0]
    if spec is None:
        return None, None
    path = golden_path("filters", spec) if isinstance(spec, str) else _write(tmp_path, shape, spec)
    return ok.Filter.load(path), oracle.load_filter_json(path)


def _devices(ok, oracle, devname, dec):
    if devname is None:
        return None, None
    return (ok.Device.load(golden_path("devices", devname), RATE // dec),
            oracle.load_device_json(golden_path("devices", devname), RATE // dec)[0])


def _dev_ptr(x, offset_bytes=0):
    """the capture in device memory, `offset_bytes` past a 16-byte boundary; returns (tensor kept alive, pointer)"""
    import torch
    raw = np.frombuffer(np.ascontiguousarray(x).tobytes(), dtype=np.uint8)
    t = torch.zeros(raw.size + 64, dtype=torch.uint8, device="cuda")
    base = (-t.data_ptr()) % 16 + offset_bytes
    if raw.size:
        t[base:base + raw.size] = torch.from_numpy(raw.copy()).cuda()
    torch.cuda.synchronize()
    return t, t.data_ptr() + base


def _same_run(rx, got, want, tag):
    bits = rx.bits()
    assert bits.size == want.bits.size, tag
    diff = np.nonzero(bits != want.bits)[0]
    assert diff.size == 0, "%s: first differing bits at %s" % (tag, diff[:5])
    assert list(rx.edges()) == list(edges_of(want.bits)), tag
    assert list(got.msg_samples) == list(want.msg_samples), tag
    assert (got.payloads == want.payloads).all(), tag
    errs, nerr = rx.errors()
    assert nerr == len(want.err_samples), tag
    if nerr <= 32:
        assert list(errs) == list(want.err_samples), tag


def _parity(ok, oracle, tmp_path, x, fmt, shape, devname="p3l-nexa2012", thr=0.1, spb=8192, keep_fir=False,
            offset_bytes=0, **kw):
    """x: the capture in the format's own dtype.  The 8-bit context on x (device pointer), the 16-bit context on the
    widened capture, the oracle on the widened capture: all the same."""
    f, of = _filter(ok, oracle, tmp_path, shape)
    dec = of.total_decimation if of else 1
    d, od = _devices(ok, oracle, devname, dec)
    w = widen(x, fmt)
    n = x.size // 2
    args = dict(SHAPES[shape][1])
    args.update(kw)
    want = oracle.rx(w, of, thr, od, spb, want_bits=True, want_fir=keep_fir)
    rx8 = ok.Receiver(f, d, max_samples=max(n, 1), threshold=thr, samples_per_buffer=spb, keep_fir=keep_fir,
                      edge_capacity=n + 64, sample_format=fmt, **args)
    assert rx8.sample_bytes == 2 and rx8.front_info()["form"] == SHAPES[shape][2]
    keep, ptr = _dev_ptr(x, offset_bytes)
    got8 = rx8.rx_device(ptr, n)
    assert got8.stats["front_form"] == SHAPES[shape][2], (shape, got8.stats["front_form"])
    _same_run(rx8, got8, want, "%s %s 8-bit" % (fmt, shape))
    rx16 = ok.Receiver(f, d, max_samples=max(n, 1), threshold=thr, samples_per_buffer=spb, keep_fir=keep_fir,
                       edge_capacity=n + 64, **args)
    assert rx16.sample_bytes == 4
    got16 = rx16.rx(w)
    assert got16.stats["front_form"] == SHAPES[shape][3]
    _same_run(rx16, got16, want, "%s %s 16-bit" % (fmt, shape))
    for key in ("guard_recomputes", "quiet_waves", "num_edges", "decimated_samples", "input_samples"):
        assert got8.stats[key] == got16.stats[key], (key, got8.stats[key], got16.stats[key])
    if keep_fir and want.decimated:
        y = rx8.fir_output()
        if args.get("exact_fir") or of is None or SHAPES[shape][2] == 2:
            assert (y.view(np.uint32) == want.fir.view(np.uint32)).all(), "FIR floats not bit-identical"
        else:
            gain = 1.0
            for st in range(of.num_stages):
                gain *= max(1.0, float(np.abs(of.stage_taps(st)).sum()))
            scale = gain * float(np.abs(w.astype(np.int32)).max()) / 2048.0
            assert (np.abs(y - want.fir) <= FIR_RTOL * np.maximum(np.abs(want.fir), scale)).all()
    stats = (got8.stats, got16.stats)
    rx8.close()
    rx16.close()
    del keep
    return stats, want


def _random_bytes(n, seed):
    """uniform over the whole range, the extremes included and placed"""
    rng = np.random.default_rng(seed)
    v = rng.integers(-128, 128, size=2 * n).astype(np.int8)
    v[:8] = [-128, 127, 127, -128, -128, -128, 127, 127]
    return v


def _square(n, period=600):
    v = np.where((np.arange(n) // period) % 2 == 0, 127, -128).astype(np.int8)
    return np.stack([v, -1 - v], axis=1).reshape(-1).astype(np.int8)


# ---- forms and parity -------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", FORMATS)
def test_both_format_bits_are_refused(ok, fmt):
    import ctypes as C
    cfg = ok.RxConfig()
    cfg.flags = ok.RX_SAMPLES_CS8 | ok.RX_SAMPLES_CU8
    cfg.threshold = 0.1
    cfg.samples_per_buffer = 8192
    cfg.max_samples = 4096
    cfg.max_captures = 1
    assert not ok.lib().ookd_rx_create(C.byref(cfg), None, None)
    assert "CS8" in ok.last_error() and "CU8" in ok.last_error()


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("fmt", FORMATS)
def test_parity_golden_captures(ok, oracle, vectors, tmp_path, fmt, shape):
    """G1 and G2 at 8 bits, clean and with seeded noise; every shape; front_form as the dispatch table says"""
    long_form = shape in ("t257", "three_stage", "sinc255")
    for name, seed in (("G1", None), ("G1", 11), ("G2", None), ("G2", 12)):
        g, v8 = golden8(vectors, name, seed)
        if long_form:
            v8 = v8[:2 * 450000]                # (the first message of either; the oracle's long filters are slow)
        x = as_format(v8, fmt)
        stats, want = _parity(ok, oracle, tmp_path, x, fmt, shape, devname=g["device"], keep_fir=(seed is not None))
        if shape in ("fs32_fs4", "valu", "exact") and not long_form:
            assert len(want.msg_samples) == (3 if name == "G1" else 2)


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("fmt", FORMATS)
def test_parity_full_range_inputs(ok, oracle, tmp_path, fmt, shape):
    """uniformly random bytes over the full range (-128, 127 / 0, 255 included) and a full-scale square wave"""
    n = 150000
    for v8, thr in ((_random_bytes(n, 5), 0.4), (_square(n), 0.5)):
        x = as_format(v8, fmt)
        if fmt == "cu8":
            assert x.min() == 0 and x.max() == 255
        else:
            assert x.min() == -128 and x.max() == 127
        _parity(ok, oracle, tmp_path, x, fmt, shape, thr=thr, keep_fir=True)


# ---- edges of the window code -----------------------------------------------------------------------------

@pytest.mark.parametrize("shape,T", [("fs32_fs4", 32), ("dec4", 16), ("none", 1), ("sinc255", 255)])
@pytest.mark.parametrize("fmt", FORMATS)
def test_ragged_lengths(ok, oracle, tmp_path, fmt, shape, T):
    spb = 8192
    lengths = sorted({0, 1, max(T - 1, 1), T, 1023, 1024, 1025, spb - 1, spb + 1, 1048573})
    v_all = _random_bytes(1048573, 9)
    v_all[2 * 5000:2 * 300000] //= 16           # a quiet stretch, so quiet and loud tiles alternate
    for n in lengths:
        if shape == "sinc255" and n > 100000:
            continue
        x = as_format(v_all[:2 * n], fmt)
        _parity(ok, oracle, tmp_path, x, fmt, shape, devname=None, thr=0.3, spb=spb)


@pytest.mark.parametrize("offset", [2, 6, 14])
@pytest.mark.parametrize("shape", ["fs32_fs4", "dec4", "none", "valu"])
@pytest.mark.parametrize("fmt", FORMATS)
def test_unaligned_device_pointers(ok, oracle, tmp_path, fmt, shape, offset):
    x = as_format(_random_bytes(40000, 13), fmt)
    _parity(ok, oracle, tmp_path, x, fmt, shape, devname=None, thr=0.3, offset_bytes=offset)


@pytest.mark.parametrize("shape", ["fs32_fs4", "dec4", "none", "valu"])
@pytest.mark.parametrize("fmt", FORMATS)
def test_batched_captures_with_a_stride(ok, oracle, tmp_path, fmt, shape):
    n, stride, caps = 30000, 30000 + 1234, 3
    f, of = _filter(ok, oracle, tmp_path, shape)
    v = _random_bytes(stride * caps, 17)
    x = as_format(v, fmt)
    rx = ok.Receiver(f, None, max_samples=n, max_captures=caps, threshold=0.3, sample_format=fmt, **SHAPES[shape][1])
    keep, ptr = _dev_ptr(x)
    got = rx.rx_device(ptr, n, num_captures=caps, stride=stride)
    assert got.stats["front_form"] == SHAPES[shape][2]
    for c in range(caps):
        w = widen(x[2 * c * stride:2 * (c * stride + n)], fmt)
        want = oracle.rx(w, of, 0.3, None, 8192, want_bits=True)
        assert (rx.bits(c) == want.bits).all(), c
        assert list(rx.edges(c)) == list(edges_of(want.bits)), c
    rx.close()


@pytest.mark.parametrize("shape", ["fs32_fs4", "dec4", "none", "valu"])
def test_cu8_padding_reads_as_128(ok, oracle, tmp_path, shape):
    """n_valid short of the padded length: the pad is value 0 -- the byte 128 -- and sets no bit even at a threshold a
    pad of byte 0 (-2048) would be far above"""
    n, spb, thr = 3000, 8192, 0.05
    rng = np.random.default_rng(3)
    x = as_format(rng.integers(-3, 4, size=2 * n).astype(np.int8), "cu8")
    x[2 * 100:2 * 300] = 200                     # something loud, so the tiles are not skipped
    stats, want = _parity(ok, oracle, tmp_path, x, "cu8", shape, devname=None, thr=thr, spb=spb)
    dec = 4 if shape == "dec4" else 1
    assert want.decimated == spb // dec
    assert not want.bits[(n + 80) // dec:].any() and want.bits[:n // dec].any()
    assert stats[0]["num_edges"] == len(edges_of(want.bits))


# ---- guard band -------------------------------------------------------------------------------------------

def _folded(stages):
    if len(stages) == 1:
        return stages[0][1].astype(np.float64), 1
    (_, h1), (_, h2) = stages
    g = np.zeros(2 * (h2.size - 1) + h1.size)
    for k2 in range(h2.size):
        g[2 * k2:2 * k2 + h1.size] += float(h2[k2]) * h1.astype(np.float64)
    return g, 4


def _sum64(x, g, D):
    return np.convolve(x.astype(np.float64), g)[:x.size][D - 1::D] / 2048.0


def _aligned16(g, D, A, n_out, rng):
    """the cancelling windows of tests/test_gpu_front_bounds.py (_aligned, cancel=True), every sample a multiple of 16"""
    T = g.size
    so = -(-T // D) + 1
    s = np.sign(g)
    s[s == 0] = 1
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
    x[rest] = 16 * rng.integers(-A // 16, A // 16 + 1, size=int(rest.sum()))
    return x, np.array(outs)


def _tight_capture16(stages, err, n_out, rng):
    """_tight_capture of tests/test_gpu_front_bounds.py from multiples of 16: the sample at the smallest non-zero tap
    moves by a random few steps of 16 LSB.  Returns I samples (multiples of 16 within +-2032) and the threshold."""
    A = 2032
    g, D = _folded(stages)
    x, outs = _aligned16(g, D, A, n_out, rng)
    nz = np.nonzero(np.abs(g) > np.abs(g).max() * 2.0 ** -12)[0]
    kp = int(nz[np.argmin(np.abs(g[nz]))])
    step = abs(g[kp]) * 16.0 / 2048.0
    r = int(min(max(1, np.ceil(2.0 * err / step)), A // 16 // 8))
    d = rng.integers(-r, r + 1, size=outs.size)
    idx = D * outs + D - 1 - kp
    x[idx] = np.sign(x[idx]) * (np.abs(x[idx]) - 16 * r) + 16 * d
    assert np.abs(x).max() <= A and not (x % 16).any()
    y = np.abs(_sum64(x, g, D))[outs]
    return x, float(np.float32(np.median(y)))


GUARD_FILTERS = {"fs32_fs4": "fs32_fs4", "t64": [(1, _sinc(64, 8.0))], "t128": [(1, _sinc(128, 16.0))],
                 "sinc255": [(1, _sinc(255, 32.0))], "dec4": "fs128_fs16_dec4"}


@pytest.mark.parametrize("name", list(GUARD_FILTERS))
@pytest.mark.parametrize("fmt", FORMATS)
def test_guard_band_at_the_threshold(ok, oracle, tmp_path, record_property, fmt, name):
    """Thousands of cancelling windows whose envelope sits on the threshold: bits are the oracle's, outputs went through
    the exact recompute, and max |y - y_ref| / err_nominal stays far below 1 (the band's premise; the 16-bit kernels
    measure 1.1 % with 32 taps and at most 0.8 % with longer filters, and the 8-bit forms run the same product on the
    same fp16 window values, the factor 16 being in the sample and not folded into the scale)."""
    spec = GUARD_FILTERS[name]
    path = golden_path("filters", spec) if isinstance(spec, str) else _write(tmp_path, name, spec)
    f, of = ok.Filter.load(path), oracle.load_filter_json(path)
    stages = [(int(of.decimation[s]), of.stage_taps(s).astype(np.float32)) for s in range(of.num_stages)]
    g, D = _folded(stages)
    probe = ok.Receiver(f, None, max_samples=1, threshold=0.1, sample_format=fmt)
    info = probe.front_info()
    probe.close()
    err = info["err_nominal"]
    assert info["form"] == (11 if D == 4 else 10)
    rng = np.random.default_rng(29)
    n_out = min(400000, 4000 * (-(-g.size // D) + 1))
    xi, thr = _tight_capture16(stages, err, n_out, rng)
    v8 = np.stack([xi // 16, np.zeros_like(xi)], axis=1).reshape(-1).astype(np.int8)
    x = as_format(v8, fmt)
    w = widen(x, fmt)
    n = x.size // 2
    want = oracle.rx(w, of, thr, None, 8192, want_bits=True, want_fir=True)
    assert 0.05 < want.bits.mean() < 0.95
    rx = ok.Receiver(f, None, max_samples=n, threshold=thr, edge_capacity=n + 64, sample_format=fmt, keep_fir=True)
    keep, ptr = _dev_ptr(x)
    got = rx.rx_device(ptr, n)
    assert got.stats["front_form"] == info["form"]
    assert (rx.bits() == want.bits).all()
    assert list(rx.edges()) == list(edges_of(want.bits))
    mag = np.hypot(want.fir[:, 0].astype(np.float64), want.fir[:, 1].astype(np.float64))
    must = int(np.count_nonzero(np.abs(mag - thr) <= err))
    assert must > 100
    assert got.stats["guard_recomputes"] >= must > 0
    ratio = float(np.abs(rx.fir_output().astype(np.float64) - want.fir.astype(np.float64)).max() / err)
    record_property("err_ratio_%s_%s_ksteps%d" % (fmt, name, info["mfma_ksteps"]), ratio)
    print("guard band %s %s: K-steps %d, max |y - y_ref| / err_nominal = %.4f, recomputes %d (>= %d)"
          % (fmt, name, info["mfma_ksteps"], ratio, got.stats["guard_recomputes"], must))
    assert ratio < 1.0
    assert ratio < 0.10, "far above the 16-bit kernels' 1.1 %: the scale of the 8-bit conversion is off"
    rx.close()


# ---- quiet shortcut ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", ["fs32_fs4", "dec4"])
@pytest.mark.parametrize("fmt", FORMATS)
def test_quiet_shortcut_skips_what_the_16bit_run_skips(ok, oracle, vectors, tmp_path, fmt, shape):
    g, v8 = golden8(vectors, "G1", 31)
    x = as_format(v8, fmt)
    stats, want = _parity(ok, oracle, tmp_path, x, fmt, shape, count_quiet=True)
    assert stats[0]["quiet_waves"] > 0 and stats[0]["quiet_waves"] == stats[1]["quiet_waves"]
    assert stats[0]["front_form"] in (10, 11)
    stats_off, _ = _parity(ok, oracle, tmp_path, x, fmt, shape, count_quiet=True, quiet_skip=False)
    assert stats_off[0]["quiet_waves"] == 0


# ---- shards, chunks, host path ------------------------------------------------------------------------------

@pytest.mark.parametrize("nshards", [2, 3])
@pytest.mark.parametrize("shape", ["fs32_fs4", "dec4", "valu"])
@pytest.mark.parametrize("fmt", FORMATS)
def test_shards_with_8bit_halos_equal_the_whole_capture(ok, oracle, vectors, tmp_path, fmt, shape, nshards):
    g, v8 = golden8(vectors, "G1", 21)
    x = as_format(v8, fmt)
    f, of = _filter(ok, oracle, tmp_path, shape)
    dec = of.total_decimation
    d, od = _devices(ok, oracle, "p3l-nexa2012", dec)
    spb, n = 8192, x.size // 2
    want = oracle.rx(widen(x, fmt), of, 0.1, od, spb, want_bits=True)
    keep, ptr = _dev_ptr(x)
    args = SHAPES[shape][1]
    whole = ok.Receiver(f, d, max_samples=n, samples_per_buffer=spb, sample_format=fmt, **args)
    _, whole_state = whole.shard_begin(ptr, n, None, True, None)
    shard = -(-(n // spb) // nshards) * spb
    bounds = list(range(0, n, shard)) + [n]
    nsh = len(bounds) - 1
    assert nsh == nshards
    rxs, outs, ins = [], [None] * nsh, [None] * nsh
    for r in range(nsh):
        rx = ok.Receiver(f, d, max_samples=shard, samples_per_buffer=spb, sample_format=fmt, **args)
        H = rx.halo_samples
        lo, hi = bounds[r], bounds[r + 1]
        halo = x[2 * (lo - H):2 * lo] if r > 0 and H else None
        _, outs[r] = rx.shard_begin(ptr + 2 * lo, hi - lo, halo, r == nsh - 1, None)
        assert rx.stats()["front_form"] == SHAPES[shape][2]
        rxs.append(rx)
    for _round in range(nsh + 1):
        changed = False
        for r in range(1, nsh):
            if ins[r] is None or ins[r].key() != outs[r - 1].key():
                ins[r] = outs[r - 1]
                _, o = rxs[r].shard_refine(ins[r])
                changed = changed or o.key() != outs[r].key()
                outs[r] = o
        if not changed:
            break
    msgs, pays, off = [], [], 0
    for r in range(nsh):
        res = rxs[r]._result()
        msgs += [int(s) + off for s in res.msg_samples]
        pays += [bytes(p) for p in res.payloads]
        b = rxs[r].bits()
        assert (b == want.bits[off:off + b.size]).all(), r
        off += b.size
        rxs[r].close()
    assert off == want.decimated
    assert msgs == list(want.msg_samples) and len(msgs) == 3
    assert pays == [bytes(p) for p in want.payloads]
    assert outs[-1].key() == whole_state.key()
    whole.close()
    with pytest.raises(TypeError):
        rx = ok.Receiver(f, d, max_samples=shard, samples_per_buffer=spb, sample_format=fmt, **args)
        try:
            rx.shard_begin(ptr, shard, widen(x[:2 * rx.halo_samples], fmt), False, None)      # an int16 halo
        finally:
            rx.close()


@pytest.mark.parametrize("shape", ["fs32_fs4", "dec4", "none"])
@pytest.mark.parametrize("fmt", FORMATS)
def test_pipelined_and_host_runs(ok, oracle, vectors, tmp_path, fmt, shape):
    g, v8 = golden8(vectors, "G1", 41)
    x = as_format(v8, fmt)
    stats, want = _parity(ok, oracle, tmp_path, x, fmt, shape, pipeline_chunk_samples=4 * 8192)
    assert stats[0]["pipeline_chunks"] >= 2 and stats[0]["pipeline_chunks"] == stats[1]["pipeline_chunks"]
    f, of = _filter(ok, oracle, tmp_path, shape)
    dec = of.total_decimation if of else 1
    d, od = _devices(ok, oracle, "p3l-nexa2012", dec)
    rx = ok.Receiver(f, d, max_samples=x.size // 2, sample_format=fmt)
    got = rx.rx(x)                              # ookd_rx_process_host: 2 bytes per sample through the ingest pipeline
    assert got.stats["front_form"] == SHAPES[shape][2] and got.stats["pipeline_chunks"] == 0
    _same_run(rx, got, want, "host path")
    wrong = x.view(np.uint8 if fmt == "cs8" else np.int8)
    for bad in (wrong, widen(x, fmt), x.astype(np.float32)):
        with pytest.raises(TypeError):
            rx.rx(bad)
    rx.close()


# ---- file backend -----------------------------------------------------------------------------------------

def test_file_backend_reads_cu8_by_name(ok, oracle, vectors, tmp_path):
    g, v8 = golden8(vectors, "G1", 43)
    x = as_format(v8, "cu8")
    n = x.size // 2
    path = tmp_path / "x.CU8"                    # (case-insensitive)
    x.tofile(path)
    be = ok.HipFileBackend(str(path), samples_per_buffer=8192)
    assert be.sample_flags == ok.RX_SAMPLES_CU8 and be.sample_format == "cu8"
    chunks, status = [], 0
    while status == 0:
        status, y = be.rx(8192)
        if status == 0:
            chunks.append(y)
    assert status == ok.FILE_EOF
    y = np.concatenate(chunks)
    assert y.shape[0] == -(-n // 8192) * 8192       # short final read padded
    want = ((x.astype(np.float32) - np.float32(128.0)) / np.float32(128.0)).reshape(-1, 2)
    assert (y[:n].view(np.uint32) == want.view(np.uint32)).all()
    assert (y[:n].view(np.uint32) == oracle.unpack(widen(x, "cu8")).view(np.uint32)).all()
    assert not y[n:].any()                          # ... with the format's zero, not the byte 0
    ptr, cn = be.capture()
    assert cn == n and ptr
    f, of = _filter(ok, oracle, tmp_path, "fs32_fs4")
    d, od = _devices(ok, oracle, "p3l-nexa2012", 1)
    rx = ok.Receiver(f, d, max_samples=n, sample_format=be.sample_format)
    got = rx.rx_device(ptr, n)
    assert got.stats["front_form"] == 10
    wantr = oracle.rx(widen(x, "cu8"), of, 0.1, od, 8192, want_bits=True)
    _same_run(rx, got, wantr, "file capture")
    assert len(got.msg_samples) == 3
    assert all(got.payload_bits(i, 36) == g["survey"]["payload_bits"] for i in range(3))
    rx.close()
    be.close()
    # the same bytes under another name are SC16Q11: half as many samples
    other = tmp_path / "x.bin"
    x.tofile(other)
    be = ok.HipFileBackend(str(other), samples_per_buffer=8192)
    assert be.sample_flags == 0 and be.sample_format == "sc16q11"
    _, cn = be.capture()
    assert cn == n // 2
    status, y = be.rx(4)
    assert status == 0 and (y.view(np.uint32) == oracle.unpack(x.view(np.int16)[:8]).view(np.uint32)).all()
    be.close()
    cs = tmp_path / "y.cs8"
    as_format(v8, "cs8").tofile(cs)
    be = ok.HipFileBackend(str(cs), samples_per_buffer=8192)
    assert be.sample_flags == ok.RX_SAMPLES_CS8
    status, y = be.rx(8192)
    assert status == 0 and (y.view(np.uint32) == (v8[:2 * 8192].astype(np.float32) / np.float32(128.0)).reshape(-1, 2).view(np.uint32)).all()
    be.close()


# ---- no widened copy on the fused path ----------------------------------------------------------------------

def _held(ok, f, max_samples, ptr, n, **kw):
    """device memory a context holds: (after create, after its first run), in bytes"""
    import torch
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    rx = ok.Receiver(f, None, max_samples=max_samples, **kw)
    torch.cuda.synchronize()
    created = free0 - torch.cuda.mem_get_info()[0]
    rx.process_device(ptr, n)
    torch.cuda.synchronize()
    ran = free0 - torch.cuda.mem_get_info()[0]
    form = rx.stats()["front_form"]
    rx.close()
    return created, ran, form


@pytest.mark.parametrize("fmt", FORMATS)
def test_fused_forms_hold_no_widened_copy(ok, oracle, tmp_path, fmt):
    """8-bit minus 16-bit context memory is the same at max_samples 2^24 and 2^28 (a staging copy would be 4 B x the
    difference in samples, about 1 GiB); with fir_valu it IS there, and only after the first run (lazy)."""
    f, _ = _filter(ok, oracle, tmp_path, "fs32_fs4")
    n = 8192
    x = as_format(_random_bytes(n, 3), fmt)
    k8, p8 = _dev_ptr(x)
    k16, p16 = _dev_ptr(widen(x, fmt))
    MiB = 1 << 20
    extra = {}
    for valu in (False, True):
        for ms in (1 << 24, 1 << 28):
            c8, r8, form8 = _held(ok, f, ms, p8, n, sample_format=fmt, fir_valu=valu)
            c16, r16, form16 = _held(ok, f, ms, p16, n, fir_valu=valu)
            assert (form8, form16) == ((3, 3) if valu else (10, 5))
            extra[(valu, ms)] = (c8 - c16, r8 - r16)
            print("context memory %s valu=%s max_samples=2^%d: 8-bit - 16-bit = %.1f MiB at create, %.1f MiB after a run"
                  % (fmt, valu, ms.bit_length() - 1, (c8 - c16) / MiB, (r8 - r16) / MiB))
    assert abs(extra[(False, 1 << 28)][1] - extra[(False, 1 << 24)][1]) <= 4 * MiB
    assert abs(extra[(False, 1 << 28)][0] - extra[(False, 1 << 24)][0]) <= 4 * MiB
    # the packed-VALU form of an 8-bit context runs behind the widening kernel: 4 B per sample of max_samples,
    # allocated by the first run, not at create time
    assert abs(extra[(True, 1 << 28)][0] - extra[(True, 1 << 24)][0]) <= 4 * MiB
    grow = extra[(True, 1 << 28)][1] - extra[(True, 1 << 24)][1]
    assert abs(grow - 4 * ((1 << 28) - (1 << 24))) <= 8 * MiB, grow / MiB
