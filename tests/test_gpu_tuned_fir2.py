"""The fused tuned front end for two decimate-by-2 stages on the GPU (OOKD_RX_TUNED_FIR2 -> OOKD_FRONT_TUNED_FIR2,
fir2_tuned_kernel in fir_tuned.hip).  Expected bits and floats come from the numpy restatement of the contract
(tests/tuned_contract.py) fed with the library's own taps; the quiet shortcut's count from the documented rule
(tests/tuned_fir2_inputs.py).  Every context is created with `tuned_fir2=True` unless a test says otherwise."""
import json
import zlib

import numpy as np
import pytest

from tests import tuned_bounds_inputs as B
from tests import tuned_fir2_inputs as T2
from tests.helpers import edges_of, golden_path
from tests.tuned_contract import RATE, SPB, THR, contract_rx, golden_capture, lib_stages, moved, to_8bit

pytestmark = pytest.mark.gpu

MARGIN = 0.5                    # the project's margin for every fused form (tests/test_gpu_front_bounds.py)


@pytest.fixture(scope="module")
def ok():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from ookiedokie_amd import build as okbuild
    okbuild.build()
    import ookiedokie_amd as okm
    okm.lib()
    return okm


def _dec4(ok):
    return ok.Filter.load(golden_path("filters", "fs128_fs16_dec4"))


_CONTRACT = {}


def _contract(key, iq, f, nu, thr, spb=SPB):
    """contract_rx with the library's taps, computed once per key and never changed"""
    k = (key, float(nu), float(thr), spb)
    if k not in _CONTRACT:
        bits, y = contract_rx(iq, lib_stages(f, nu), thr, spb)
        bits.setflags(write=False)
        y.setflags(write=False)
        _CONTRACT[k] = (bits, y)
    return _CONTRACT[k]


def _check_bits(rx, k, bits, what=""):
    edges = list(rx.edges(k))
    b = rx.bits(k)
    assert b.size == bits.size
    diff = np.nonzero(b != bits)[0]
    assert diff.size == 0, "result %d %s: first differing bits at %s" % (k, what, diff[:5])
    assert edges == list(edges_of(bits)), (k, what)


def _worst(rx, k, y, err):
    return float(np.abs(rx.fir_output(k).astype(np.float64) - y.astype(np.float64)).max() / err)


def _tiles(n, spb, results=1):
    """256-output tiles of a run, per result"""
    n_pad = -(-n // spb) * spb
    return results * -(-(n_pad // 4) // T2.F)


# ------------------------------------------------------------------------------- 1. parity ----

@pytest.mark.parametrize("nu", T2.NUS, ids=T2.NU_IDS)
@pytest.mark.parametrize("cap", ["G1", "G2"])
def test_parity_with_the_contract(ok, record_property, cap, nu):
    """form 15 on a golden capture moved to nu with DC and noise: bits and edges the contract's, floats within err_valu
    per component; the same context without the flag runs form 12 and gives the same bits"""
    _, iq, _ = T2.moved_golden(cap, nu)
    f = _dec4(ok)
    n = iq.size // 2
    bits, y = _contract(("parity", cap), iq, f, nu, THR)
    rx = ok.Receiver(f, None, max_samples=n, edge_capacity=n + 64, keep_fir=True, tune=nu, tuned_fir2=True)
    info = rx.front_info()
    assert info["form"] == ok.FRONT_TUNED_FIR2
    got = rx.rx(iq)
    assert got.stats["front_form"] == ok.FRONT_TUNED_FIR2
    assert got.stats["total_waves"] == _tiles(n, SPB) and got.stats["quiet_waves"] == 0
    _check_bits(rx, 0, bits, "form 15")
    assert info["err_valu"] > 0 and info["p_lo"] < info["p_star"] < info["p_hi"]
    worst = _worst(rx, 0, y, info["err_valu"])
    record_property("worst_over_err_valu", worst)
    print("worst |y - y_contract| / err_valu", cap, nu, worst)
    assert worst <= 1.0
    rx.close()
    rx = ok.Receiver(f, None, max_samples=n, edge_capacity=n + 64, keep_fir=True, tune=nu)
    assert rx.front_info()["form"] == ok.FRONT_TUNED_GENERIC
    got = rx.rx(iq)
    assert got.stats["front_form"] == ok.FRONT_TUNED_GENERIC
    _check_bits(rx, 0, bits, "form 12")
    assert (rx.fir_output().view(np.uint32) == y.view(np.uint32)).all()
    rx.close()


# ------------------------------------------------------------------------------ 2. recovery ----

@pytest.mark.parametrize("nu", [0.2, -0.3], ids=["p0.2", "m0.3"])
@pytest.mark.parametrize("cap", ["G1", "G2"])
def test_recovery_of_an_off_centre_carrier(ok, oracle, cap, nu):
    """payloads and message sample indices of the flagged decode are the oracle's on the capture that was never moved"""
    base, iq, g = T2.moved_golden(cap, nu)
    n = iq.size // 2
    f = _dec4(ok)
    rate = RATE // f.total_decimation
    d = ok.Device.load(golden_path("devices", g["device"]), rate)
    od = oracle.load_device_json(golden_path("devices", g["device"]), rate)[0]
    want = oracle.rx(base, oracle.load_filter_json(golden_path("filters", "fs128_fs16_dec4")), THR, od, SPB)
    assert len(want.msg_samples) > 0
    rx = ok.Receiver(f, d, max_samples=n, tune=nu, tuned_fir2=True)
    got = rx.rx(iq)
    assert got.stats["front_form"] == ok.FRONT_TUNED_FIR2
    assert list(got.msg_samples) == list(want.msg_samples)
    assert (got.payloads == want.payloads).all()
    _check_bits(rx, 0, _contract(("parity", cap), iq, f, nu, THR)[0])
    rx.close()


# ------------------------------------------------------------------------ 3. quiet shortcut ----

@pytest.mark.parametrize("dense", [False, True], ids=["sparse", "dense"])
@pytest.mark.parametrize("nu", [0.2, -0.3, 1.0 / 3000.0], ids=["p0.2", "m0.3", "1_3000"])
def test_quiet_shortcut(ok, monkeypatch, nu, dense):
    """bits and edges identical with the shortcut on and off, sparse and dense output; quiet_waves is the count the
    documented rule gives on the CPU (evaluated in float32 as the kernel evaluates it: tests/test_tuned_fir2_host.py
    holds that form equal to the documented one on these captures).  Each context runs a loud capture first, so a
    word a quiet tile leaves behind shows."""
    if dense:
        monkeypatch.setenv("OOKD_DEVELOPER", "1")
        monkeypatch.setenv("OOKD_DENSE_BITS", "1")
    _, iq, _ = T2.moved_golden("G2", nu)
    f = _dec4(ok)
    n = iq.size // 2
    bits, _ = _contract(("parity", "G2"), iq, f, nu, THR)
    census = T2.quiet_census(iq, lib_stages(f, nu), THR, bits)
    loud = B.loud_capture(n)
    loud_bits, _ = _contract(("loud", n), loud, f, nu, THR)
    assert loud_bits.mean() > 0.5
    res = {}
    for quiet in (True, False):
        rx = ok.Receiver(f, None, max_samples=n, edge_capacity=n + 64, tune=nu, tuned_fir2=True, quiet_skip=quiet,
                         count_quiet=True)
        got = rx.rx(loud)
        assert got.stats["front_form"] == ok.FRONT_TUNED_FIR2 and got.stats["quiet_waves"] == 0
        _check_bits(rx, 0, loud_bits, "the loud run")
        got = rx.rx(iq)
        _check_bits(rx, 0, bits, "quiet_skip %s" % quiet)
        st = got.stats
        assert st["total_waves"] == _tiles(n, SPB)
        print("quiet tiles", nu, "dense" if dense else "sparse", quiet, st["quiet_waves"], "of", st["total_waves"], census)
        assert st["quiet_waves"] == (census["taken32"] if quiet else 0)
        if quiet:
            assert census["half"] <= st["quiet_waves"] <= census["zero"]
        res[quiet] = rx.bits().copy()
        rx.close()
    assert (res[True] == res[False]).all()
    assert census["bad"] == 0 and (census["taken32"] > 0) == (nu != 1.0 / 3000.0)


# -------------------------------------------------------------- 4. tile edges and tap shapes ----

EDGE_SPB = 1024
EDGE_N = 5 * EDGE_SPB + 300


@pytest.fixture(scope="module")
def edge_iq():
    """noise of +-1500 LSB with a stretch of +-30 LSB that holds whole tile windows"""
    rng = np.random.default_rng(41)
    x = rng.integers(-1500, 1501, size=2 * EDGE_N)
    x[2 * 900:2 * 3400] = rng.integers(-30, 31, size=2 * 2500)
    x = x.astype(np.int16)
    x.setflags(write=False)
    return x


@pytest.mark.parametrize("nu", [0.37, -0.5])
@pytest.mark.parametrize("shape", [(1, 1), (3, 5), (15, 31), (16, 32), (16, 1), (1, 32)], ids=lambda s: "%dx%d" % s)
def test_tile_edges_and_tap_shapes(ok, tmp_path, edge_iq, shape, nu):
    """a first tile whose window starts before the capture, interior tiles, a ragged last tile with zero padding;
    behind a host pointer, and behind a device pointer one sample past a 16-byte boundary (every tile takes the
    per-sample path)"""
    import torch
    n1, n2 = shape
    f = ok.Filter.load(B.write_filter(tmp_path, "s%dx%d" % shape, [(2, B.rand_taps(n1, 10 + n1)), (2, B.rand_taps(n2, 50 + n2))]))
    n, spb = EDGE_N, EDGE_SPB
    bits, y = _contract(("edge", shape), edge_iq, f, nu, THR, spb)
    assert bits.any() and not bits.all()
    dev_t = torch.zeros(2 * (n + 8), dtype=torch.int16, device="cuda")
    dev_t[2:2 + 2 * n] = torch.from_numpy(np.array(edge_iq)).cuda()
    assert (dev_t.data_ptr() + 4) % 16 == 4
    for keep in (True, False):
        rx = ok.Receiver(f, None, max_samples=n, samples_per_buffer=spb, edge_capacity=n + spb + 64, keep_fir=keep,
                         tune=nu, tuned_fir2=True, count_quiet=True)
        info = rx.front_info()
        assert info["form"] == ok.FRONT_TUNED_FIR2
        for where in ("host", "device + 4 bytes"):
            got = rx.rx(edge_iq) if where == "host" else rx.rx_device(dev_t.data_ptr() + 4, n)
            assert got.stats["front_form"] == ok.FRONT_TUNED_FIR2
            assert got.stats["total_waves"] == _tiles(n, spb)
            _check_bits(rx, 0, bits, "%s keep_fir %s" % (where, keep))
            if keep:
                assert _worst(rx, 0, y, info["err_valu"]) <= 1.0
            if keep or where != "host":
                assert got.stats["quiet_waves"] == 0        # floats wanted / no tile is interior behind such a pointer
            else:
                census = T2.quiet_census(edge_iq, lib_stages(f, nu), THR, bits)
                assert got.stats["quiet_waves"] == census["taken32"] and census["bad"] == 0
        rx.close()


# ---------------------------------------------------------------------------- 5. guard band ----

@pytest.mark.parametrize("shape", [(16, 32), (15, 31)], ids=lambda s: "%dx%d" % s)
def test_guard_band_at_the_threshold(ok, tmp_path, shape):
    """threshold at the median contract |y| of a noisy stretch: outputs inside the band are recomputed in the contract's
    order and the bits are exactly the contract's; exact_fir (form 12) on the same input as the cross-check"""
    n1, n2 = shape
    nu = 0.2
    f = ok.Filter.load(B.write_filter(tmp_path, "g%dx%d" % shape, [(2, B.rand_taps(n1, 3)), (2, B.rand_taps(n2, 4))]))
    n = 10 * 8192
    iq = np.random.default_rng(n1).integers(-1500, 1501, size=2 * n).astype(np.int16)
    _, y = _contract(("guard", shape), iq, f, nu, 1.0)
    mag = np.hypot(y[:, 0].astype(np.float64), y[:, 1].astype(np.float64))
    thr = float(np.float32(np.median(mag)))
    bits, _ = _contract(("guard", shape), iq, f, nu, thr)
    assert 0.4 < bits.mean() < 0.6
    rx = ok.Receiver(f, None, max_samples=n, threshold=thr, edge_capacity=n + 64, tune=nu, tuned_fir2=True)
    info = rx.front_info()
    got = rx.rx(iq)
    assert got.stats["front_form"] == ok.FRONT_TUNED_FIR2
    _check_bits(rx, 0, bits, "form 15")
    # every output the bound cannot place lies inside the band the bound was turned into
    must = int(np.count_nonzero(np.abs(mag - thr) <= info["err_valu"]))
    print("guard recomputes", shape, got.stats["guard_recomputes"], "must", must)
    assert must > 0 and got.stats["guard_recomputes"] >= must
    rx.close()
    rx = ok.Receiver(f, None, max_samples=n, threshold=thr, edge_capacity=n + 64, tune=nu, tuned_fir2=True, exact_fir=True)
    got = rx.rx(iq)
    assert got.stats["front_form"] == ok.FRONT_TUNED_GENERIC and got.stats["guard_recomputes"] == 0
    _check_bits(rx, 0, bits, "form 12")
    rx.close()


# --------------------------------------------------------------------------------- 6. bound ----

BOUND_SEG = 4096                # input samples per segment


def _bound_capture(nu, A, rng):
    """a full-scale tone at nu beside one at -nu, then full-scale noise; with A = 32767 some samples sit at -32768"""
    t = np.arange(BOUND_SEG, dtype=np.float64)
    ph = 2.0 * np.pi * ((nu * t) % 1.0)
    z = np.rint(0.7 * A * np.exp(1j * ph)) + np.rint(0.3 * A * np.exp(-1j * ph))
    tones = B.interleave(np.clip(z.real, -A, A) + 1j * np.clip(z.imag, -A, A))
    lo = -32768 if A == 32767 else -A
    nz = rng.integers(lo, A + 1, size=2 * BOUND_SEG)
    if A == 32767:
        tones = tones.copy()
        tones[tones == -32767] = -32768
        nz[rng.integers(0, nz.size, size=64)] = -32768
    return np.concatenate([tones, nz.astype(np.int16)])


@pytest.mark.parametrize("nu", T2.NUS, ids=T2.NU_IDS)
@pytest.mark.parametrize("shape", [(16, 32), (15, 31)], ids=lambda s: "%dx%d" % s)
def test_error_bound_margin(ok, tmp_path, record_property, shape, nu):
    """max |y_kernel - y_contract| / err_valu per component at full-scale tones and noise, nominal (2047) and wide
    (32767, with samples at -32768) amplitudes: <= 1.0 (tuned_guard_error's derivation over both stages) and
    <= MARGIN, the project's margin for every fused form"""
    n1, n2 = shape
    f = ok.Filter.load(B.write_filter(tmp_path, "b%dx%d" % shape, [(2, B.rand_taps(n1, 21)), (2, B.rand_taps(n2, 22))]))
    rng = np.random.default_rng(zlib.crc32(("%dx%d/%g" % (n1, n2, nu)).encode()))
    worst = {}
    for amp, A in (("nominal", 2047), ("wide", 32767)):
        iq = _bound_capture(nu, A, rng)
        if amp == "wide":
            assert iq.min() == -32768
        n = iq.size // 2
        bits, y = _contract(("bound", shape, amp), iq, f, nu, THR, 4096)
        rx = ok.Receiver(f, None, max_samples=n, samples_per_buffer=4096, edge_capacity=n + 64, keep_fir=True, tune=nu,
                         tuned_fir2=True)
        err = rx.front_info()["err_valu"]
        got = rx.rx(iq)
        assert got.stats["front_form"] == ok.FRONT_TUNED_FIR2 and err > 0
        _check_bits(rx, 0, bits, amp)
        d = np.abs(rx.fir_output().astype(np.float64) - y.astype(np.float64)).max(axis=1) / err
        seg = BOUND_SEG // 4
        worst["%s_tones" % amp] = float(d[:seg].max())
        worst["%s_noise" % amp] = float(d[seg:].max())
        rx.close()
    for key, r in sorted(worst.items()):
        record_property(key, r)
    print("worst |y - y_contract| / err_valu", shape, nu, json.dumps(worst))
    bad = {k: r for k, r in worst.items() if r > 1.0}
    assert not bad, "error beyond the bound: the guard band is unsound %s" % bad
    thin = {k: r for k, r in worst.items() if r > MARGIN}
    assert not thin, "error within a factor %.1f of the bound %s" % (1.0 / MARGIN, thin)


# ------------------------------------------------------------------------------ 7. carriers ----

def test_carriers_are_the_tuned_contexts(ok, oracle):
    """three carriers (two nu, one repeated with another threshold): form 15; carrier k's bit words, edges and messages
    are the single flagged tuned context's, quiet_waves is the sum"""
    base, g = golden_capture("G2")
    iq = (moved(base, 0.2, T2.DC, T2.NOISE, seed=7).astype(np.int32) + moved(base, -0.3, 0j, 0, seed=8, scale=0.5)).astype(np.int16)
    n = iq.size // 2
    f = _dec4(ok)
    d = ok.Device.load(golden_path("devices", g["device"]), RATE // f.total_decimation)
    cl = [(0.2, THR), (-0.3, THR), (0.2, 0.05)]
    single = []
    for nu, thr in cl:
        rx = ok.Receiver(f, d, max_samples=n, threshold=thr, edge_capacity=n + 64, tune=nu, tuned_fir2=True, count_quiet=True)
        got = rx.rx(iq)
        assert got.stats["front_form"] == ok.FRONT_TUNED_FIR2
        _check_bits(rx, 0, _contract(("carriers",), iq, f, nu, thr)[0], "tuned %g %g" % (nu, thr))
        single.append((rx.bits().copy(), list(rx.edges()), list(got.msg_samples), got.payloads.copy(), got.stats["quiet_waves"]))
        rx.close()
    assert len(single[0][2]) > 0 and len(single[1][2]) > 0
    rx = ok.Receiver(f, d, max_samples=n, edge_capacity=3 * (n + 64), carriers=cl, tuned_fir2=True, count_quiet=True)
    assert rx.num_carriers == 3
    for k in range(3):
        assert rx.carrier_front_info(k)["form"] == ok.FRONT_TUNED_FIR2
    got = rx.rx(iq)
    assert got.stats["front_form"] == ok.FRONT_TUNED_FIR2
    assert got.stats["total_waves"] == _tiles(n, SPB, 3)
    for k, (b, e, ms, pay, _) in enumerate(single):
        assert (rx.bits(k) == b).all(), k
        assert list(rx.edges(k)) == e, k
        r = got.for_capture(k)
        assert list(r.msg_samples) == ms and (r.payloads == pay).all(), k
    assert got.stats["quiet_waves"] == sum(s[4] for s in single) > 0
    rx.close()
    # without the flag: the generic form, the same bits
    rx = ok.Receiver(f, d, max_samples=n, edge_capacity=3 * (n + 64), carriers=cl)
    got = rx.rx(iq)
    assert got.stats["front_form"] == ok.FRONT_TUNED_GENERIC
    for k, s in enumerate(single):
        assert (rx.bits(k) == s[0]).all(), k
    rx.close()


# --------------------------------------------------------------------------------- 8. 8-bit ----

@pytest.mark.parametrize("carriers", [False, True], ids=["tuned", "carriers"])
@pytest.mark.parametrize("fmt", ["cs8", "cu8"])
def test_8bit_captures_are_widened_once(ok, fmt, carriers):
    nu = 0.2
    _, iq, _ = T2.moved_golden("G2", nu)
    raw, wide = to_8bit(iq, fmt)
    n = wide.size // 2
    f = _dec4(ok)
    cl = [(nu, THR), (-0.3, 0.05)] if carriers else [(nu, THR)]
    kw = dict(carriers=cl) if carriers else dict(tune=nu)
    rx = ok.Receiver(f, None, max_samples=n, edge_capacity=len(cl) * (n + 64), sample_format=fmt, tuned_fir2=True, **kw)
    assert rx.front_info()["form"] == ok.FRONT_TUNED_FIR2
    for _ in range(2):
        got = rx.rx(raw)
        assert got.stats["front_form"] == ok.FRONT_TUNED_FIR2
        for k, (cnu, cthr) in enumerate(cl):
            _check_bits(rx, k, _contract(("8bit", fmt), wide, f, cnu, cthr)[0], fmt)
    rx.close()


# ----------------------------------------------------------------------------- 9. structure ----

def test_batch_of_two_captures(ok, oracle):
    import torch
    base, g = golden_capture("G2")
    nu = -0.3
    f = _dec4(ok)
    n = base.size // 2
    stride = n + 1000
    host = np.zeros((2, 2 * stride), np.int16)
    for c in range(2):
        host[c, :2 * n] = moved(base, nu, T2.DC, T2.NOISE, seed=90 + c)
    dev_t = torch.from_numpy(host).cuda()
    rx = ok.Receiver(f, None, max_samples=n, max_captures=2, edge_capacity=2 * (n + 64), tune=nu, tuned_fir2=True,
                     count_quiet=True)
    got = rx.rx_device(dev_t.data_ptr(), n, num_captures=2, stride=stride)
    assert got.stats["front_form"] == ok.FRONT_TUNED_FIR2 and got.stats["total_waves"] == _tiles(n, SPB, 2)
    quiet = 0
    for c in range(2):
        bits, _ = _contract(("batch", c), host[c, :2 * n], f, nu, THR)
        _check_bits(rx, c, bits, "capture %d" % c)
        quiet += T2.quiet_census(host[c, :2 * n], lib_stages(f, nu), THR, bits)["taken32"]
    assert got.stats["quiet_waves"] == quiet > 0
    rx.close()


def test_two_shards_with_halo_equal_the_whole_capture(ok, oracle):
    import torch
    base, iq, g = T2.moved_golden("G2", 0.2)
    nu = 0.2
    f = _dec4(ok)
    n = iq.size // 2
    rate = RATE // f.total_decimation
    d = ok.Device.load(golden_path("devices", g["device"]), rate)
    bits_w, _ = _contract(("parity", "G2"), iq, f, nu, THR)
    rx = ok.Receiver(f, d, max_samples=n, tune=nu, tuned_fir2=True)
    whole = rx.rx(iq)
    assert len(whole.msg_samples) > 0
    rx.close()
    dev_t = torch.from_numpy(iq).cuda()
    half = (n // 2) // SPB * SPB                            # a multiple of lcm(samples_per_buffer, 4)
    state, msgs, pays = None, [], []
    for r, (lo, hi) in enumerate(((0, half), (half, n))):
        rx = ok.Receiver(f, d, max_samples=n, tune=nu, tuned_fir2=True)
        H = rx.halo_samples
        assert H == 15 + 2 * 31
        halo = iq[2 * (lo - H):2 * lo] if r else None
        res, state = rx.shard_begin(dev_t.data_ptr() + 4 * lo, hi - lo, halo, r == 1, state)
        assert res.stats["front_form"] == ok.FRONT_TUNED_FIR2
        b = rx.bits()
        assert (b == bits_w[lo // 4:lo // 4 + b.size]).all(), r
        msgs += [int(s) + lo // 4 for s in res.msg_samples]
        pays += [bytes(x) for x in res.payloads]
        rx.close()
    assert msgs == [int(s) for s in whole.msg_samples]
    assert pays == [bytes(x) for x in whole.payloads]


@pytest.mark.parametrize("n", [B.SPLIT_N, 8 * 65536 + 777], ids=["5x65536", "8x65536"])
def test_split_launches(ok, monkeypatch, n):
    """OOKD_FRONT_LAUNCH_LOG2=16 (launches of 65536 outputs = 256 tiles; a run of up to 384 tiles stays one launch):
    the result equals that of a context without the variable, for the tuned context and for the carrier context.
    5 * 65536 + 777 samples are 336 tiles behind the decimation by 4 and still go out as one launch; 8 * 65536 + 777
    are 528 tiles in three launches (tile_base, tile_begin / tile_count)."""
    nu = 0.2
    tiles = -(-(-(-n // SPB) * SPB // 4) // 4096) * 16
    assert tiles == (336 if n == B.SPLIT_N else 528)
    g1, _ = golden_capture("G1")
    iq = moved(B.tiled(g1, n), nu, T2.DC, T2.NOISE, seed=51)
    f = _dec4(ok)
    cl = [(nu, THR), (-0.3, 0.05)]
    want = [_contract(("split", n), iq, f, cnu, cthr)[0] for cnu, cthr in cl]
    assert want[0].any() and not want[0].all()
    monkeypatch.delenv("OOKD_FRONT_LAUNCH_LOG2", raising=False)
    for kw, k_n in ((dict(tune=nu), 1), (dict(carriers=cl), 2)):
        runs = []
        for split in (False, True):
            if split:
                monkeypatch.setenv("OOKD_DEVELOPER", "1")
                monkeypatch.setenv("OOKD_FRONT_LAUNCH_LOG2", "16")
            else:
                monkeypatch.delenv("OOKD_FRONT_LAUNCH_LOG2", raising=False)
            rx = ok.Receiver(f, None, max_samples=n, edge_capacity=k_n * (n + 8192 + 64), tuned_fir2=True, count_quiet=True, **kw)
            got = rx.rx(iq)
            assert got.stats["front_form"] == ok.FRONT_TUNED_FIR2
            assert got.stats["front_launches"] == (3 if split and tiles > 384 else 1)
            for j in range(k_n):
                _check_bits(rx, j, want[j], "split %s" % split)
            runs.append(([list(rx.edges(j)) for j in range(k_n)], got.stats["quiet_waves"], got.stats["total_waves"]))
            rx.close()
        assert runs[0] == runs[1]
        assert 0 < runs[1][1] < runs[1][2]


def test_pulse_hist_is_that_of_the_unflagged_run(ok):
    _, iq, _ = T2.moved_golden("G2", 0.2)
    n = iq.size // 2
    f = _dec4(ok)
    hists = []
    for flag in (True, False):
        rx = ok.Receiver(f, None, max_samples=n, edge_capacity=n + 64, tune=0.2, tuned_fir2=flag)
        got = rx.rx(iq)
        assert got.stats["front_form"] == (ok.FRONT_TUNED_FIR2 if flag else ok.FRONT_TUNED_GENERIC)
        hists.append(rx.pulse_hist(0))
        rx.close()
    assert hists[0]["num_edges"] > 0 and sorted(hists[0]) == sorted(hists[1])
    for key in hists[0]:
        assert np.array_equal(np.asarray(hists[0][key]), np.asarray(hists[1][key])), key
