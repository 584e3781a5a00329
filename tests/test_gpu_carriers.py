"""Carrier contexts on the GPU (ookd_rx_create_carriers; fir1_tuned_multi_kernel in fir_tuned.hip): several carriers
of one capture decoded in one pass.  The contract is the header's: carrier k is, bit for bit, a context tuned to
nu_k with threshold_k.  Expected values come from the numpy restatement of the tuned contract
(tests/tuned_contract.py) fed with the library's own taps, so bits and edges are compared exactly."""
import ctypes as C

import numpy as np
import pytest

from tests.helpers import edges_of, golden_path
from tests.test_gpu_tuned import _dev, _fs32, _rand_taps, _tight, _write
from tests.tuned_contract import RATE, SPB, THR, contract_rx, golden_capture, lib_stages, moved, to_8bit

pytestmark = pytest.mark.gpu

DC = 400.0 * (1 + 0.5j)
NOISE = 40
NU1, NU2 = 600e3 / RATE, -900e3 / RATE
WINDOW = 512                    # outputs per wave tile with the quiet shortcut (R = 8)


@pytest.fixture(scope="module")
def ok():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from ookiedokie_amd import build as okbuild
    okbuild.build()
    import ookiedokie_amd as okm
    okm.lib()
    return okm


@pytest.fixture(scope="module")
def two_carriers():
    """G1 at +600 kHz plus G2 (zero-extended) at -900 kHz, with a DC term and noise, both transmitters at half level
    (as tests/spectrum_contract.py: two_transmitters).  The level follows from the filter and the threshold, not from
    the code under test: at full level the other transmitter's keying transients pass fs32_fs4 with up to 0.148
    (at +600 kHz) and 0.156 (at -900 kHz) where the carrier itself is off -- above the threshold of 0.1, so no decoder
    at that threshold recovers the messages, a single tuned context included (it reports 464 edges instead of 228).
    At half level they reach 0.081 and 0.091 (the contract in numpy, on the CPU)."""
    g1, m1 = golden_capture("G1")
    g2, m2 = golden_capture("G2")
    ext = np.zeros_like(g1)
    ext[:g2.size] = g2
    z = moved(g1, NU1, scale=0.5).astype(np.int32) + moved(ext, NU2, DC, NOISE, seed=11, scale=0.5).astype(np.int32)
    iq = np.clip(z, -32768, 32767).astype(np.int16)
    iq.setflags(write=False)
    return iq, (g1, m1), (g2, m2)


CARRIERS1 = [(NU1, 0.1), (NU2, 0.1), (0.0, 0.1), (NU1, 0.05)]


@pytest.fixture(scope="module")
def two_carriers_contract(ok, two_carriers):
    """bits and floats of the contract for every carrier of CARRIERS1 (computed once)"""
    iq = two_carriers[0]
    f = _fs32(ok)
    out = [contract_rx(iq, lib_stages(f, nu), thr, SPB) for nu, thr in CARRIERS1]
    for b, y in out:
        b.setflags(write=False)
        y.setflags(write=False)
    return out


def _check_bits(rx, k, bits, what=""):
    b = rx.bits(k)
    assert b.size == bits.size
    diff = np.nonzero(b != bits)[0]
    assert diff.size == 0, "carrier %d %s: first differing bits at %s" % (k, what, diff[:5])


# ------------------------------------------------------------- 1. each carrier is its own tuned context ----

def test_each_carrier_is_its_own_tuned_context(ok, oracle, two_carriers, two_carriers_contract):
    iq, (g1, m1), (g2, m2) = two_carriers
    n = iq.size // 2
    f = _fs32(ok)
    ofir = oracle.load_filter_json(golden_path("filters", "fs32_fs4"))
    K = len(CARRIERS1)
    # what single tuned contexts give on the GPU
    single = []
    for nu, thr in CARRIERS1:
        rx = ok.Receiver(f, None, max_samples=n, threshold=thr, tune=nu)
        rx.rx(iq)
        single.append(rx.bits().copy())
        rx.close()
    for cap_k, (base, meta) in ((0, (g1, m1)), (1, (g2, m2))):
        d, od = _dev(ok, oracle, meta)
        want = oracle.rx(base, ofir, THR, od, SPB)
        assert len(want.msg_samples) > 0
        res = {}
        for quiet in (True, False):
            rx = ok.Receiver(f, d, max_samples=n, carriers=CARRIERS1, quiet_skip=quiet, count_quiet=True)
            assert rx.num_carriers == K and rx.tune == 0.0
            assert rx.front_info()["form"] == ok.FRONT_TUNED_MULTI
            for k, (nu, thr) in enumerate(CARRIERS1):
                assert rx.carrier(k) == (nu, float(np.float32(thr)))
                assert rx.carrier_front_info(k)["form"] == ok.FRONT_TUNED_MULTI
            got = rx.rx(iq)
            assert got.stats["front_form"] == ok.FRONT_TUNED_MULTI
            for k in range(K):
                bits = two_carriers_contract[k][0]
                _check_bits(rx, k, bits, "quiet=%s" % quiet)
                assert list(rx.edges(k)) == list(edges_of(bits)), k
                assert (rx.bits(k) == single[k]).all(), k
            r = got.for_capture(cap_k)
            assert list(r.msg_samples) == list(want.msg_samples)
            assert (r.payloads == want.payloads).all()
            res[quiet] = got.stats
            rx.close()
        st = res[True]
        print("quiet (window, carrier) pairs", st["quiet_waves"], "of", st["total_waves"])
        windows = -(-(-(-n // SPB) * SPB) // 4096) * (4096 // WINDOW)
        assert st["total_waves"] == K * windows
        assert 0 < st["quiet_waves"] < st["total_waves"]
        assert res[False]["quiet_waves"] == 0
        assert res[False]["total_waves"] == K * (windows // 2)          # R = 16 without the shortcut


# ------------------------------------------------------------------------------------------- 2. floats ----

def test_floats(ok, record_property, two_carriers, two_carriers_contract):
    iq = two_carriers[0]
    n = iq.size // 2
    f = _fs32(ok)
    K = len(CARRIERS1)
    rx = ok.Receiver(f, None, max_samples=n, carriers=CARRIERS1, keep_fir=True, edge_capacity=4 * n + 64)
    got = rx.rx(iq)
    assert got.stats["front_form"] == ok.FRONT_TUNED_MULTI
    worst = 0.0
    for k in range(K):
        bits, y = two_carriers_contract[k]
        info = rx.carrier_front_info(k)
        assert info["err_valu"] > 0 and info["p_lo"] < info["p_star"] < info["p_hi"]
        _check_bits(rx, k, bits, "keep_fir")
        ratio = float(np.abs(rx.fir_output(k).astype(np.float64) - y.astype(np.float64)).max() / info["err_valu"])
        print("worst |y - y_ref| / err_valu, carrier", k, ratio)
        worst = max(worst, ratio)
    record_property("worst_over_err_valu", worst)
    assert worst <= 1.0
    rx.close()
    rx = ok.Receiver(f, None, max_samples=n, carriers=CARRIERS1, keep_fir=True, exact_fir=True, edge_capacity=4 * n + 64)
    assert rx.front_info()["form"] == ok.FRONT_TUNED_GENERIC
    got = rx.rx(iq)
    assert got.stats["front_form"] == ok.FRONT_TUNED_GENERIC
    for k in range(K):
        bits, y = two_carriers_contract[k]
        _check_bits(rx, k, bits, "exact_fir")
        assert (rx.fir_output(k).view(np.uint32) == y.view(np.uint32)).all(), k
    rx.close()


# --------------------------------------------- 3. quiet for some, loud for others, and nothing leaks ----

@pytest.mark.parametrize("stamp0", [None, 0xffff - 1], ids=["stamp-1", "stamp-wraps"])
def test_quiet_for_some_loud_for_others_and_nothing_leaks(ok, stamp0, monkeypatch):
    if stamp0 is not None:
        monkeypatch.setenv("OOKD_DEVELOPER", "1")
        monkeypatch.setenv("OOKD_TILE_STAMP_START", str(stamp0))       # the second run's stamp wraps
    nu = NU1
    g1, _ = golden_capture("G1")
    g2, _ = golden_capture("G2")
    a = moved(g1, nu, DC, NOISE, seed=31)
    b = moved(g2, -nu, DC, NOISE, seed=32)                  # other pulses, on the other carrier, and shorter
    carriers = [(nu, 0.1), (nu, 8.0), (-nu, 0.1)]
    f = _fs32(ok)
    want = {}
    for name, iq in (("a", a), ("b", b)):
        want[name] = [contract_rx(iq, lib_stages(f, c), t, SPB)[0] for c, t in carriers]
    assert want["a"][0].any() and want["b"][2].any()
    rx = ok.Receiver(f, None, max_samples=a.size // 2, carriers=carriers, count_quiet=True, edge_capacity=a.size)
    for name, iq in (("a", a), ("b", b), ("a", a)):
        got = rx.rx(iq)
        assert got.stats["front_form"] == ok.FRONT_TUNED_MULTI
        for k in range(3):
            assert list(rx.edges(k)) == list(edges_of(want[name][k])), (name, k)        # (before the bits are read
            _check_bits(rx, k, want[name][k], name)                                    #  back, which cleans up)
        assert not rx.bits(1).any()
        # the 8.0 carrier takes the shortcut in every interior window: all that hold capture samples only, but the first
        assert got.stats["quiet_waves"] >= (iq.size // 2) // WINDOW - 1
        assert got.stats["quiet_waves"] < got.stats["total_waves"]
    rx.close()


# -------------------------------------------------------------------------------------- 4. guard band ----

@pytest.mark.parametrize("ntaps", [32, 255])
def test_guard_band_on_one_carriers_threshold(ok, tmp_path, ntaps):
    nus = [-0.3, 0.2, 0.45]
    f = ok.Filter.load(_write(tmp_path, "t%d" % ntaps, [(1, _rand_taps(ntaps, ntaps))]))
    stages = lib_stages(f, nus[1])
    iq, outs = _tight(stages[0][1], stages[0][2], 2047, 3000, np.random.default_rng(ntaps), False)
    n = iq.size // 2
    _, y = contract_rx(iq, stages, 1.0, SPB)
    mag = np.hypot(y[outs, 0].astype(np.float64), y[outs, 1].astype(np.float64))
    thr = float(np.float32(np.median(mag)))
    carriers = [(nus[0], thr), (nus[1], thr), (nus[2], 0.5 * thr)]
    rx = ok.Receiver(f, None, max_samples=n, carriers=carriers, edge_capacity=3 * n + 64)
    got = rx.rx(iq)
    assert got.stats["front_form"] == ok.FRONT_TUNED_MULTI
    for k, (nu, t) in enumerate(carriers):
        bits, _ = contract_rx(iq, lib_stages(f, nu), t, SPB)
        if k == 1:
            assert 0.2 < bits[outs].mean() < 0.8                # the planted outputs straddle carrier 1's threshold
        _check_bits(rx, k, bits)
    must = int(np.count_nonzero(np.abs(mag - thr) <= rx.carrier_front_info(1)["err_valu"]))
    assert must > 100
    assert got.stats["guard_recomputes"] >= must
    rx.close()


# --------------------------------------------------------------------- 5. carrier counts and lengths ----

@pytest.mark.parametrize("quiet", [True, False], ids=["R8", "R16"])
@pytest.mark.parametrize("K", [1, 16])
def test_carrier_counts_and_lengths(ok, tmp_path, K, quiet):
    rng = np.random.default_rng(12 + K)
    one = ok.Filter.load(_write(tmp_path, "one", [(1, np.array([0.75], np.float32))]))
    t31 = ok.Filter.load(_write(tmp_path, "t31", [(1, _rand_taps(31, 4))]))
    nus = [0.37] if K == 1 else [float(v) for v in np.linspace(-0.5, 0.5, K)]
    carriers = [(nu, 0.05 + 0.01 * (k % 3)) for k, nu in enumerate(nus)]
    for f, n, spb in ((one, 777, 100), (t31, 20, 8192), (t31, 20, 16), (t31, 8192 + 513, 1000), (one, 5000, 8192)):
        iq = rng.integers(-400, 401, size=2 * n).astype(np.int16)
        rx = ok.Receiver(f, None, max_samples=n, samples_per_buffer=spb, edge_capacity=K * (2 * n + 8192), carriers=carriers,
                         quiet_skip=quiet)
        got = rx.rx(iq)
        assert got.stats["front_form"] == ok.FRONT_TUNED_MULTI and rx.num_carriers == K
        for k, (nu, thr) in enumerate(carriers):
            bits, _ = contract_rx(iq, lib_stages(f, nu), thr, spb)
            _check_bits(rx, k, bits, "n=%d spb=%d" % (n, spb))
            assert list(rx.edges(k)) == list(edges_of(bits))
        rx.close()


# ------------------------------------------------------------------------------------ 6. other shapes ----

def test_other_shapes_run_the_generic_form_per_carrier(ok, tmp_path):
    base, _ = golden_capture("G2")
    iq = (moved(base, 0.2, DC, NOISE, seed=6).astype(np.int32) + moved(base, -0.1, seed=7).astype(np.int32))
    iq = np.clip(iq, -32768, 32767).astype(np.int16)[:2 * 150000]
    n = iq.size // 2
    carriers = [(0.2, THR), (-0.1, 0.07), (0.0, THR)]
    for name, path in (("dec4", golden_path("filters", "fs128_fs16_dec4")),
                       ("t257", _write(tmp_path, "t257", [(1, _rand_taps(257, 9))])),
                       ("dec3x2", _write(tmp_path, "dec3x2", [(3, _rand_taps(7, 1)), (2, _rand_taps(40, 2))]))):
        f = ok.Filter.load(path)
        rx = ok.Receiver(f, None, max_samples=n, edge_capacity=3 * n + 64, keep_fir=True, carriers=carriers,
                         samples_per_buffer=6144)
        assert rx.front_info()["form"] == ok.FRONT_TUNED_GENERIC, name
        got = rx.rx(iq)
        assert got.stats["front_form"] == ok.FRONT_TUNED_GENERIC
        for k, (nu, thr) in enumerate(carriers):
            bits, y = contract_rx(iq, lib_stages(f, nu), thr, 6144)
            _check_bits(rx, k, bits, name)
            assert (rx.fir_output(k).view(np.uint32) == y.view(np.uint32)).all(), (name, k)
        rx.close()


# ------------------------------------------------------------------------------------------- 7. 8-bit ----

def _held(ok, f, max_samples, ptr, n, **kw):
    """device memory a context holds after its first run, in bytes; the form that ran"""
    import torch
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    rx = ok.Receiver(f, None, max_samples=max_samples, edge_capacity=1 << 16, **kw)
    rx.process_device(ptr, n)
    torch.cuda.synchronize()
    ran = free0 - torch.cuda.mem_get_info()[0]
    form = rx.stats()["front_form"]
    rx.close()
    return ran, form


@pytest.mark.parametrize("fmt", ["cs8", "cu8"])
def test_8bit_captures_are_widened_once(ok, two_carriers, fmt):
    import torch
    raw, wide = to_8bit(two_carriers[0], fmt)
    n = raw.size // 2
    f = _fs32(ok)
    carriers = [(NU1, THR), (NU2, THR), (0.0, 0.05)]
    rx = ok.Receiver(f, None, max_samples=n, carriers=carriers, sample_format=fmt, edge_capacity=3 * n + 64)
    assert rx.sample_bytes == 2
    got = rx.rx(raw)
    assert got.stats["front_form"] == ok.FRONT_TUNED_MULTI
    for k, (nu, thr) in enumerate(carriers):
        bits, _ = contract_rx(wide, lib_stages(f, nu), thr, SPB)
        assert bits.any()
        _check_bits(rx, k, bits, fmt)
    rx.close()
    # One staging copy, not K: the carrier context holds what a single tuned 8-bit context holds plus the result
    # buffers of K - 1 more captures.  Per capture and sample those are 1/8 B of bit words and less than that of tile
    # infos and block counts (the edge list is fixed here): under 1 B; a staging copy is 4 B per sample.
    M = 1 << 24
    dev_raw = torch.from_numpy(raw.view(np.uint8)).cuda()
    K = len(carriers)
    one, form1 = _held(ok, f, M, dev_raw.data_ptr(), n, tune=NU1, sample_format=fmt)
    many, formk = _held(ok, f, M, dev_raw.data_ptr(), n, carriers=carriers, sample_format=fmt)
    assert form1 == ok.FRONT_TUNED_FIR1 and formk == ok.FRONT_TUNED_MULTI
    print("context bytes: single %d, %d carriers %d, max_samples %d" % (one, K, many, M))
    assert one >= 4 * M                                         # the staging copy is there
    assert many - one <= (K - 1) * M, "more than the result buffers of %d captures: a staging copy per carrier?" % (K - 1)


# ------------------------------------------------------------------------- 8. host path and reruns ----

def test_host_path_submit_and_wait(ok, oracle, two_carriers, two_carriers_contract):
    import torch
    iq, (g1, m1), _ = two_carriers
    n = iq.size // 2
    f = _fs32(ok)
    d, od = _dev(ok, oracle, m1)
    want = oracle.rx(g1, oracle.load_filter_json(golden_path("filters", "fs32_fs4")), THR, od, SPB)
    dev_t = torch.from_numpy(np.array(iq)).cuda()
    rx = ok.Receiver(f, d, max_samples=n, carriers=CARRIERS1)
    runs = []
    got = rx.rx(iq)                                             # ookd_rx_process_host
    runs.append(([rx.bits(k).copy() for k in range(4)], got))
    got = rx.rx_device(dev_t.data_ptr(), n)                     # ookd_rx_process_device
    runs.append(([rx.bits(k).copy() for k in range(4)], got))
    rx.submit_device(dev_t.data_ptr(), n)
    rx.wait()
    got = rx.result()
    runs.append(([rx.bits(k).copy() for k in range(4)], got))
    for bits, got in runs:
        for k in range(4):
            assert (bits[k] == two_carriers_contract[k][0]).all(), k
        assert list(got.msg_samples) == list(runs[0][1].msg_samples)
        assert list(got.captures) == list(runs[0][1].captures)
        assert (got.payloads == runs[0][1].payloads).all()
        r = got.for_capture(0)
        assert list(r.msg_samples) == list(want.msg_samples) and (r.payloads == want.payloads).all()
    rx.close()


# --------------------------------------------------------------------------------------- 9. refusals ----

def _raw_create(ok, f, entries, reserved=0, max_captures=0, null=False, count=None):
    cfg = ok.RxConfig()
    cfg.threshold = 0.1
    cfg.samples_per_buffer = 8192
    cfg.max_samples = 8192
    cfg.max_captures = max_captures
    arr = (ok.RxCarrier * max(len(entries), 1))()
    for k, (nu, thr) in enumerate(entries):
        arr[k].nu, arr[k].threshold = nu, thr
        arr[k].reserved[3] = reserved
    h = ok.lib().ookd_rx_create_carriers(C.byref(cfg), f._h if f else None, None, None if null else arr,
                                         len(entries) if count is None else count)
    return h, ok.last_error()


def test_refusals(ok):
    import torch
    f = _fs32(ok)
    with pytest.raises(ok.OokdError, match="carriers"):
        ok.Receiver(f, None, max_samples=64, carriers=[])
    with pytest.raises(ok.OokdError, match="carriers"):
        ok.Receiver(f, None, max_samples=64, carriers=[0.01 * k for k in range(17)])
    with pytest.raises(ok.OokdError, match="nu must be within"):
        ok.Receiver(f, None, max_samples=64, carriers=[0.1, float("nan")])
    with pytest.raises(ok.OokdError, match="nu must be within"):
        ok.Receiver(f, None, max_samples=64, carriers=[0.51])
    with pytest.raises(ok.OokdError, match="needs a filter"):
        ok.Receiver(None, None, max_samples=64, carriers=[0.1])
    with pytest.raises(ok.OokdError, match="one capture per run"):
        ok.Receiver(f, None, max_samples=64, carriers=[0.1], max_captures=2)
    with pytest.raises(ValueError):
        ok.Receiver(f, None, max_samples=64, carriers=[0.1], tune=0.1)
    with pytest.raises(ValueError):
        ok.Receiver(f, None, max_samples=64, carriers=[0.1], tune_hz=1e5, sample_rate=3e6)
    h, msg = _raw_create(ok, f, [(0.1, 0.1)], reserved=1)
    assert not h and "reserved" in msg
    h, msg = _raw_create(ok, f, [(0.1, 0.1)], null=True)
    assert not h and "NULL" in msg
    h, msg = _raw_create(ok, f, [(0.1, 0.1)])
    assert h, msg
    ok.lib().ookd_rx_destroy(C.c_void_p(h))
    # runs a carrier context does not take; it stays usable
    n = 3 * 8192
    iq = np.random.default_rng(3).integers(-900, 901, size=4 * n).astype(np.int16)
    dev_t = torch.from_numpy(iq).cuda()
    carriers = [(0.2, 0.1), (-0.2, 0.1)]
    rx = ok.Receiver(f, None, max_samples=n, carriers=carriers, edge_capacity=2 * n + 64)
    with pytest.raises(ok.OokdError, match="one capture per run"):
        rx.rx_device(dev_t.data_ptr(), n, num_captures=2)
    with pytest.raises(ok.OokdError, match="shards"):
        rx.shard_begin(dev_t.data_ptr(), n, None, True, None)
    with pytest.raises(ok.OokdError, match="shards"):
        rx.shard_refine(ok.FsmState())
    with pytest.raises(ok.OokdError):
        rx.carrier(2)
    with pytest.raises(ok.OokdError):
        rx.carrier_front_info(2)
    rx.rx_device(dev_t.data_ptr(), n)
    for k, (nu, thr) in enumerate(carriers):
        bits, _ = contract_rx(iq[:2 * n], lib_stages(f, nu), thr, SPB)
        _check_bits(rx, k, bits)
    with pytest.raises(ok.OokdError):
        rx.bits(2)
    rx.close()
    # every other context has no carriers
    rx = ok.Receiver(f, None, max_samples=64, tune=0.1)
    assert rx.num_carriers == 0
    with pytest.raises(ok.OokdError):
        rx.carrier(0)
    rx.close()
