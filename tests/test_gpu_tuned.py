"""The frequency-tuned front end on the GPU (ookd_rx_create_tuned; fir_tuned.hip).  Expected values come from the
numpy restatement of the contract (tests/tuned_contract.py; test_tuned_host.py pins it to the CPU oracle at nu = 0)
fed with the library's own taps (Filter.tuned_taps), so bits -- and the floats of the contract-order form -- are
compared exactly."""
import zlib

import numpy as np
import pytest

from tests.helpers import edges_of, golden_path
from tests.tuned_bounds_inputs import rand_taps as _rand_taps, tight as _tight, write_filter as _write
from tests.tuned_contract import RATE, SPB, THR, contract_rx, golden_capture, lib_stages, moved, to_8bit

pytestmark = pytest.mark.gpu

DC = 400.0 * (1 + 0.5j)
NOISE = 40


@pytest.fixture(scope="module")
def ok():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from ookiedokie_amd import build as okbuild
    okbuild.build()
    import ookiedokie_amd as okm
    okm.lib()
    return okm


def _fs32(ok):
    return ok.Filter.load(golden_path("filters", "fs32_fs4"))


def _dev(ok, oracle, g, rate=RATE):
    """the device a golden capture was generated for (vectors.json), for the library and for the oracle"""
    return (ok.Device.load(golden_path("devices", g["device"]), rate),
            oracle.load_device_json(golden_path("devices", g["device"]), rate)[0])


# ---------------------------------------------------------------- 1. nu = 0 is ookd_rx_create ----

@pytest.mark.parametrize("fname", ["fs32_fs4", "fs128_fs16_dec4"])
def test_nu_0_is_the_untuned_context(ok, oracle, fname):
    iq, g = golden_capture("G2")
    iq = (iq + np.random.default_rng(1).integers(-NOISE, NOISE + 1, size=iq.size)).astype(np.int16)
    f = ok.Filter.load(golden_path("filters", fname))
    d, _ = _dev(ok, oracle, g, RATE // f.total_decimation)
    n = iq.size // 2
    res = []
    for tune in (None, 0.0, -0.0):
        rx = ok.Receiver(f, d, max_samples=n, tune=tune)
        assert rx.tune == 0.0
        info = rx.front_info()
        got = rx.rx(iq)
        st = {k: v for k, v in got.stats.items() if not k.endswith("_ms")}
        res.append((info, st, rx.bits().copy(), list(got.msg_samples), got.payloads.copy()))
        rx.close()
    assert res[0][0]["form"] in (ok.FRONT_FIR1_MFMA, ok.FRONT_FIR2_MFMA)
    assert len(res[0][3]) == 2 or fname != "fs32_fs4"
    for r in res[1:]:
        assert r[0] == res[0][0]
        assert r[1] == res[0][1]
        assert (r[2] == res[0][2]).all()
        assert r[3] == res[0][3]
        assert (r[4] == res[0][4]).all()


def test_create_tuned_refusals(ok):
    f = _fs32(ok)
    for nu in (0.51, -0.7, float("nan")):
        with pytest.raises(ok.OokdError):
            ok.Receiver(f, None, max_samples=64, tune=nu)
    with pytest.raises(ok.OokdError, match="does not depend on nu"):
        ok.Receiver(None, None, max_samples=64, tune=0.1)
    rx = ok.Receiver(None, None, max_samples=64, tune=0.0)             # no filter, nothing to tune: fine
    assert rx.front_info()["form"] == ok.FRONT_NO_FILTER
    rx.close()
    rx = ok.Receiver(f, None, max_samples=64, tune_hz=600e3, sample_rate=3e6)
    assert rx.tune == 600e3 / 3e6 and rx.halo_samples == 31
    rx.close()


# ------------------------------------------------------------------------------- 2. parity ----

NUS = [0.2, -0.3, 1.0 / 3000.0, 0.5]


@pytest.mark.parametrize("fmt", ["sc16q11", "cs8", "cu8"])
@pytest.mark.parametrize("nu", NUS, ids=["p0.2", "m0.3", "1_3000", "0.5"])
@pytest.mark.parametrize("cap", ["G1", "G2"])
def test_parity_with_the_contract(ok, record_property, cap, nu, fmt):
    """forms 13 and 12 (exact_fir) on a golden capture moved to nu with DC and noise: bits identical; floats
    bitwise for form 12, within err_valu per component for form 13"""
    base, _ = golden_capture(cap)
    iq = moved(base, nu, DC, NOISE, seed=zlib.crc32(("%s/%g" % (cap, nu)).encode()))
    if fmt != "sc16q11":
        raw, iq = to_8bit(iq, fmt)
    else:
        raw = iq
    f = _fs32(ok)
    n = iq.size // 2
    bits, y = contract_rx(iq, lib_stages(f, nu), THR, SPB)
    for exact in (False, True):
        rx = ok.Receiver(f, None, max_samples=n, edge_capacity=n + 64, keep_fir=True, exact_fir=exact, tune=nu,
                         sample_format=fmt, fir_valu=not exact)          # fir_valu: accepted, changes nothing
        form = ok.FRONT_TUNED_GENERIC if exact else ok.FRONT_TUNED_FIR1
        info = rx.front_info()
        assert info["form"] == form
        got = rx.rx(raw)
        assert got.stats["front_form"] == form
        b = rx.bits()
        diff = np.nonzero(b != bits)[0]
        assert diff.size == 0, "first differing bits at %s (exact=%s)" % (diff[:5], exact)
        assert list(rx.edges()) == list(edges_of(bits))
        yo = rx.fir_output()
        if exact:
            assert (yo.view(np.uint32) == y.view(np.uint32)).all()
        else:
            assert info["err_valu"] > 0 and info["p_lo"] < info["p_star"] < info["p_hi"]
            worst = float(np.abs(yo.astype(np.float64) - y.astype(np.float64)).max() / info["err_valu"])
            record_property("worst_over_err_valu", worst)
            print("worst |y - y_ref| / err_valu", cap, nu, fmt, worst)
            assert worst <= 1.0
        rx.close()


# ------------------------------------------------------------------------------ 3. recovery ----

@pytest.mark.parametrize("hz", [600e3, -900e3])
@pytest.mark.parametrize("cap,nmsg", [("G1", 3), ("G2", 2)])
def test_recovery_of_an_off_centre_carrier(ok, oracle, cap, nmsg, hz):
    """payloads and message sample indices of the tuned decode are the oracle's on the capture that was never moved;
    an untuned context finds nothing in the moved one; the quiet shortcut takes some windows and not all"""
    base, g = golden_capture(cap)
    nu = hz / RATE
    iq = moved(base, nu, DC, NOISE, seed=int(abs(hz)) + nmsg)
    n = iq.size // 2
    f = _fs32(ok)
    d, od = _dev(ok, oracle, g)
    want = oracle.rx(base, oracle.load_filter_json(golden_path("filters", "fs32_fs4")), THR, od, SPB)
    assert len(want.msg_samples) == nmsg
    res = {}
    for quiet in (True, False):
        rx = ok.Receiver(f, d, max_samples=n, tune_hz=hz, sample_rate=RATE, quiet_skip=quiet, count_quiet=True)
        got = rx.rx(iq)
        assert got.stats["front_form"] == ok.FRONT_TUNED_FIR1
        assert list(got.msg_samples) == list(want.msg_samples)
        assert (got.payloads == want.payloads).all()
        res[quiet] = (rx.bits().copy(), got.stats)
        rx.close()
    # 5. the shortcut changes no bit, and it is taken: the DC term does not keep the silence loud
    assert (res[True][0] == res[False][0]).all()
    st = res[True][1]
    print("quiet windows", cap, hz, st["quiet_waves"], "of", st["total_waves"])
    assert 0 < st["quiet_waves"] < st["total_waves"]
    assert res[False][1]["quiet_waves"] == 0
    bits, _ = contract_rx(iq, lib_stages(f, nu), THR, SPB)
    assert (res[True][0] == bits).all()
    rx = ok.Receiver(f, d, max_samples=n)
    assert len(rx.rx(iq).msg_samples) == 0
    rx.close()


# ---------------------------------------------------------------------------- 4. guard band ----

@pytest.mark.parametrize("cancel", [False, True], ids=["aligned", "cancel"])
@pytest.mark.parametrize("ntaps", [32, 255])
def test_guard_band_at_the_threshold(ok, tmp_path, ntaps, cancel):
    nu = 0.2
    path = _write(tmp_path, "t%d" % ntaps, [(1, _rand_taps(ntaps, ntaps))])
    f = ok.Filter.load(path)
    stages = lib_stages(f, nu)
    rng = np.random.default_rng(ntaps + cancel)
    iq, outs = _tight(stages[0][1], stages[0][2], 2047, 3000, rng, cancel)
    n = iq.size // 2
    _, y = contract_rx(iq, stages, 1.0, SPB)
    mag = np.hypot(y[outs, 0].astype(np.float64), y[outs, 1].astype(np.float64))
    thr = float(np.float32(np.median(mag)))
    bits, _ = contract_rx(iq, stages, thr, SPB)
    assert 0.2 < bits[outs].mean() < 0.8                        # the planted outputs straddle the threshold
    rx = ok.Receiver(f, None, max_samples=n, threshold=thr, edge_capacity=n + 64, tune=nu)
    info = rx.front_info()
    got = rx.rx(iq)
    assert got.stats["front_form"] == ok.FRONT_TUNED_FIR1
    diff = np.nonzero(rx.bits() != bits)[0]
    assert diff.size == 0, "first differing bits at %s" % diff[:5]
    must = int(np.count_nonzero(np.abs(mag - thr) <= info["err_valu"]))
    assert must > 100
    assert got.stats["guard_recomputes"] >= must
    rx.close()


@pytest.mark.parametrize("thr", [0.0, float("nan")])
def test_empty_band_thresholds(ok, thr):
    """threshold 0 / NaN: p_lo == p_hi == p_star, nothing is recomputed, bits as the contract's (all 1 / all 0)"""
    f = _fs32(ok)
    iq = np.random.default_rng(5).integers(-1500, 1501, size=2 * (2 * 8192 + 77)).astype(np.int16)
    n = iq.size // 2
    rx = ok.Receiver(f, None, max_samples=n, threshold=thr, edge_capacity=n + 64, tune=-0.3)
    info = rx.front_info()
    if thr == 0.0:
        assert info["p_lo"] == info["p_hi"] == info["p_star"] == 0.0
    else:
        assert np.isnan(info["p_star"]) and np.isnan(info["p_lo"]) and np.isnan(info["p_hi"])
    got = rx.rx(iq)
    bits, _ = contract_rx(iq, lib_stages(f, -0.3), thr, SPB)
    assert (rx.bits() == bits).all()
    assert bits.all() if thr == 0.0 else not bits.any()
    assert got.stats["guard_recomputes"] == 0 and got.stats["front_form"] == ok.FRONT_TUNED_FIR1
    rx.close()


# -------------------------------------------------------------------------------- 6. shapes ----

def test_shapes_that_run_the_generic_form(ok, oracle, tmp_path):
    base, _ = golden_capture("G2")
    nu = 0.2
    iq = moved(base, nu, DC, NOISE, seed=6)[:2 * 150000]
    n = iq.size // 2
    for name, path in (("dec4", golden_path("filters", "fs128_fs16_dec4")),
                       ("t257", _write(tmp_path, "t257", [(1, _rand_taps(257, 9))])),
                       ("dec3x2", _write(tmp_path, "dec3x2", [(3, _rand_taps(7, 1)), (2, _rand_taps(40, 2))]))):
        f = ok.Filter.load(path)
        rx = ok.Receiver(f, None, max_samples=n, edge_capacity=n + 64, keep_fir=True, tune=nu, samples_per_buffer=6144)
        assert rx.front_info()["form"] == ok.FRONT_TUNED_GENERIC, name
        got = rx.rx(iq)
        assert got.stats["front_form"] == ok.FRONT_TUNED_GENERIC
        bits, y = contract_rx(iq, lib_stages(f, nu), THR, 6144)
        assert (rx.bits() == bits).all(), name
        assert (rx.fir_output().view(np.uint32) == y.view(np.uint32)).all(), name
        rx.close()


@pytest.mark.parametrize("exact", [False, True])
def test_one_tap_and_odd_lengths(ok, tmp_path, exact):
    """1 tap; lengths that are no multiple of the tile or of samples_per_buffer, and shorter than the taps"""
    rng = np.random.default_rng(12)
    one = ok.Filter.load(_write(tmp_path, "one", [(1, np.array([0.75], np.float32))]))
    t31 = ok.Filter.load(_write(tmp_path, "t31", [(1, _rand_taps(31, 4))]))
    form = ok.FRONT_TUNED_GENERIC if exact else ok.FRONT_TUNED_FIR1
    for f, n, spb in ((one, 5000, 8192), (one, 777, 100), (t31, 20, 8192), (t31, 20, 16), (t31, 8192 + 513, 1000),
                      (t31, 3 * 4096, 4096), (t31, 1, 1)):
        iq = rng.integers(-400, 401, size=2 * n).astype(np.int16)
        rx = ok.Receiver(f, None, max_samples=n, threshold=0.05, samples_per_buffer=spb, edge_capacity=2 * n + 8192,
                         tune=0.37, exact_fir=exact)
        got = rx.rx(iq)
        assert got.stats["front_form"] == form
        bits, _ = contract_rx(iq, lib_stages(f, 0.37), 0.05, spb)
        assert rx.bits().size == bits.size
        assert (rx.bits() == bits).all(), (n, spb)
        assert list(rx.edges()) == list(edges_of(bits))
        rx.close()


# ------------------------------------------------------------------------------ 7. plumbing ----

def test_batched_host_shards_reruns_recorder(ok, oracle, tmp_path):
    import torch
    base, g = golden_capture("G2")
    nu = -0.3
    f = _fs32(ok)
    d, od = _dev(ok, oracle, g)
    stages = lib_stages(f, nu)
    want_msgs = oracle.rx(base, oracle.load_filter_json(golden_path("filters", "fs32_fs4")), THR, od, SPB)
    # batched: three captures, stride > length, each with its own noise
    n = base.size // 2
    caps, stride = 3, n + 1000
    host = np.zeros((caps, 2 * stride), np.int16)
    for c in range(caps):
        host[c, :2 * n] = moved(base, nu, DC, NOISE, seed=70 + c)
    dev_t = torch.from_numpy(host).cuda()
    rx = ok.Receiver(f, d, max_samples=n, max_captures=caps, tune=nu)
    got = rx.rx_device(dev_t.data_ptr(), n, num_captures=caps, stride=stride)
    assert got.stats["front_form"] == ok.FRONT_TUNED_FIR1
    for c in range(caps):
        bits, _ = contract_rx(host[c, :2 * n], stages, THR, SPB)
        assert (rx.bits(c) == bits).all(), c
        r = got.for_capture(c)
        assert list(r.msg_samples) == list(want_msgs.msg_samples) and (r.payloads == want_msgs.payloads).all()
    rx.close()

    # one context, two runs of different lengths (sparse output, the run stamp), from host memory; the recorder
    iq = host[0, :2 * n].copy()
    short = iq[:2 * 150000]
    rx = ok.Receiver(f, d, max_samples=n, tune=nu)
    for run in (iq, short, iq):
        got = rx.rx(run)
        bits, _ = contract_rx(run, stages, THR, SPB)
        assert (rx.bits() == bits).all()
        assert list(rx.edges()) == list(edges_of(bits))
    assert list(got.msg_samples) == list(want_msgs.msg_samples)
    rx.rx(short)
    bits_s, _ = contract_rx(short, stages, THR, SPB)
    p = tmp_path / "dig.csv"
    rx.record_dig(str(p))
    assert p.read_text() == oracle.dig_text(bits_s, SPB) == rx.dig_text()
    rx.close()

    # whole capture == two shards, the second with the first one's tail as its halo
    bits_w, _ = contract_rx(iq, stages, THR, SPB)
    dev_t = torch.from_numpy(iq).cuda()
    half = (n // 2) // SPB * SPB
    state, msgs, pays = None, [], []
    for r, (lo, hi) in enumerate(((0, half), (half, n))):
        rx = ok.Receiver(f, d, max_samples=n, tune=nu)
        H = rx.halo_samples
        halo = iq[2 * (lo - H):2 * lo] if r else None
        res, state = rx.shard_begin(dev_t.data_ptr() + 4 * lo, hi - lo, halo, r == 1, state)
        assert res.stats["front_form"] == ok.FRONT_TUNED_FIR1
        b = rx.bits()
        assert (b == bits_w[lo:lo + b.size]).all(), r
        msgs += [int(s) + lo for s in res.msg_samples]
        pays += [bytes(x) for x in res.payloads]
        rx.close()
    assert msgs == [int(s) for s in want_msgs.msg_samples]
    assert pays == [bytes(x) for x in want_msgs.payloads]
