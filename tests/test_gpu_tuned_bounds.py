"""The fused tuned kernels at their bounds and tap shapes: fir1_tuned_kernel<8 / 16> (a context tuned to nu, form 13)
and fir1_tuned_multi_kernel<8 / 16> (a carrier context, form 14), every test on both from one parametrisation.  The
carrier leg holds the tested nu, another nu, nu = 0 and the tested nu at a second threshold.  Expected bits and floats
come from the numpy contract (tests/tuned_contract.py) with the library's own taps; where an error is judged it is
also taken against a float64 sum over the same float32 taps and samples.  The inputs are built, and checked on the
CPU, in tests/tuned_bounds_inputs.py / tests/test_tuned_bounds_host.py.  Every test asserts the form that ran."""
import json
import zlib

import numpy as np
import pytest

from tests import tuned_bounds_inputs as B
from tests.helpers import edges_of, golden_path
from tests.test_gpu_front_bounds import MARGIN
from tests.tuned_contract import SPB, THR, contract_rx, golden_capture, lib_stages, moved

pytestmark = pytest.mark.gpu

FORMS = ["tuned", "carriers"]
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


_CONTRACT = {}


def _contract(key, iq, f, nu, thr, spb):
    """contract_rx with the library's taps, computed once per (capture, filter, nu, threshold) and never changed"""
    k = (key, float(nu), float(thr), spb)
    if k not in _CONTRACT:
        bits, y = contract_rx(iq, lib_stages(f, nu), thr, spb)
        bits.setflags(write=False)
        y.setflags(write=False)
        _CONTRACT[k] = (bits, y)
    return _CONTRACT[k]


def _other_nu(nu):
    return 0.11 if abs(abs(nu) - 0.11) > 1e-3 else 0.23


def _carrier_list(nu, thr, thr2=None):
    """the carrier leg: the tested (nu, thr) at index 1, among another nu, nu = 0 and nu at a second threshold"""
    return [(_other_nu(nu), thr), (nu, thr), (0.0, thr), (nu, 2.0 * thr if thr2 is None else thr2)], 1


def _create(ok, f, form, nu, thr, n, spb=SPB, carriers=None, **kw):
    """-> receiver, [(nu, thr)] per result index, the index of the tested carrier, the form it must run"""
    n_pad = -(-n // spb) * spb
    if form == "tuned":
        rx = ok.Receiver(f, None, max_samples=n, threshold=thr, samples_per_buffer=spb, edge_capacity=n_pad + 64,
                         tune=nu, **kw)
        return rx, [(nu, thr)], 0, ok.FRONT_TUNED_FIR1
    cl, k = (carriers, 0) if carriers is not None else _carrier_list(nu, thr)
    rx = ok.Receiver(f, None, max_samples=n, threshold=thr, samples_per_buffer=spb,
                     edge_capacity=len(cl) * (n_pad + 64), carriers=cl, **kw)
    assert rx.num_carriers == len(cl)
    return rx, cl, k, ok.FRONT_TUNED_MULTI


def _info(rx, form, k):
    return rx.front_info() if form == "tuned" else rx.carrier_front_info(k)


def _check_bits(rx, k, bits, what=""):
    edges = list(rx.edges(k))
    b = rx.bits(k)
    assert b.size == bits.size
    diff = np.nonzero(b != bits)[0]
    assert diff.size == 0, "result %d %s: first differing bits at %s" % (k, what, diff[:5])
    assert edges == list(edges_of(bits)), (k, what)


def _filter(ok, tmp_path, name, scale=1.0):
    if name == "fs32_fs4":
        return ok.Filter.load(golden_path("filters", name))
    n = int(name[1:])
    return ok.Filter.load(B.write_filter(tmp_path, name, [(1, B.rand_taps(n, n, 1.3 * scale))]))


def _waves(n, spb, R, results):
    """wave tiles of a run: whole 4096-output blocks of the padded capture, per result"""
    n_pad = -(-n // spb) * spb
    return results * (-(-n_pad // 4096) * (4096 // (64 * R)))


# ------------------------------------------------------------- 1. tap counts and register blocks ----

@pytest.fixture(scope="module")
def sweep_iq():
    iq = B.sweep_capture()
    iq.setflags(write=False)
    return iq


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("R", [8, 16])
@pytest.mark.parametrize("ntaps", B.SWEEP_TAPS)
def test_tap_count_sweep(ok, tmp_path, sweep_iq, ntaps, R, form):
    """every ntaps_pad from 32 to 256 at both register blocks: the chunk loop's window base, the partial last load
    round and the LDS window size all depend on it.  Floats within err_valu (keep_fir, every window filtered), bits
    and edges with the shortcut live (R = 8: some windows quiet, not all)."""
    import torch
    f = _filter(ok, tmp_path, "t%d" % ntaps)
    n, spb = B.SWEEP_N, B.SWEEP_SPB
    for nu in ((0.37, -0.5) if ntaps in (33, 96, 256) else (0.37,)):
        for keep in (True, False):
            rx, cl, k, want_form = _create(ok, f, form, nu, THR, n, spb, keep_fir=keep, quiet_skip=(R == 8),
                                           count_quiet=True)
            assert _info(rx, form, k)["form"] == want_form
            got = rx.rx(sweep_iq)
            assert got.stats["front_form"] == want_form
            assert got.stats["total_waves"] == _waves(n, spb, R, len(cl)), "another register block ran"
            for j, (cnu, cthr) in enumerate(cl):
                bits, y = _contract(("sweep", ntaps), sweep_iq, f, cnu, cthr, spb)
                _check_bits(rx, j, bits, "t%d nu %g keep_fir %s" % (ntaps, cnu, keep))
                if keep:
                    err = _info(rx, form, j)["err_valu"]
                    assert err > 0
                    d = np.abs(rx.fir_output(j).astype(np.float64) - y.astype(np.float64)).max()
                    assert d <= err, (j, d, err)
            st = got.stats
            if keep or R == 16:
                assert st["quiet_waves"] == 0
            else:
                print("quiet windows t%d nu %g %s: %d of %d" % (ntaps, nu, form, st["quiet_waves"], st["total_waves"]))
                assert 0 < st["quiet_waves"] < st["total_waves"]
            if ntaps in (33, 256) and nu == 0.37 and not keep:
                # the same samples behind a host pointer that is not 16-byte aligned (staged: the kernel still sees
                # an aligned buffer), and behind a device pointer one sample past a boundary (every window goes
                # through the per-sample fetch)
                got = rx.rx(B.unaligned_view(sweep_iq))
                assert got.stats["front_form"] == want_form
                for j, (cnu, cthr) in enumerate(cl):
                    _check_bits(rx, j, _contract(("sweep", ntaps), sweep_iq, f, cnu, cthr, spb)[0], "host + 4 bytes")
                dev_t = torch.zeros(2 * (n + 8), dtype=torch.int16, device="cuda")
                dev_t[2:2 + 2 * n] = torch.from_numpy(np.array(sweep_iq)).cuda()
                assert (dev_t.data_ptr() + 4) % 16 == 4
                got = rx.rx_device(dev_t.data_ptr() + 4, n)
                assert got.stats["front_form"] == want_form
                assert got.stats["quiet_waves"] == 0            # no window is "interior" behind such a pointer
                for j, (cnu, cthr) in enumerate(cl):
                    _check_bits(rx, j, _contract(("sweep", ntaps), sweep_iq, f, cnu, cthr, spb)[0], "device + 4 bytes")
            rx.close()


@pytest.mark.parametrize("form", FORMS)
def test_257_taps_run_the_generic_form(ok, tmp_path, sweep_iq, form):
    f = _filter(ok, tmp_path, "t257")
    n, spb = B.SWEEP_N, B.SWEEP_SPB
    rx, cl, k, _ = _create(ok, f, form, 0.37, THR, n, spb, keep_fir=True)
    assert rx.front_info()["form"] == ok.FRONT_TUNED_GENERIC
    got = rx.rx(sweep_iq)
    assert got.stats["front_form"] == ok.FRONT_TUNED_GENERIC
    for j, (cnu, cthr) in enumerate(cl):
        bits, y = _contract(("sweep", 257), sweep_iq, f, cnu, cthr, spb)
        _check_bits(rx, j, bits, "t257")
        assert (rx.fir_output(j).view(np.uint32) == y.view(np.uint32)).all(), j
    rx.close()


# ------------------------------------------------------------------------ 2. distance to the bound ----

MARGIN_NUS = [0.2, -0.3, 1.0 / 3000.0, 0.5]


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("nu", MARGIN_NUS, ids=["p0.2", "m0.3", "1_3000", "0.5"])
@pytest.mark.parametrize("name", ["t32", "t64", "t128", "t255", "t256"])
def test_error_bound_margin(ok, tmp_path, record_property, name, nu, form):
    """max |y_kernel - y_contract| / err_valu and max |y_kernel - y_float64| / err_valu per component and segment,
    at sign-aligned, cancelling, two-tone and full-scale noise inputs, nominal (2047) and wide (32767, with samples
    at -32768) amplitudes, both register blocks: <= 1.0 (tuned_guard_error's derivation: the fused chain is within
    gamma_2T S x_max of the exact sum, the contract within gamma_(2T+1)), and <= MARGIN, the project's safety
    factor.  Bits are the contract's in every leg.
    Measured on an MI355X (the same for both forms and both R): at most 0.0209 against the contract and 0.0243
    against the float64 sum, both at t32, nu = 1/3000, wide amplitude; 0.0013 / 0.0019 at nominal amplitude."""
    f = _filter(ok, tmp_path, name)
    rng = np.random.default_rng(zlib.crc32(("%s/%g" % (name, nu)).encode()))
    (_, re, im), = lib_stages(f, nu)
    worst = {}
    for amp, A in (("nominal", 2047), ("wide", 32767)):
        iq, _ = B.margin_capture(re, im, nu, A, rng)
        n = iq.size // 2
        y64 = B.sum64(iq, re, im, SPB)
        for R in (8, 16):
            rx, cl, k, want_form = _create(ok, f, form, nu, THR, n, keep_fir=True, quiet_skip=(R == 8))
            got = rx.rx(iq)
            assert got.stats["front_form"] == want_form
            assert got.stats["total_waves"] == _waves(n, SPB, R, len(cl))
            for j, (cnu, cthr) in enumerate(cl):
                bits, y = _contract(("margin", name, nu, amp), iq, f, cnu, cthr, SPB)
                _check_bits(rx, j, bits, "%s R=%d" % (amp, R))
            err = _info(rx, form, k)["err_valu"]
            assert err > 0
            yk = rx.fir_output(k).astype(np.float64)
            _, y = _contract(("margin", name, nu, amp), iq, f, nu, THR, SPB)
            dc = np.abs(yk - y.astype(np.float64)).max(axis=1) / err
            d64 = np.abs(yk - y64).max(axis=1) / err
            for s, seg in enumerate(B.MARGIN_SEGMENTS):
                sl = slice(s * B.MARGIN_SEG, (s + 1) * B.MARGIN_SEG)
                worst["contract_%s_R%d_%s" % (amp, R, seg)] = float(dc[sl].max())
                worst["float64_%s_R%d_%s" % (amp, R, seg)] = float(d64[sl].max())
            rx.close()
    for key, r in sorted(worst.items()):
        record_property(key, r)
    print("worst |y - y_ref| / err_valu", name, nu, form, json.dumps(worst))
    bad = {k: r for k, r in worst.items() if r > 1.0}
    assert not bad, "error beyond the bound: the guard band is unsound %s" % bad
    thin = {k: r for k, r in worst.items() if r > MARGIN}
    assert not thin, "error within a factor %.1f of the bound %s" % (1.0 / MARGIN, thin)


# ---------------------------------------------------------------------------- 3. tap magnitudes ----

@pytest.fixture(scope="module")
def scale_iq():
    iq = B.scale_capture()
    iq.setflags(write=False)
    return iq


def _no_nan(info):
    return not any(isinstance(v, float) and np.isnan(v) for v in info.values())


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("scale", B.SCALES, ids=["%g" % s for s in B.SCALES])
@pytest.mark.parametrize("name", ["t32", "t255"])
def test_tap_magnitudes(ok, tmp_path, scale_iq, name, scale, form):
    """taps of sum|h| = 1.3e-15 .. 1.3e15 with the threshold at the median of the contract's |y|: the quiet weights
    and the guard band are built from sums that scale with the taps; bits are the contract's with the shortcut on
    and off, the band is ordered and holds no NaN, and the fused form runs at every scale"""
    nu = 0.2
    f = _filter(ok, tmp_path, name, scale)
    n = B.SCALE_N
    _, y = _contract(("scale", name, scale), scale_iq, f, nu, 1.0, SPB)
    thr = float(np.float32(np.median(np.hypot(y[:, 0].astype(np.float64), y[:, 1].astype(np.float64)))))
    assert thr > 0 and np.isfinite(thr)
    for quiet in (True, False):
        rx, cl, k, want_form = _create(ok, f, form, nu, thr, n, quiet_skip=quiet, count_quiet=True)
        got = rx.rx(scale_iq)
        assert got.stats["front_form"] == want_form
        hi = 0
        for j, (cnu, cthr) in enumerate(cl):
            info = _info(rx, form, j)
            assert info["form"] == want_form and _no_nan(info), info
            assert info["p_lo"] <= info["p_star"] <= info["p_hi"] and info["err_valu"] > 0
            bits, _ = _contract(("scale", name, scale), scale_iq, f, cnu, cthr, SPB)
            assert bits.any() and not bits.all() or j != k
            _check_bits(rx, j, bits, "scale %g quiet %s" % (scale, quiet))
            hi += B.quiet_count_bounds(scale_iq, *lib_stages(f, cnu)[0][1:], cthr, bits, B.ntaps_pad(int(name[1:])))[1]
        print("quiet windows", name, scale, form, quiet, got.stats["quiet_waves"], "of", got.stats["total_waves"])
        assert got.stats["quiet_waves"] <= hi
        if not quiet:
            assert got.stats["quiet_waves"] == 0
        rx.close()


@pytest.mark.parametrize("form", FORMS)
def test_quiet_weights_out_of_range_switch_the_shortcut_off(ok, tmp_path, scale_iq, form):
    """taps of 1e15 against a threshold of 1e-20: the weights pass 1e30 and the carrier has no quiet test -- it must
    never be taken for quiet, alone or beside a carrier whose weights are in range"""
    nu, name, scale = 0.2, "t32", 1e15
    f = _filter(ok, tmp_path, name, scale)
    n = B.SCALE_N
    _, y = _contract(("scale", name, scale), scale_iq, f, nu, 1.0, SPB)
    thr = float(np.float32(np.median(np.hypot(y[:, 0].astype(np.float64), y[:, 1].astype(np.float64)))))
    carriers = [(nu, 1e-20), (nu, thr), (0.0, 1e-20)]
    rx, cl, k, want_form = _create(ok, f, form, nu, 1e-20, n, carriers=carriers, count_quiet=True)
    got = rx.rx(scale_iq)
    assert got.stats["front_form"] == want_form
    hi = 0
    for j, (cnu, cthr) in enumerate(cl):
        bits, _ = _contract(("scale", name, scale), scale_iq, f, cnu, cthr, SPB)
        _check_bits(rx, j, bits, "thr %g" % cthr)
        if cthr == thr:
            hi += B.quiet_count_bounds(scale_iq, *lib_stages(f, cnu)[0][1:], cthr, bits, 32)[1]
    assert got.stats["quiet_waves"] <= hi               # (0 for the tuned context: its only carrier has no test)
    rx.close()


# --------------------------------------------------- 4. the quiet shortcut at its decision ----

QUIET_NUS = [0.2, 0.125, 1.0 / 3000.0, 0.5]


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("dense", [False, True], ids=["sparse", "dense"])
@pytest.mark.parametrize("nu", QUIET_NUS, ids=["0.2", "0.125", "1_3000", "0.5"])
@pytest.mark.parametrize("thr", [0.02, 0.1, 0.5])
@pytest.mark.parametrize("name", ["fs32_fs4", "t255"])
def test_quiet_shortcut_soundness(ok, tmp_path, monkeypatch, name, thr, nu, dense, form):
    """Windows planted around the analytic quiet test a quiet_a + b quiet_b < 1 (tests/tuned_bounds_inputs.py:
    quiet_capture): worst-case spreads swept across the decision, a lone spike in the tap history, in the last
    partial load vector and at the tile's ends, both int16 extremes in one window, DC-only windows.  Each context
    runs a loud capture first, so a word a quiet window leaves behind shows.  Bits and edges are the contract's with
    the shortcut and without; quiet_waves lies between the windows whose documented left-hand side is below half the
    threshold and the windows whose contract bits are all zero (per carrier, summed)."""
    if dense:
        monkeypatch.setenv("OOKD_DEVELOPER", "1")
        monkeypatch.setenv("OOKD_DENSE_BITS", "1")
    f = _filter(ok, tmp_path, name)
    (_, re, im), = lib_stages(f, nu)
    Tp = B.ntaps_pad(re.size)
    iq, _ = B.quiet_capture(re, im, thr)
    n = iq.size // 2
    loud = B.loud_capture(n)
    # carriers at thr and 8 thr on the tested nu, thr on another (nu = 0)
    carriers = [(nu, thr), (nu, 8.0 * thr), (0.0, thr)] if form == "carriers" else None
    key = ("quiet", name, nu, thr)
    res = {}
    for quiet in (True, False):
        rx, cl, k, want_form = _create(ok, f, form, nu, thr, n, carriers=carriers, quiet_skip=quiet, count_quiet=True)
        got = rx.rx(loud)
        assert got.stats["front_form"] == want_form
        _check_bits(rx, k, _contract(("loud", name, n), loud, f, nu, thr, SPB)[0], "the loud run")
        got = rx.rx(iq)
        assert got.stats["front_form"] == want_form
        lo = hi = 0
        for j, (cnu, cthr) in enumerate(cl):
            bits, _ = _contract(key, iq, f, cnu, cthr, SPB)
            _check_bits(rx, j, bits, "quiet_skip %s" % quiet)
            (_, cre, cim), = lib_stages(f, cnu)
            a, b = B.quiet_count_bounds(iq, cre, cim, cthr, bits, Tp)
            lo, hi = lo + a, hi + b
        res[quiet] = [rx.bits(j).copy() for j in range(len(cl))]
        st = got.stats
        if quiet:
            print("quiet windows", name, thr, nu, form, "dense" if dense else "sparse", lo, "<=", st["quiet_waves"],
                  "<=", hi, "of", st["total_waves"])
            assert st["total_waves"] == _waves(n, SPB, 8, len(cl))
            assert 0 < lo <= st["quiet_waves"] <= hi
        else:
            assert st["quiet_waves"] == 0 and st["total_waves"] == _waves(n, SPB, 16, len(cl))
        rx.close()
    for a, b in zip(res[True], res[False]):
        assert (a == b).all()


# ------------------------------------------------------------------------- 5. split launches ----

@pytest.fixture(scope="module")
def split_captures():
    g1, _ = golden_capture("G1")
    base = B.tiled(g1, B.SPLIT_N)
    tuned = moved(base, 0.2, B.DC, NOISE, seed=51)
    plain = moved(base, 0.0, 0j, NOISE, seed=52)
    tuned.setflags(write=False)
    plain.setflags(write=False)
    return tuned, plain


@pytest.mark.parametrize("quiet", [True, False], ids=["R8", "R16"])
@pytest.mark.parametrize("form", FORMS + ["valu", "mfma"])
def test_split_launches(ok, oracle, monkeypatch, split_captures, form, quiet):
    """OOKD_FRONT_LAUNCH_LOG2=16: the front end goes out as several grid launches (tile_base, tile_begin /
    tile_count); bits, edges and quiet_waves are those of the one-launch context and the contract's (the oracle's
    for the real-tap forms, which share the launch loop)"""
    nu, n = 0.2, B.SPLIT_N
    f = _filter(ok, None, "fs32_fs4")
    if form in FORMS:
        iq = split_captures[0]
        cl = [(nu, THR), (0.0, THR), (nu, 0.05)] if form == "carriers" else [(nu, THR)]
        want = [_contract(("split",), iq, f, cnu, cthr, SPB)[0] for cnu, cthr in cl]
        assert want[0].any() and not want[0].all()
    else:
        iq = split_captures[1]
        of = oracle.load_filter_json(golden_path("filters", "fs32_fs4"))
        want = [oracle.rx(iq, of, THR, None, SPB, want_bits=True).bits]
        cl = [(0.0, THR)]

    def create():
        if form in FORMS:
            rx, _, _, want_form = _create(ok, f, form, nu, THR, n, carriers=cl if form == "carriers" else None,
                                          quiet_skip=quiet, count_quiet=True)
            return rx, want_form
        rx = ok.Receiver(f, None, max_samples=n, edge_capacity=n + 8192 + 64, fir_valu=(form == "valu"),
                         quiet_skip=quiet, count_quiet=True)
        return rx, (ok.FRONT_FIR1_VALU if form == "valu" else ok.FRONT_FIR1_MFMA)

    monkeypatch.delenv("OOKD_FRONT_LAUNCH_LOG2", raising=False)
    runs = []
    for split in (False, True):
        if split:
            monkeypatch.setenv("OOKD_DEVELOPER", "1")
            monkeypatch.setenv("OOKD_FRONT_LAUNCH_LOG2", "16")
        rx, want_form = create()
        got = rx.rx(iq)
        assert got.stats["front_form"] == want_form
        if split:
            assert got.stats["front_launches"] > 1
        else:
            assert got.stats["front_launches"] == 1
        for j in range(len(cl)):
            _check_bits(rx, j, want[j], "split %s" % split)
        runs.append(([list(rx.edges(j)) for j in range(len(cl))], got.stats["quiet_waves"], got.stats["total_waves"]))
        rx.close()
    print("launches split, quiet windows", form, quiet, runs[1][1], "of", runs[1][2])
    assert runs[0] == runs[1]
    if form in FORMS:
        assert (0 < runs[1][1] < runs[1][2]) if quiet else runs[1][1] == 0
