"""CPU-side tests of the burst spectra: the new symbols, the span rule (ookd_burst_spectra_span) and the host rule
ookd_suggest_burst_carriers against the Python restatement (tests/burst_spectra_contract.py) on designed tables and
on a few hundred random ones."""
import ctypes as C

import numpy as np
import pytest

from tests.burst_spectra_contract import (MAX_ROWS, MIN_SHARE, MIN_SPACING, N, as_tuples, bin_nu, py_suggest_burst_carriers,
                                          span_rule, spans_of)

import ookiedokie_amd as ok
from ookiedokie_amd import build as okbuild


@pytest.fixture(scope="session", autouse=True)
def built_lib():
    okbuild.build()
    return ok.lib()


def table(rows):
    """rows of (frames, total, dc, peak, bin) -> the dict of arrays Receiver.burst_spectra returns"""
    rows = list(rows)
    return dict(frames=np.array([r[0] for r in rows], dtype=np.uint64),
                total_power=np.array([r[1] for r in rows], dtype=np.float64),
                dc_power=np.array([r[2] for r in rows], dtype=np.float64),
                peak_power=np.array([r[3] for r in rows], dtype=np.float64),
                peak_bin=np.array([r[4] for r in rows], dtype=np.uint32))


def _same(t, **kw):
    """the library's suggestion equals the rule's; returns it"""
    got, of = ok.suggest_burst_carriers(t, min_share=kw.get("min_share", 0.0), min_spacing_bins=kw.get("min_spacing", 0),
                                        capacity=kw.get("capacity", 16))
    want, wof = py_suggest_burst_carriers(t, **kw)
    assert as_tuples(got) == want, (as_tuples(got), want)
    assert of.dtype == np.int32 and of.tolist() == wof, (of.tolist(), wof)
    for c in got:
        assert c.nu == bin_nu(c.bin) and -N // 2 <= c.bin < N // 2
    return got, of.tolist()


# ---- interface --------------------------------------------------------------------------------------------

def test_new_symbols_and_constants(built_lib):
    for name in ("ookd_rx_burst_spectra", "ookd_rx_get_burst_spectra", "ookd_rx_get_keyed_spectrum",
                 "ookd_rx_get_burst_spectra_info", "ookd_rx_burst_spectrum", "ookd_rx_burst_spectra_kernel_ms",
                 "ookd_burst_spectra_span", "ookd_suggest_burst_carriers"):
        assert hasattr(built_lib, name), name
    assert built_lib.ookd_rx_burst_spectra_kernel_ms(None) == 0.0
    assert C.sizeof(ok.BurstSpectrum) == 40 == ok.BURST_SPECTRUM_DTYPE.itemsize and C.sizeof(ok.BurstCarrierStruct) == 40
    assert C.sizeof(ok.BurstSpectraInfo) == 48
    header = open(ok.HEADER_PATH).read()
    assert "#define OOKD_BURST_MIN_SHARE 0.125" in header and ok.BURST_MIN_SHARE == MIN_SHARE == 0.125
    assert "#define OOKD_BURST_SPECTRA_MIN_SPAN 32" in header and "#define OOKD_BURST_SPECTRA_MAX_ROWS 8192" in header
    assert (ok.BURST_SPECTRA_MIN_SPAN, ok.BURST_SPECTRA_MAX_ROWS) == (32, MAX_ROWS)


# ---- the span rule ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("total", [0, 1, 1023, 1 << 18, (1 << 27) - 1, 1 << 27, (1 << 27) + 1, 1 << 28, 1 << 32, (1 << 40) + 5])
def test_span_chosen(total):
    want = span_rule(total)
    assert ok.burst_spectra_span(total) == want
    assert 2 * spans_of(total, want) <= MAX_ROWS and (want == 32 or 2 * spans_of(total, want // 2) > MAX_ROWS)
    if total <= 1 << 27:
        assert want == 32


@pytest.mark.parametrize("span", [1, 16, 31, 33, 48, 96, (1 << 20) + 1])
def test_span_invalid(span):
    assert span_rule(1 << 18, span) == "arg"
    with pytest.raises(ok.OokdError) as err:
        ok.burst_spectra_span(1 << 18, span)
    assert err.value.code == -1 and "power of two" in str(err.value)


def test_span_given_and_capacity():
    # a fabricated total: the check is the one ookd_rx_burst_spectra makes of the table's total
    for span in (32, 64, 1 << 12, 1 << 31):
        assert ok.burst_spectra_span(1 << 27, span) == span == span_rule(1 << 27, span)
    total = (1 << 27) + 1                   # 4097 spans of 32 frames: 8194 rows
    assert span_rule(total, 32) == "capacity" and span_rule(total, 64) == 64
    with pytest.raises(ok.OokdError) as err:
        ok.burst_spectra_span(total, 32)
    assert err.value.code == -5 and "smallest span that fits is 64" in str(err.value) and "8194" in str(err.value)
    assert ok.burst_spectra_span(total, 64) == 64
    with pytest.raises(ok.OokdError) as err:
        ok.burst_spectra_span(1 << 32, 512)
    assert err.value.code == -5 and "smallest span that fits is 1024" in str(err.value)
    assert ok.lib().ookd_burst_spectra_span(5, 0, None) == -1


# ---- the host rule -----------------------------------------------------------------------------------------

def test_designed_two_transmitters():
    # total 10, dc 1: off-DC 9; peaks 5.5 (share 0.61) and 5 on two bins far apart, one burst of noise (share 0.01)
    t = table([(3, 10.0, 1.0, 5.5, 205), (2, 10.0, 1.0, 5.0, N - 307), (4, 10.0, 1.0, 5.25, 205), (9, 10.0, 1.0, 0.09, 77),
               (1, 10.0, 1.0, 6.0, N - 306)])
    got, of = _same(t)
    # bin 205 weighs 10.75; bin -306 weighs 6 and takes its neighbour -307 with it
    assert [(c.bin, c.bursts, c.frames) for c in got] == [(205, 2, 7), (-306, 2, 3)] and of == [0, 1, 0, -1, 1]
    assert got[0].power == 5.5 + 5.25 and got[1].power == 5.0 + 6.0
    # burst 3 qualifies at a share of 0.005 and becomes a carrier of its own, the weakest
    got, of = _same(t, min_share=0.005)
    assert [c.bin for c in got] == [205, -306, 77] and of == [0, 1, 0, 2, 1]


def test_ties_go_to_the_lowest_bin():
    t = table([(1, 4.0, 0.0, 2.0, 700), (1, 4.0, 0.0, 2.0, 100), (1, 4.0, 0.0, 2.0, 400)])
    got, of = _same(t)
    assert [c.bin for c in got] == [100, 400, 700 - N] and of == [2, 0, 1]
    # equal weights inside one neighbourhood: the lowest k is emitted and takes the other
    t = table([(1, 4.0, 0.0, 1.0, 110), (2, 4.0, 0.0, 1.0, 100)])
    got, of = _same(t)
    assert [(c.bin, c.bursts, c.frames, c.power) for c in got] == [(100, 2, 3, 2.0)] and of == [0, 0]


def test_circular_neighbourhoods():
    # bins 1023, 0 and 1 never carry a peak: the neighbours across the seam are 2 and 1022
    t = table([(1, 4.0, 0.0, 3.0, 2), (1, 4.0, 0.0, 2.0, N - 2), (1, 4.0, 0.0, 1.0, N - 30), (1, 4.0, 0.0, 1.5, N - 31)])
    got, of = _same(t)
    assert [(c.bin, c.bursts) for c in got] == [(2, 3), (-31, 1)] and of == [0, 0, 0, 1]
    got, of = _same(t, min_spacing=3)
    assert [(c.bin, c.bursts) for c in got] == [(2, 1), (-2, 1), (-31, 2)] and of == [0, 1, 2, 2]
    got, of = _same(t, min_spacing=4)
    assert [(c.bin, c.bursts) for c in got] == [(2, 2), (-31, 2)] and of == [0, 0, 1, 1]
    # a spacing of half the bins or more reaches every bin
    got, of = _same(t, min_spacing=512)
    assert [(c.bin, c.bursts) for c in got] == [(2, 4)] and of == [0, 0, 0, 0]
    # a dead bin between two live ones is not a member of the later carrier
    t = table([(1, 4.0, 0.0, 5.0, 100), (1, 4.0, 0.0, 1.0, 120), (1, 4.0, 0.0, 4.0, 140)])
    got, of = _same(t, min_spacing=20)
    assert [(c.bin, c.bursts) for c in got] == [(100, 2), (140, 1)] and of == [0, 0, 1]


def test_capacity():
    t = table([(1, 4.0, 0.0, 3.0, 100), (1, 4.0, 0.0, 2.0, 300), (1, 4.0, 0.0, 1.0, 500)])
    got, of = _same(t, capacity=2)
    assert [c.bin for c in got] == [100, 300] and of == [0, 1, -1]
    got, of = _same(t, capacity=1)
    assert of == [0, -1, -1]
    got, of = ok.suggest_burst_carriers(t, capacity=0)
    assert got == [] and of.tolist() == [-1, -1, -1]


def test_bursts_that_do_not_qualify():
    t = table([(0, 0.0, 0.0, 0.0, 0),               # no frames
               (0, 4.0, 0.0, 3.0, 100),             # no frames, whatever else it says
               (2, 3.0, 3.0, 1.0, 200),             # total = dc
               (2, 3.0, 3.5, 1.0, 300),             # total < dc
               (2, 8.0, 0.0, 1.0, 400),             # on the boundary: 1 >= 0.125 * 8 qualifies
               (2, 8.0, 0.0, np.nextafter(1.0, 0.0), 600),      # just below it
               (2, 9.0, 1.0, 1.0, 800)])            # on the boundary with a DC term
    got, of = _same(t)
    assert [c.bin for c in got] == [400, 800 - N] and of == [-1, -1, -1, -1, 0, -1, 1]
    got, of = _same(table([]))
    assert got == [] and of == []
    got, of = _same(t, min_share=0.5)
    assert got == [] and of == [-1] * 7


def test_argument_errors():
    lib = ok.lib()
    s = (ok.BurstSpectrum * 2)()
    out = (ok.BurstCarrierStruct * 2)()
    count = C.c_uint32(7)
    of = (C.c_int32 * 2)()
    assert lib.ookd_suggest_burst_carriers(None, 2, 0.0, 0, out, 2, C.byref(count), of) == -1
    assert "NULL" in ok.last_error()
    assert lib.ookd_suggest_burst_carriers(s, 2, 0.0, 0, out, 2, None, of) == -1
    assert lib.ookd_suggest_burst_carriers(s, 2, 0.0, 0, None, 2, C.byref(count), of) == -1
    assert lib.ookd_suggest_burst_carriers(s, 2, -0.5, 0, out, 2, C.byref(count), of) == -1
    assert "min_share" in ok.last_error()
    assert lib.ookd_suggest_burst_carriers(s, 2, float("nan"), 0, out, 2, C.byref(count), of) == -1
    s[1].peak_bin = N
    assert lib.ookd_suggest_burst_carriers(s, 2, 0.0, 0, out, 2, C.byref(count), of) == -1
    assert "peak_bin" in ok.last_error()
    s[1].peak_bin = N - 1
    # what may be NULL: the table of no bursts, out with no capacity, carrier_of_burst
    assert lib.ookd_suggest_burst_carriers(None, 0, 0.0, 0, None, 0, C.byref(count), None) == 0 and count.value == 0
    assert lib.ookd_suggest_burst_carriers(s, 2, 0.0, 0, out, 2, C.byref(count), None) == 0 and count.value == 0


@pytest.mark.parametrize("seed", range(6))
def test_random_tables(seed):
    rng = np.random.default_rng(1000 + seed)
    for _ in range(50):
        nb = int(rng.integers(0, 60))
        homes = rng.integers(2, N - 1, size=int(rng.integers(1, 6)))
        rows = []
        for _ in range(nb):
            k = int((homes[rng.integers(0, homes.size)] + rng.integers(-40, 41) - 2) % (N - 3)) + 2
            total = float(rng.integers(1, 1000))
            dc = float(rng.integers(0, 3)) * total / 2.0                    # 0, half, or all of it
            peak = float(rng.integers(0, 9)) / 8.0 * max(total - dc, 0.0)   # shares of k / 8: the boundary is met
            rows.append((int(rng.integers(0, 4)), total, dc, peak, k))
        kw = dict(min_share=float(rng.choice([0.0, 0.125, 0.5, 1.0])), min_spacing=int(rng.choice([0, 1, 7, 32, 200, 600])),
                  capacity=int(rng.choice([1, 2, 16])))
        got, of = ok.suggest_burst_carriers(table(rows), kw["min_share"], kw["min_spacing"], kw["capacity"])
        want, wof = py_suggest_burst_carriers(table(rows), **kw)
        assert as_tuples(got) == want and of.tolist() == wof, (seed, rows, kw)
