"""The pulse moments on the GPU (ookd_rx_run_moments; run_moments_kernel in run_moments.hip).  The sums are integers
taken modulo 2^64, exact and independent of any order, so every comparison is equality of int64 values against the
numpy restatement of the contract (tests/run_moments_contract.py) over `rx.edges(c)` and the reference's -- or the
tuned contract's -- complex filter output of the capture zero padded to whole buffers.

The seams (S1 .. S10, tests/run_moment_seams_inputs.py): without a filter the captures hold the layouts of the levels'
seam catalogue with an I and a Q of its own in every on sample; behind a filter the edges are shifted onto the seams
(filtered_capture of tests/run_level_seams_inputs.py), the pulses turning slowly so that both lag sums are exercised.
A multiple of 1024 outputs is a tile seam of every filter whatever tile the pass reports: its tile is a power of two up
to 1024.  Every capture is a few thousand to 133 000 samples: each test takes seconds."""
import subprocess

import numpy as np
import pytest

from tests import run_level_seams_inputs as S
from tests import run_moment_seams_inputs as M
from tests.helpers import edges_of, golden_path
from tests.run_levels_contract import (RATE, SPB, THR, SEAM_NU, assert_targets, oracle_fir, padded, ref_edges,
                                       seam_tuned, tiles_filtered_of)
from tests.run_moments_contract import (TWO_NU, TWO_TUNE, message_carriers_of, moments_of, moved_seam, oracle_y,
                                        two_carrier_capture)
from tests.tuned_contract import contract_rx, lib_stages, moved

pytestmark = pytest.mark.gpu

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
def plain(ok):
    """unfiltered contexts by (samples, samples per buffer, sample format), shared by the tests of this module"""
    made = {}

    def get(n, spb, fmt="sc16q11"):
        if (n, spb, fmt) not in made:
            made[n, spb, fmt] = ok.Receiver(None, None, max_samples=n, samples_per_buffer=spb, threshold=THR,
                                            edge_capacity=n + 64, sample_format=fmt)
        return made[n, spb, fmt]
    yield get
    for rx in made.values():
        rx.close()


def lib_filter(ok, shape):
    if shape == "three":
        return ok.Filter.from_stages(S.three_stages())
    return ok.Filter.load(golden_path("filters", shape))


def check(rx, capture, y, clean=False, what="", decimation=None):
    """one capture's answer against the restatement over its own edge list; -> (the answer, the edges)"""
    n_out = rx.stats()["decimated_samples"]
    e = rx.edges(capture, clean)
    mo = rx.run_moments(capture, clean)
    y = np.ascontiguousarray(y, dtype=np.float32).reshape(-1, 2)
    assert y.shape[0] == n_out, (what, y.shape, n_out)
    want = moments_of(y, e, n_out)
    for k, key in enumerate(("power", "lag_re", "lag_im")):
        assert mo[key].dtype == np.int64 and mo[key].shape == (want.shape[0],), (what, key)
        bad = np.nonzero(mo[key] != want[:, k])[0]
        assert bad.size == 0, (what, key, bad[:6].tolist(), mo[key][bad[:6]].tolist(), want[bad[:6], k].tolist())
    assert mo["num_runs"] == (e.size + 1) // 2, what
    tile = mo["tile_outputs"]
    assert tile >= 1 and tile & (tile - 1) == 0 and tile <= 1024, what
    assert mo["tiles_total"] == -(-n_out // tile), what
    assert mo["tiles_filtered"] == tiles_filtered_of(e, n_out, tile), what
    if decimation is not None:
        assert mo["decimation"] == decimation, what
    return mo, e


# ------------------------------------------------------------------------------- 1. no filter: S1 - S6, S9, S10 ----

NO_FILTER = M.seam_cases() + M.dense_cases() + [M.long_run_case()]


@pytest.mark.parametrize("case", NO_FILTER, ids=lambda c: c.name)
def test_no_filter_seams(plain, oracle, case):
    iq = M.lay_hashed(case)
    rx = plain(case.n, case.spb)
    rx.rx(iq)
    assert rx.moments_kernel_ms == 0.0                          # nobody has asked about this run yet
    mo, e = check(rx, 0, oracle_y(oracle, None, padded(iq, case.spb)), what=case.name, decimation=1)
    assert mo["tile_outputs"] == S.T, "the cases are laid for tiles of 1024 outputs"
    assert e.tolist() == S.edges_of_case(case), case.name
    assert rx.moments_kernel_ms > 0.0
    assert (mo["power"] > 0).all()
    if not case.name.startswith(("dense-even", "dense-odd", "seams-singles")):
        assert mo["lag_re"].any() and mo["lag_im"].any()
    if case.name.startswith(("dense-even", "dense-odd")):       # S9: runs of one output, 32 in a wave and 512 in a tile
        assert mo["num_runs"] >= case.n // 2 and not mo["lag_re"].any() and not mo["lag_im"].any()
    if case.name.startswith("long_run"):                        # S10
        assert mo["num_runs"] == 1 and mo["tiles_filtered"] == 71


@pytest.mark.parametrize("fmt", ["cs8", "cu8"])
def test_8bit_seams_equal_the_widened_capture(plain, oracle, fmt):
    for case in M.seam_cases()[:3] + M.dense_cases()[2:]:
        v = M.lay_hashed(case, M.MIN_RAIL8, M.SPAN8)
        raw = v.astype(np.int8) if fmt == "cs8" else (v + 128).astype(np.uint8)
        wide = (v * 16).astype(np.int16)
        rx8 = plain(case.n, case.spb, fmt)
        rx8.rx(raw)
        mo, e = check(rx8, 0, oracle_y(oracle, None, padded(wide, case.spb)), what="%s %s" % (case.name, fmt))
        assert e.tolist() == S.edges_of_case(case)


def test_8bit_behind_a_filter(ok, oracle):
    iq, n, spb, targets = moved_seam(oracle, "fs128_fs16_dec4", "a")
    v = np.clip(np.rint(iq.astype(np.float64) / 16.0), -128, 127).astype(np.int16)
    wide = (v * 16).astype(np.int16)
    y = oracle_y(oracle, oracle_fir(oracle, "fs128_fs16_dec4"), padded(wide, spb))
    for fmt in ("cs8", "cu8"):
        raw = v.astype(np.int8) if fmt == "cs8" else (v + 128).astype(np.uint8)
        rx = ok.Receiver(lib_filter(ok, "fs128_fs16_dec4"), None, max_samples=n, samples_per_buffer=spb, threshold=THR,
                         sample_format=fmt)
        rx.rx(raw)
        mo, e = check(rx, 0, y, what=fmt, decimation=4)
        assert mo["num_runs"] >= 3
        rx.close()


# ---------------------------------------------------------------------------- 2. behind a filter: seams, S7 ----

@pytest.mark.parametrize("which", sorted(S.FILTERED_TARGETS))
@pytest.mark.parametrize("shape", sorted(S.SHAPE_D))
def test_filtered_seams(ok, oracle, shape, which):
    """an untuned context on fs32_fs4, the multi-stage D = 4 filter and the three-stage shape: a rise and a fall on a
    tile seam and on a block seam, a rise at the last output, a run open to it"""
    iq, n, spb, targets = moved_seam(oracle, shape, which)
    rx = ok.Receiver(lib_filter(ok, shape), None, max_samples=n, samples_per_buffer=spb, threshold=THR)
    rx.rx(iq)
    y = oracle_y(oracle, oracle_fir(oracle, shape), padded(iq, spb))
    mo, e = check(rx, 0, y, what="%s %s" % (shape, which), decimation=S.SHAPE_D[shape])
    assert rx.stats()["decimated_samples"] == S.FILTERED_OUT and S.T % mo["tile_outputs"] == 0
    assert_targets(e, S.FILTERED_OUT, targets, shape)
    assert mo["lag_re"].any() and mo["lag_im"].any()
    ms = rx.moments_kernel_ms
    assert ms > 0.0
    again = rx.run_moments(0)                                   # the same run asked about twice launches nothing
    assert rx.moments_kernel_ms == ms and again["power"].tolist() == mo["power"].tolist()
    rx.close()


def test_run_open_through_the_padding(ok, oracle):
    """S7: n is no multiple of the buffer and the last run is on up to n_out, PAD outputs into the zero padding"""
    iq, n, spb = M.open_pad_capture()
    rx = ok.Receiver(lib_filter(ok, "fs32_fs4"), None, max_samples=n, samples_per_buffer=spb, threshold=THR)
    rx.rx(iq)
    mo, e = check(rx, 0, oracle_y(oracle, oracle_fir(oracle, "fs32_fs4"), padded(iq, spb)), what="open pad", decimation=1)
    n_out = rx.stats()["decimated_samples"]
    assert n_out == n + M.PAD and e.size == 3 and int(e[2]) < n
    rx.close()


NARROW_TAPS = 3270                  # one stage of decimation 1 whose tile + 1 outputs leave the pass a tile of 8


def test_narrow_tiles_and_the_grid_stride_loop(ok, oracle):
    """a tile narrower than a wave (most lanes of segment_add hold nothing, and the extra output is a ninth of the
    work), in a batch with at least twice as many chunks per capture as workgroups can be launched for it: every
    workgroup walks a second chunk with the table and the count of filtered tiles it used for the first"""
    import torch
    caps = S.GRID_CAPTURES
    stages = [(1, S.window(NARROW_TAPS))]
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    bound, n = S.grid_stride_samples(cus, 8)
    stride = n + 256
    fir = oracle.make_fir(stages)
    contents = [moved(S.grid_stride_capture(n, k), 1.0 / 9973.0) for k in range(S.GRID_CONTENTS)]
    ys = [oracle_y(oracle, fir, c) for c in contents]
    host = np.zeros((caps, 2 * stride), dtype=np.int16)
    host[:, 0::2] = 30000
    for c in range(caps):
        host[c, :2 * n] = contents[S.grid_stride_content(c)]
    rx = ok.Receiver(ok.Filter.from_stages(stages), None, max_samples=n, max_captures=caps, threshold=S.GRID_THR)
    dev_t = torch.from_numpy(host).cuda()
    rx.rx_device(dev_t.data_ptr(), n, num_captures=caps, stride=stride)
    mo = rx.run_moments(0)
    assert mo["tile_outputs"] == 8
    chunks = -(-mo["tiles_total"] // 64)
    assert chunks >= 2 * bound and bound >= -(-cus * 4 // caps), (chunks, bound, cus)      # (4 workgroups of 40 KiB a CU)
    filtered = []
    for c in range(caps):
        mo, e = check(rx, c, ys[S.grid_stride_content(c)], what="capture %d" % c, decimation=1)
        assert int(e[0]) < 64 * 8 and e.size == 5, (c, e)           # on in the first chunk and in the last
        assert mo["lag_im"].any()
        filtered.append(mo["tiles_filtered"])
    assert len(set(filtered[:S.GRID_CONTENTS])) == S.GRID_CONTENTS
    rx.close()


# -------------------------------------------------------------------------------------- 3. tuned and carriers ----

@pytest.mark.parametrize("which", sorted(S.FILTERED_TARGETS))
def test_tuned_seams(ok, which):
    f = lib_filter(ok, "fs32_fs4")
    iq, n, spb, targets, stages = seam_tuned(f, which)
    rx = ok.Receiver(f, None, max_samples=n, samples_per_buffer=spb, threshold=THR, tune=SEAM_NU)
    rx.rx(iq)
    mo, e = check(rx, 0, contract_rx(iq, stages, THR, spb)[1], what="tuned %s" % which, decimation=1)
    assert_targets(e, S.FILTERED_OUT, targets, "tuned")
    # the pulses sit on the carrier: their phase step is SEAM_NU, a fifth of a turn per output
    at = np.arctan2(mo["lag_im"].astype(np.float64), mo["lag_re"].astype(np.float64)) / (2 * np.pi)
    long_runs = np.diff(np.append(e, S.FILTERED_OUT))[0::2][:at.size] > 50
    assert long_runs.any() and np.abs(at[long_runs] - SEAM_NU).max() < 1e-3
    rx.close()


def test_carrier_context_with_two_carriers(ok):
    from tests.test_gpu_run_levels import _two_carriers
    iq, carriers = _two_carriers()
    n = iq.size // 2
    f = ok.Filter.load(golden_path("filters", "fs32_fs4"))
    rx = ok.Receiver(f, None, max_samples=n, carriers=[carriers[0][0], carriers[1]], threshold=carriers[0][1])
    rx.rx(iq)
    for k, (nu, thr) in enumerate(carriers):
        y = contract_rx(iq, lib_stages(f, nu), thr)[1]
        mo, e = check(rx, k, y, what="carrier %d" % k, decimation=1)
        assert e.size == (228, 136)[k]
        one = ok.Receiver(f, None, max_samples=n, threshold=thr, tune=nu)
        one.rx(iq)
        mo1, e1 = check(one, 0, y, what="tuned to carrier %d" % k)
        assert e1.tolist() == e.tolist()
        for key in ("power", "lag_re", "lag_im"):
            assert mo1[key].tolist() == mo[key].tolist()
        one.close()
    with pytest.raises(ok.OokdError) as err:
        rx.run_moments(2)
    assert err.value.code == -1
    rx.close()


# -------------------------------------------------------------------------------------- 4. batched runs: S8 ----

def test_batch_where_a_capture_ends_on_and_the_next_begins_on(ok, oracle):
    """S8: nine captures, odd and even lists; no pair joins the last output of one capture and output 0 of the next"""
    import torch
    cases = S.parity_cases()
    caps, n, spb, stride = len(cases), S.PARITY_N, S.PARITY_SPB, S.PARITY_N + 500
    host = np.zeros((caps, 2 * stride), dtype=np.int16)
    host[:, 0::2] = 30000                                       # the gaps are loud
    host[:, 1::2] = -20000
    iqs = [M.lay_hashed(c) for c in cases]
    for c in range(caps):
        host[c, :2 * n] = iqs[c]
    rx = ok.Receiver(None, None, max_samples=n, max_captures=caps, samples_per_buffer=spb, threshold=THR)
    dev_t = torch.from_numpy(host).cuda()
    rx.rx_device(dev_t.data_ptr(), n, num_captures=caps, stride=stride)
    ms = None
    for c in (4, 8, 0, 3, 7, 1, 6, 2, 5):
        mo, e = check(rx, c, oracle_y(oracle, None, padded(iqs[c], spb)), what="capture %d" % c)
        assert e.tolist() == S.edges_of_case(cases[c])
        ms = ms or rx.moments_kernel_ms
        assert ms > 0.0 and rx.moments_kernel_ms == ms          # one pass answered all captures
    m = S.PARITY_SHORT                                          # a shorter run of two captures on the same context
    rx.rx_device(dev_t.data_ptr(), m, num_captures=2, stride=stride)
    assert rx.moments_kernel_ms == 0.0
    for c in (1, 0):
        mo, e = check(rx, c, oracle_y(oracle, None, padded(iqs[c][:2 * m], spb)), what="short capture %d" % c)
        assert e.size % 2 == 1
    with pytest.raises(ok.OokdError):
        rx.run_moments(2)
    rx.close()


def test_batch_of_three_behind_a_filter(ok, oracle):
    import torch
    a, n, spb, _ = moved_seam(oracle, "fs32_fs4", "a")
    b = moved_seam(oracle, "fs32_fs4", "b")[0]                  # ends on: open to n_out
    c = b.copy()
    c[1::2] = -c[1::2]                                          # the same pulses turning the other way
    iqs = [b, c, a]
    stride = n + 700
    host = np.zeros((3, 2 * stride), dtype=np.int16)
    host[:, 0::2] = 30000
    for k in range(3):
        host[k, :2 * n] = iqs[k]
    rx = ok.Receiver(lib_filter(ok, "fs32_fs4"), None, max_samples=n, max_captures=3, samples_per_buffer=spb, threshold=THR)
    dev_t = torch.from_numpy(host).cuda()
    rx.rx_device(dev_t.data_ptr(), n, num_captures=3, stride=stride)
    fir = oracle_fir(oracle, "fs32_fs4")
    got = [check(rx, k, oracle_y(oracle, fir, padded(iqs[k], spb)), what="capture %d" % k)[0] for k in (2, 0, 1)]
    assert got[1]["lag_im"].tolist() == (-got[2]["lag_im"]).tolist() and got[1]["lag_re"].tolist() == got[2]["lag_re"].tolist()
    rx.close()


# ------------------------------------------------------------------------------------------ 5. cleaned lists ----

GLITCHED = S.Case("glitched", 3 * 500 * 8 - 100, 500,
                  [(1000, 1050, 1000), (1053, 1100, 1053), (3000, 3400, 3000), (5000, 5040, 5000), (5043, 5100, 5043),
                   (9000, 9700, 9000)], [], 0)


@pytest.mark.parametrize("debounced", [False, True], ids=["clean_edges", "debounced-context"])
def test_clean_list(ok, oracle, debounced):
    iq = M.lay_hashed(GLITCHED)
    n = GLITCHED.n
    y = oracle_y(oracle, None, padded(iq, GLITCHED.spb))
    rx = ok.Receiver(None, None, max_samples=n, samples_per_buffer=GLITCHED.spb, threshold=THR, min_off=5 if debounced else 0)
    rx.rx(iq)
    if not debounced:
        with pytest.raises(ok.OokdError) as err:
            rx.run_moments(0, clean=True)
        assert err.value.code == -1 and "cleaned list" in str(err.value)
        assert rx.clean_edges(0, 5)[0]["deleted"] == [2, 0]
    raw, e_raw = check(rx, 0, y, what="raw list")
    mo, e = check(rx, 0, y, clean=True, what="cleaned list")
    assert e_raw.size == 12 and e.tolist() == [1000, 1100, 3000, 3400, 5000, 5100, 9000, 9700]
    # a swallowed dropout: the power of both halves, and pairs with the zero outputs between them, which add nothing
    assert mo["power"][0] == raw["power"][0] + raw["power"][1] and mo["lag_re"][0] == raw["lag_re"][0] + raw["lag_re"][1]
    ms = rx.moments_kernel_ms
    rx.clean_edges(0, 2000)                                     # other minimums on the same run: another cleaned list
    mo2, e2 = check(rx, 0, y, clean=True, what="cleaned again")
    assert e2.tolist() == [1000, 5100, 9000, 9700] and mo2["num_runs"] == 2
    at = ok.RxResult(np.zeros(2, np.uint32), np.array([6000, 9500], np.uint64), np.zeros((2, 0), np.uint8), {})
    got = rx.message_carriers(at, pulses=3, clean=True)
    want = message_carriers_of(e2, mo2, [6000, 9500], 3, 1, 0.0, rx.stats()["decimated_samples"])
    assert got["outputs"].tolist() == [4100, 700] == [w[3] for w in want]
    assert got["carrier"] == pytest.approx([w[0] for w in want], abs=1e-15)
    rx.clean_edges(0, 5)                                        # ... and back
    mo3, e3 = check(rx, 0, y, clean=True, what="cleaned a third time")
    assert e3.tolist() == e.tolist() and mo3["power"].tolist() == mo["power"].tolist()
    assert rx.moments_kernel_ms == ms                           # the raw list's pass untouched throughout
    rx.close()


# ----------------------------------------------------------------------------------------------- 6. refusals ----

def test_refusals(ok, vectors):
    import torch
    from tests.pulse_contract import golden_iq
    n = 1 << 15
    i = np.zeros(n // 2, dtype=np.int16)
    for k in (10, 11, 12):
        i[k::6] = 2047
    iq = np.zeros(n, dtype=np.int16)
    iq[0::2] = i
    rx = ok.Receiver(None, None, max_samples=n, threshold=THR, edge_capacity=256)
    with pytest.raises(ok.OokdError) as e:
        rx.run_moments(0)
    assert e.value.code == -1 and "no finished run" in str(e.value)
    with pytest.raises(ok.OokdError) as e:                      # an overflowed edge list
        rx.rx(iq)
    assert e.value.code == -5
    with pytest.raises(ok.OokdError) as e:
        rx.run_moments(0)
    assert e.value.code == -5 and "overflow" in str(e.value)
    assert rx.moments_kernel_ms == 0.0
    rx.close()
    rx = ok.Receiver(None, None, max_samples=n, threshold=THR, edge_capacity=n)
    dev_t = torch.from_numpy(iq).cuda()
    rx.submit_device(dev_t.data_ptr(), iq.size // 2)            # a run in flight
    with pytest.raises(ok.OokdError) as e:
        rx.run_moments(0)
    assert e.value.code == -1 and "ookd_rx_wait first" in str(e.value)
    rx.wait()
    assert rx.run_moments(0)["num_runs"] > 100
    with pytest.raises(ok.OokdError) as e:
        rx.run_moments(1)
    assert e.value.code == -1 and "capture 1 of 1" in str(e.value)
    rx.shard_begin(dev_t.data_ptr(), iq.size // 2, None, True, None)
    with pytest.raises(ok.OokdError) as e:
        rx.run_moments(0)
    assert e.value.code == -1 and "shard" in str(e.value)
    rx.rx(iq)                                                   # a whole run on the same context is answered again
    assert rx.run_moments(0)["num_runs"] > 100
    rx.rx(np.zeros(0, dtype=np.int16))                          # a run of no samples launches nothing
    mo = rx.run_moments(0)
    assert mo["num_runs"] == 0 and mo["tiles_total"] == 0 and rx.moments_kernel_ms == 0.0
    rx.close()
    g = vectors["G1"]                                           # a pipelined run
    giq = golden_iq(vectors, "G1")
    f = ok.Filter.load(golden_path("filters", g["filter"]))
    d = ok.Device.load(golden_path("devices", g["device"]), RATE // f.total_decimation)
    rx = ok.Receiver(f, d, max_samples=giq.size // 2, pipeline_chunk_samples=4 * SPB)
    res = rx.rx(giq)
    assert res.stats["pipeline_chunks"] >= 2
    with pytest.raises(ok.OokdError) as e:
        rx.run_moments(0)
    assert e.value.code == -1 and "pipelined" in str(e.value)
    rx.close()
    long_taps = np.full(11000, 1.0 / 11000.0, dtype=np.float32)   # a filter the pass's LDS window cannot hold
    rx = ok.Receiver(ok.Filter.from_stages([(1, long_taps)]), None, max_samples=SPB, threshold=THR)
    rx.rx(np.zeros(2 * SPB, dtype=np.int16))
    with pytest.raises(ok.OokdError) as e:
        rx.run_moments(0)
    assert e.value.code == -1 and "does not fit the kernel's LDS window" in str(e.value)
    rx.close()


# ------------------------------------------------------------------ 7. two transmitters 6 kHz apart, end to end ----

@pytest.mark.parametrize("filt", ["fs32_fs4", "fs128_fs16_dec4"])
def test_two_transmitters_end_to_end(ok, vectors, filt):
    """the capture of the host test's T3 through a context tuned between the transmitters: the run is what it was
    before anybody asked, the sums are the contract's, and every message is within 1.5 kHz of its own transmitter"""
    g, iq, half = two_carrier_capture(vectors)
    f = ok.Filter.load(golden_path("filters", filt))
    D = f.total_decimation
    d = ok.Device.load(golden_path("devices", g["device"]), RATE // D)
    rx = ok.Receiver(f, d, max_samples=iq.size // 2, threshold=THR, tune=TWO_TUNE, pipeline=False)
    res = rx.rx(iq)
    assert len(res.msg_samples) == 6 and res.stats["num_errors"] == 0
    before = (rx.result(), rx.edges(0), rx.pulse_hist(0), rx.stats(), rx.bits(0), rx.run_levels(0))
    mo, e = check(rx, 0, contract_rx(iq, lib_stages(f, TWO_TUNE), THR)[1], what=filt, decimation=D)
    got = rx.message_carriers(res)
    after = (rx.result(), rx.edges(0), rx.pulse_hist(0), rx.stats(), rx.bits(0), rx.run_levels(0))
    assert (after[0].msg_samples == before[0].msg_samples).all() and (after[0].payloads == before[0].payloads).all()
    assert after[0].stats == before[0].stats and after[1].tolist() == before[1].tolist()
    for key in before[2]:
        assert np.array_equal(after[2][key], before[2][key]), key
    assert after[3] == before[3] and np.array_equal(after[4], before[4])
    assert after[5]["peaks"].tolist() == before[5]["peaks"].tolist()
    want = message_carriers_of(e, mo, res.msg_samples, d.num_bits + 2, D, TWO_TUNE, rx.stats()["decimated_samples"])
    assert got["outputs"].tolist() == [w[3] for w in want]
    for k, key in enumerate(("carrier", "mean_power", "coherence")):
        assert got[key] == pytest.approx([w[k] for w in want], rel=1e-12, abs=1e-15), key
    own = np.where(res.msg_samples < half // D, TWO_NU[0], TWO_NU[1])
    assert (np.abs(got["carrier"] - own) * RATE <= 1500.0).all() and (got["coherence"] >= 0.99).all()
    rx.close()


def test_c_example_carriers(ok, vectors, tmp_path):
    """examples/ookd_rx.c --carriers on the same capture: stdout is what it is without the option, the level lines are
    untouched, and stderr holds two groups of carriers 6 kHz apart"""
    from tests.test_host import _build_c_example
    exe = _build_c_example(tmp_path)
    g, iq, _ = two_carrier_capture(vectors)
    cap = tmp_path / "two.sc16q11"
    iq.tofile(str(cap))
    args = ["--tune", "603000", str(cap), golden_path("devices", g["device"]), golden_path("filters", "fs32_fs4"), str(RATE), "csv"]
    plain = subprocess.run([exe, "--levels"] + args, capture_output=True, text=True, timeout=120)
    both = subprocess.run([exe, "--levels", "--carriers"] + args, capture_output=True, text=True, timeout=120)
    assert plain.returncode == 0 and both.returncode == 0, (plain.stderr, both.stderr)
    fields = lambda text: [ln.split(",", 1)[1:] for ln in text.split("\n")]         # (the first is the wall clock)
    assert fields(both.stdout) == fields(plain.stdout) and len(plain.stdout.strip().split("\n")) == 7
    assert "carrier " not in plain.stderr
    levels = lambda text: [ln for ln in text.split("\n") if ln.startswith("level ")]
    assert levels(both.stderr) == levels(plain.stderr) and len(levels(plain.stderr)) == 6
    f = ok.Filter.load(golden_path("filters", "fs32_fs4"))
    d = ok.Device.load(golden_path("devices", g["device"]), RATE)
    rx = ok.Receiver(f, d, max_samples=iq.size // 2, threshold=THR, tune=603000.0 / RATE)
    res = rx.rx(iq)
    mc = rx.message_carriers(res)
    rx.close()
    want = ["carrier 0 %d %.1f %.2f %.4f" % (s, c * RATE, 10.0 * np.log10(p), k)
            for s, c, p, k in zip(res.msg_samples, mc["carrier"], mc["mean_power"], mc["coherence"])]
    got = [ln for ln in both.stderr.split("\n") if ln.startswith("carrier ")]
    assert got == want and len(got) == 6
    hz = [float(ln.split()[3]) for ln in got]
    assert max(hz[:3]) - min(hz[:3]) < 300 and max(hz[3:]) - min(hz[3:]) < 300
    assert abs(np.mean(hz[3:]) - np.mean(hz[:3]) - 6000.0) < 300
