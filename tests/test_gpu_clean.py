"""Edge cleaning on the GPU (ookd_rx_clean_edges; the three kernels of clean.hip) and the two clean readers.  The
cleaned list is an exact function of a run's edge list and the two minimums, so every comparison is equality against
the restatement of the rule (tests/clean_contract.py) fed with `rx.edges(c)`; the readers are compared with the
restatements of their own contracts (tests/pulse_contract.py, tests/symbol_contract.py) fed with the cleaned list."""
import numpy as np
import pytest

from tests.clean_contract import assert_invariants, clean_of, clean_of_long, info_of
from tests.helpers import golden_path
from tests.pulse_contract import RATE, SPB, THR, assert_same_hist, golden_iq, hist_of
from tests.symbol_contract import SIDE, SYNC, ZERO, ONE, assert_same_survey, py_chain, survey_of
from tests.tuned_contract import golden_capture, moved

pytestmark = pytest.mark.gpu

ON = 2047                       # I of an "on" sample (no filter: |x| = 2047 / 2048 against the threshold 0.1)
T = 2048                        # edges of a tile (kCleanTile)
LANE = 8                        # tile aggregates a lane of the aggregate scan folds (kCleanScanPerThread)
STEP = 256 * LANE               # tiles the aggregate scan takes per step

# a class table and roles for the symbol reader over lists of runs of 1 .. 11 samples
TABLE = dict(lower=[[1, 4, 8], [1, 5]], upper=[[3, 7, 11], [4, 11]])
ROLES = np.zeros((SIDE, SIDE), dtype=np.uint8)
ROLES[0, 0], ROLES[0, 1], ROLES[1, 2] = ZERO, ONE, SYNC


@pytest.fixture(scope="module")
def ok():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from ookiedokie_amd import build as okbuild
    okbuild.build()
    import ookiedokie_amd as okm
    okm.lib()
    return okm


def capture_of(closed, lead=5, n=None):
    """(I,Q, edges) of a capture without a filter whose edge list has len(closed) + 1 edges: `lead` off samples, the
    closed runs of the given lengths, on first, and the open run behind the last edge up to the end of the capture, a
    whole number of buffers.  closed = None: no edge at all."""
    used = lead + (int(np.sum(closed)) if closed is not None else 0)
    if n is None:
        n = -(-(used + 1) // SPB) * SPB
    assert n % SPB == 0 and used < n
    i = np.zeros(n, dtype=np.int16)
    e = np.zeros(0, dtype=np.uint64)
    if closed is not None:
        runs = np.append(np.asarray(closed, dtype=np.int64), n - used)
        lv = np.zeros(runs.size, dtype=np.int16)
        lv[0::2] = ON
        i[lead:] = np.repeat(lv, runs)
        e = (lead + np.concatenate([[0], np.cumsum(runs[:-1])])).astype(np.uint64)
    iq = np.zeros(2 * n, dtype=np.int16)
    iq[0::2] = i
    return iq, e


def random_capture(E, rng, n=None):
    if E == 0:
        return capture_of(None, n=n)
    return capture_of(rng.integers(1, 12, size=E - 1), lead=int(rng.integers(0, 9)), n=n)


def check(rx, capture, mins, want_edges=None, what=""):
    """the capture's cleaned list and counts (rx.clean_edges(*mins) has run) against the restatement over its own
    edge list; returns the cleaned list"""
    e = rx.edges(capture)
    if want_edges is not None:
        assert e.tolist() == np.asarray(want_edges).tolist(), what
    want, _ = clean_of(e, *mins)
    got = rx.edges(capture, clean=True)
    assert got.dtype == np.uint64 and got.tolist() == want.tolist(), (what, mins, e.size, got.size, want.size)
    return got


def clean_and_check(rx, mins, want_edges=None, what="", captures=1):
    infos = rx.clean_edges(*mins)
    assert len(infos) == captures, what
    out = []
    for c in range(captures):
        got = check(rx, c, mins, want_edges if captures == 1 else None, "%s capture %d" % (what, c))
        assert infos[c] == info_of(rx.edges(c), *mins), (what, c, mins)
        assert_invariants(rx.edges(c), got, *mins)
        out.append(got)
    return out


# ------------------------------------------------------------------------------------ 1. edge counts ----

EDGE_COUNTS = [0, 1, 2, 3, 63, 64, 65, T - 1, T, T + 1, 2 * T + 1]
MINS = [(3, 0), (0, 3), (4, 6), (7, 2), (0, 0), (1, 1), (1, 0)]


def test_edge_counts_around_the_wave_and_the_tile(ok):
    rng = np.random.default_rng(19)
    n = -(-(11 * (2 * T + 2)) // SPB) * SPB
    rx = ok.Receiver(None, None, max_samples=n, threshold=THR, edge_capacity=n)
    for E in EDGE_COUNTS:
        iq, want_e = random_capture(E, rng)
        rx.rx(iq)
        assert rx.clean_kernel_ms == 0.0
        for mins in MINS:
            got = clean_and_check(rx, mins, want_e, "E=%d" % E)[0]
            assert got.size % 2 == E % 2
            if max(mins) <= 1:          # the list itself, and its counts
                assert got.tolist() == want_e.tolist()
                assert rx.clean_edges(*mins)[0] == dict(edges_in=E, edges_out=E, deleted=[0, 0], min_on=mins[0], min_off=mins[1])
            elif E > 60:
                assert got.size < E
        assert rx.clean_kernel_ms > 0.0
    rx.close()


# -------------------------------------------------------------------------------------------- 2. chains ----

@pytest.mark.parametrize("m", [2, 3, 4, 5])
def test_a_short_chain_across_a_tile_boundary(ok, m):
    """m short runs among long ones, the chain's first run at T - k: the tile behind the boundary learns d of the run
    in front of it from the scan, at either parity and with the chain ending at, across and starting at the boundary"""
    n = -(-(20 * (T + 64)) // SPB) * SPB
    rx = ok.Receiver(None, None, max_samples=n, threshold=THR, edge_capacity=n)
    for k in range(0, m + 2):
        closed = np.full(T + 40, 20, dtype=np.int64)
        closed[T - k:T - k + m] = 2
        iq, want_e = capture_of(closed)
        rx.rx(iq)
        got = clean_and_check(rx, (3, 3), want_e, "m=%d k=%d" % (m, k))[0]
        # an odd chain vanishes, an even one leaves its last edge
        assert want_e.size - got.size == (m + 1 if m % 2 else m), (m, k)
    rx.close()


@pytest.mark.parametrize("extra", [1, 2])
def test_one_chain_over_three_tiles_and_more(ok, extra):
    """every sample alternating: one chain over all runs; E = 3 T + 1 and 3 T + 2"""
    E = 3 * T + extra
    n = -(-(E + 8) // SPB) * SPB
    iq, want_e = capture_of(np.ones(E - 1, dtype=np.int64), lead=2, n=n)
    rx = ok.Receiver(None, None, max_samples=n, threshold=THR, edge_capacity=n)
    rx.rx(iq)
    got = clean_and_check(rx, (2, 2), want_e, "alternating E=%d" % E)[0]
    assert got.tolist() == (want_e[-1:].tolist() if E % 2 else [])
    assert rx.clean_edges(2, 2)[0]["deleted"] == [0, E // 2]
    # the on-runs alone: every on-run goes, whatever lies between two of them is one off-run
    got = clean_and_check(rx, (2, 0), want_e, "alternating, min_on alone")[0]
    assert got.tolist() == (want_e[-1:].tolist() if E % 2 else [])
    got = clean_and_check(rx, (0, 2), want_e, "alternating, min_off alone")[0]
    assert got.tolist() == (want_e[[0]].tolist() if E % 2 else want_e[[0, -1]].tolist())
    rx.close()


@pytest.mark.parametrize("extra", [1, 2])
def test_chains_from_lane_to_lane_of_the_aggregate_scan(ok, extra):
    """more tiles than one lane of the aggregate scan folds: one chain over all of them, and random runs whose chains
    cross the tile boundaries where they fall"""
    rng = np.random.default_rng(50 + extra)
    E = (2 * LANE + 1) * T + extra
    n = -(-(3 * E) // SPB) * SPB
    rx = ok.Receiver(None, None, max_samples=n, threshold=THR, edge_capacity=n)
    iq, want_e = capture_of(np.ones(E - 1, dtype=np.int64), lead=2, n=n)
    rx.rx(iq)
    got = clean_and_check(rx, (2, 2), want_e, "alternating over %d tiles" % (2 * LANE + 2))[0]
    assert got.tolist() == (want_e[-1:].tolist() if E % 2 else [])
    iq, want_e = capture_of(rng.integers(1, 4, size=E - 1), lead=1, n=n)
    rx.rx(iq)
    for mins in ((2, 2), (3, 2), (2, 3)):
        got = clean_and_check(rx, mins, want_e, "runs of 1 .. 3 over %d tiles" % (2 * LANE + 2))[0]
        assert_same_hist(rx.pulse_hist(0, clean=True), hist_of(got, n), "lanes")
    rx.close()


def test_a_list_beyond_one_step_of_the_aggregate_scan(ok):
    """STEP + 2 tiles and more: the aggregate scan carries d and its sums from its first step into its second.  4.2
    million edges, so the restatement is the parity form in numpy alone (tests/clean_contract.py: clean_of_long, which
    tests/test_clean_host.py holds against the sequential form)"""
    import torch
    rng = np.random.default_rng(77)
    E = (STEP + 2) * T + 3
    n = -(-(2 * E + 16) // SPB) * SPB
    iq, want_e = capture_of(rng.integers(1, 3, size=E - 1), lead=3, n=n)         # runs of 1 and 2: chains everywhere
    rx = ok.Receiver(None, None, max_samples=n, threshold=THR, edge_capacity=E + 64)
    dev_t = torch.from_numpy(iq).cuda()
    rx.rx_device(dev_t.data_ptr(), n)
    e = rx.edges()
    assert e.size == E and (e == want_e).all()
    for mins in ((2, 2), (2, 0)):
        want, deleted = clean_of_long(e, *mins)
        info = rx.clean_edges(*mins)
        got = rx.edges(0, clean=True)
        assert info == [dict(edges_in=E, edges_out=int(want.size), deleted=deleted, min_on=mins[0], min_off=mins[1])]
        assert got.size == want.size and (got == want).all(), (mins, np.argwhere(got != want)[:4].tolist())
        assert 0 < want.size < E and (E - want.size) % 2 == 0
    assert_same_hist(rx.pulse_hist(0, clean=True), hist_of(got, n), "beyond one step")
    rx.close()


# ----------------------------------------------------------------------------------- 3. batched run ----

def test_batched_run_keeps_the_captures_apart(ok):
    """[a chain up to the last edge, no edge, a chain from the first edge, T + 1 edges, one edge]: no carry and no
    offset crosses from a capture into the next"""
    import torch
    rng = np.random.default_rng(3)
    n = -(-(20 * (T + 64)) // SPB) * SPB
    up_to_last = np.full(T + 9, 20, dtype=np.int64)
    up_to_last[-5:] = 1                                         # runs E - 6 .. E - 2 are short: d of the last run is 1
    from_first = np.full(300, 20, dtype=np.int64)
    from_first[:4] = 1
    parts = [capture_of(up_to_last, n=n), capture_of(None, n=n), capture_of(from_first, lead=0, n=n),
             random_capture(T + 1, rng, n=n), capture_of(np.zeros(0, dtype=np.int64), lead=77, n=n)]
    caps = len(parts)
    host = np.stack([p[0] for p in parts])
    rx = ok.Receiver(None, None, max_samples=n, max_captures=caps, threshold=THR, edge_capacity=caps * (T + 64))
    dev_t = torch.from_numpy(host).cuda()
    rx.rx_device(dev_t.data_ptr(), n, num_captures=caps)
    for c in range(caps):
        assert rx.edges(c).tolist() == parts[c][1].tolist(), c
    for mins in ((3, 3), (2, 0), (0, 5), (1, 1)):
        got = clean_and_check(rx, mins, None, "batch", captures=caps)
        assert [g.size for g in got][1] == 0 and got[4].tolist() == [77]
        n_out = rx.stats()["decimated_samples"]
        for c in range(caps):
            assert_same_hist(rx.pulse_hist(c, clean=True), hist_of(got[c], n_out), "batch capture %d" % c)
            assert_same_survey(rx.symbol_survey(TABLE, ROLES, c, clean=True), survey_of(got[c], TABLE, ROLES), "batch %d" % c)
    for call in (lambda: rx.edges(caps, clean=True), lambda: rx.pulse_hist(caps, clean=True),
                 lambda: rx.symbol_survey(TABLE, None, caps, clean=True)):
        with pytest.raises(ok.OokdError) as e:
            call()
        assert e.value.code == -1
    rx.close()


# --------------------------------------------------------------------------------------- 4. carriers ----

def test_carrier_lists_are_the_tuned_contexts(ok):
    nu1, nu2 = 600e3 / RATE, -900e3 / RATE
    g1, _ = golden_capture("G1")
    g2, _ = golden_capture("G2")
    ext = np.zeros_like(g1)
    ext[:g2.size] = g2
    # (tests/test_gpu_pulses.py: test_carrier_histograms_are_the_tuned_contexts)
    z = moved(g1, nu1, scale=0.5).astype(np.int32) + moved(ext, nu2, 400.0 * (1 + 0.5j), 40, seed=11, scale=0.5).astype(np.int32)
    iq = np.clip(z, -32768, 32767).astype(np.int16)
    n = iq.size // 2
    f = ok.Filter.load(golden_path("filters", "fs32_fs4"))
    carriers = [(nu1, 0.1), (nu2, 0.12)]
    mins = (1600, 1700)                 # G1's bit pulses (1503) and G2's short gaps (1647) are short
    rx = ok.Receiver(f, None, max_samples=n, carriers=carriers)
    rx.rx(iq)
    got = clean_and_check(rx, mins, None, "carriers", captures=2)
    for k, (nu, thr) in enumerate(carriers):
        one = ok.Receiver(f, None, max_samples=n, threshold=thr, tune=nu)
        one.rx(iq)
        assert one.edges().tolist() == rx.edges(k).tolist()
        alone = clean_and_check(one, mins, None, "tuned %d" % k)[0]
        assert alone.tolist() == got[k].tolist()
        assert one.clean_edges(*mins) == [rx.clean_edges(*mins)[k]]
        assert_same_hist(one.pulse_hist(0, clean=True), rx.pulse_hist(k, clean=True), "carrier %d" % k)
        one.close()
        assert rx.edges(k).size == (228, 136)[k] and got[k].size < rx.edges(k).size
    rx.close()


# ------------------------------------------------------- 5. the clean readers and the untouched originals ----

def test_readers_of_the_cleaned_list_and_the_originals(ok, vectors):
    rng = np.random.default_rng(41)
    iq, want_e = random_capture(3 * T + 17, rng)
    n = iq.size // 2
    rx = ok.Receiver(None, None, max_samples=n, threshold=THR, edge_capacity=n)
    res = rx.rx(iq)
    n_out = res.stats["decimated_samples"]
    before = (rx.edges(0).tolist(), rx.pulse_hist(0), rx.symbol_survey(TABLE, ROLES))
    for mins in ((4, 0), (0, 5), (4, 5)):
        cleaned = clean_and_check(rx, mins, want_e, "readers")[0]
        assert_same_hist(rx.pulse_hist(0, clean=True), hist_of(cleaned, n_out), "clean histogram %s" % (mins,))
        assert_same_survey(rx.symbol_survey(TABLE, ROLES, 0, clean=True), survey_of(cleaned, TABLE, ROLES), "clean survey")
        assert_same_survey(rx.symbol_survey(TABLE, None, 0, clean=True), survey_of(cleaned, TABLE), "clean kinds")
        # the run's own list and what is computed from it are what they were
        assert rx.edges(0).tolist() == before[0]
        assert_same_hist(rx.pulse_hist(0), before[1])
        assert_same_hist(rx.pulse_hist(0), hist_of(want_e, n_out))
        assert_same_survey(rx.symbol_survey(TABLE, ROLES), before[2])
        after = rx.result()
        assert after.stats == res.stats == rx.stats()
    rx.close()
    # with a device behind the front end: the messages and the statistics of the run stay
    g = vectors["G1"]
    giq = golden_iq(vectors, "G1")
    f = ok.Filter.load(golden_path("filters", g["filter"]))
    d = ok.Device.load(golden_path("devices", g["device"]), RATE // f.total_decimation)
    rx = ok.Receiver(f, d, max_samples=giq.size // 2, threshold=THR)
    res = rx.rx(giq)
    assert len(res.msg_samples) > 0
    clean_and_check(rx, (1600, 0), None, "G1")
    after = rx.result()
    assert after.stats == res.stats
    assert (after.msg_samples == res.msg_samples).all() and (after.payloads == res.payloads).all()
    rx.close()


# ------------------------------------------------------------------------------ 6. caching and reuse ----

def test_caching_and_a_new_run(ok):
    rng = np.random.default_rng(8)
    iq, want_e = random_capture(T + 300, rng)
    n = iq.size // 2
    rx = ok.Receiver(None, None, max_samples=n, threshold=THR, edge_capacity=n)
    rx.rx(iq)
    n_out = rx.stats()["decimated_samples"]
    assert rx.clean_kernel_ms == 0.0
    first = clean_and_check(rx, (4, 4), want_e)[0]
    ms = rx.clean_kernel_ms
    assert ms > 0.0
    h = rx.pulse_hist(0, clean=True)
    assert rx.clean_edges(4, 4) == [info_of(want_e, 4, 4)]
    assert rx.clean_kernel_ms == ms                             # the same minimums: nothing was launched
    assert_same_hist(rx.pulse_hist(0, clean=True), h)
    other = clean_and_check(rx, (6, 2), want_e)[0]              # other minimums: computed again
    assert other.tolist() != first.tolist()
    assert_same_hist(rx.pulse_hist(0, clean=True), hist_of(other, n_out), "the clean histogram follows")
    assert rx.edges(0, clean=True).tolist() == other.tolist()
    # a new run: its cleaned list does not exist until somebody asks for it
    iq2, want_e2 = random_capture(500, rng, n=n)
    rx.rx(iq2)
    assert rx.clean_kernel_ms == 0.0
    for call in (lambda: rx.edges(0, clean=True), lambda: rx.pulse_hist(0, clean=True),
                 lambda: rx.symbol_survey(TABLE, None, 0, clean=True), lambda: rx.symbol_survey(TABLE, ROLES, 0, clean=True)):
        with pytest.raises(ok.OokdError) as e:
            call()
        assert e.value.code == -1 and "no cleaned list of the last run" in str(e.value)
    assert_same_hist(rx.pulse_hist(0), hist_of(want_e2, n_out))  # the original answers as ever
    second = clean_and_check(rx, (6, 2), want_e2)[0]            # (the minimums of the run before: still a new pass)
    assert rx.clean_kernel_ms > 0.0
    assert_same_hist(rx.pulse_hist(0, clean=True), hist_of(second, n_out))
    rx.close()


def test_one_context_small_dense_sparse_empty_dense(ok):
    n = 1 << 16
    rng = np.random.default_rng(6)
    dense, _ = capture_of(rng.integers(1, 4, size=n // 4), n=n)
    small, _ = capture_of([300, 5000, 2, 7000, 300], lead=1000, n=n)
    empty = np.zeros(2 * SPB, dtype=np.int16)
    rx = ok.Receiver(None, None, max_samples=n, threshold=THR, edge_capacity=n + 64)
    seen = []
    for label, iq in (("small", small), ("dense", dense), ("sparse", small), ("empty", empty), ("dense", dense)):
        rx.rx(iq)
        assert rx.clean_kernel_ms == 0.0, label                 # nobody has asked about this run yet
        got = clean_and_check(rx, (3, 2), None, label)[0]
        assert rx.clean_kernel_ms > 0.0, label
        n_out = rx.stats()["decimated_samples"]
        assert_same_hist(rx.pulse_hist(0, clean=True), hist_of(got, n_out), label)
        seen.append(got)
    rx.close()
    assert seen[0].size == 4 and seen[0].tolist() == seen[2].tolist() and seen[3].size == 0
    assert 1000 < seen[1].size < n // 4 and seen[4].tolist() == seen[1].tolist()
    # a capture of no samples at all: a valid run, an empty cleaned list, and nothing to launch
    rx = ok.Receiver(None, None, max_samples=n, threshold=THR)
    rx.rx(np.zeros(0, dtype=np.int16))
    assert rx.clean_edges(5, 5) == [dict(edges_in=0, edges_out=0, deleted=[0, 0], min_on=5, min_off=5)]
    assert rx.clean_kernel_ms == 0.0 and rx.edges(0, clean=True).size == 0
    assert_same_hist(rx.pulse_hist(0, clean=True), hist_of([], 0))
    assert rx.symbol_survey(TABLE, None, 0, clean=True)["num_symbols"] == 0
    rx.close()


# -------------------------------------------------------------------------------------- 7. refusals ----

def test_refusals(ok, vectors):
    import torch
    n = 1 << 15
    iq, _ = capture_of(np.full(1999, 3, dtype=np.int64), lead=10)
    readers = (lambda rx: rx.edges(0, clean=True), lambda rx: rx.pulse_hist(0, clean=True),
               lambda rx: rx.symbol_survey(TABLE, None, 0, clean=True))
    # no run yet
    rx = ok.Receiver(None, None, max_samples=n, threshold=THR, edge_capacity=256)
    with pytest.raises(ok.OokdError) as e:
        rx.clean_edges(2, 2)
    assert e.value.code == -1 and "no finished run" in str(e.value)
    # an overflowed edge list
    with pytest.raises(ok.OokdError) as e:
        rx.rx(iq)
    assert e.value.code == -5
    with pytest.raises(ok.OokdError) as e:
        rx.clean_edges(2, 2)
    assert e.value.code == -5 and "overflow" in str(e.value)
    assert rx.clean_kernel_ms == 0.0
    # the next run fits: the clean readers before any clean call, then the answer
    rx.rx(capture_of(np.full(99, 3, dtype=np.int64), lead=10)[0])
    for reader in readers:
        with pytest.raises(ok.OokdError) as e:
            reader(rx)
        assert e.value.code == -1 and "no cleaned list of the last run" in str(e.value)
    assert clean_and_check(rx, (4, 0))[0].size == 0             # 100 edges, every on-run short: 50 on-runs go
    rx.close()
    # a shard run
    rx = ok.Receiver(None, None, max_samples=n, threshold=THR)
    dev_t = torch.from_numpy(iq).cuda()
    rx.shard_begin(dev_t.data_ptr(), iq.size // 2, None, True, None)
    with pytest.raises(ok.OokdError) as e:
        rx.clean_edges(2, 2)
    assert e.value.code == -1 and "shard" in str(e.value)
    rx.rx(iq)                                                   # a whole run on the same context is answered again
    assert clean_and_check(rx, (0, 4))[0].size == 2
    rx.close()
    # a pipelined run (needs a state machine behind the front end)
    g = vectors["G1"]
    giq = golden_iq(vectors, "G1")
    f = ok.Filter.load(golden_path("filters", g["filter"]))
    d = ok.Device.load(golden_path("devices", g["device"]), RATE // f.total_decimation)
    rx = ok.Receiver(f, d, max_samples=giq.size // 2, pipeline_chunk_samples=4 * SPB)
    res = rx.rx(giq)
    assert res.stats["pipeline_chunks"] >= 2
    with pytest.raises(ok.OokdError) as e:
        rx.clean_edges(2, 2)
    assert e.value.code == -1 and "pipelined" in str(e.value)
    rx.close()


# ------------------------------------------------------------- 8. the synthetic capture, made on the GPU ----

@pytest.mark.parametrize("filt", ["fs32_fs4", "fs128_fs16_dec4"])
def test_synthetic_capture_loses_its_glitches(ok, filt):
    """2^24 samples at 3 Msps, seed 5, p3l-nexa2012 with pauses of 4 .. 20 ms: the cleaned list of the capture with a
    glitch in every eighth message is the list of the capture without (tests/test_clean_host.py says why), and
    suggest_device with min_on on the one answers what it answers on the other"""
    import torch
    n = 1 << 24
    f = ok.Filter.load(golden_path("filters", filt))
    rate = RATE // f.total_decimation
    min_on = int(250e-6 * rate)
    d = ok.Device.load(golden_path("devices", "p3l-nexa2012"), RATE)
    cap = torch.empty(2 * n + 64, dtype=torch.int16, device="cuda")
    rx = ok.Receiver(f, None, max_samples=n, threshold=THR)
    seen = {}
    for glitch_every in (0, 8):
        syn = ok.Synth(d, n, seed=5, sample_rate=RATE, gap_us=(4000, 20000), glitch_every=glitch_every)
        syn.fill_device(cap.data_ptr())
        torch.cuda.synchronize()
        syn.close()
        rx.rx_device(cap.data_ptr(), n)
        e = rx.edges()
        if glitch_every == 0:
            seen[0] = (e, rx.suggest_device(rate))
            assert rx.clean_kernel_ms == 0.0                    # min_on = 0: nothing was cleaned
        else:
            seen[8] = (e, rx.suggest_device(rate, min_on=min_on), rx.edges(clean=True), rx.suggest_device(rate))
            assert rx.clean_kernel_ms > 0.0
            check(rx, 0, (min_on, 0))
    d.close()
    n_out = rx.stats()["decimated_samples"]
    rx.close()
    plain, glitched, cleaned = seen[0][0], seen[8][0], seen[8][2]
    assert glitched.size > plain.size and cleaned.tolist() == plain.tolist()
    assert seen[8][1] == seen[0][1] == py_chain(plain, n_out, rate)[0]
    s = seen[8][1]
    assert (s["found"], s["num_bits"], s["frames_seen"], s["frames_counted"], s["frames_clean"]) == (1, 36, 48, 37, 26)
    assert seen[8][3]["frames_clean"] == 22                     # without cleaning: four frames hold a glitch symbol
