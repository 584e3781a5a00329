"""The symbol survey on the GPU (ookd_rx_symbol_survey; the three kernels of symbols.hip).  The survey is an exact
integer function of a capture's edge list, a class table and the roles, so every comparison is equality of all
members against the numpy restatement of the contract (tests/symbol_contract.py) fed with `rx.edges(c)`.  The inputs
are hand-laid bit streams through a context without a filter, laid the way tests/test_gpu_pulses.py lays its runs."""
import numpy as np
import pytest

from tests.helpers import golden_path
from tests.pulse_contract import RATE, SPB, THR, assert_same_hist, golden_iq, hist_of
from tests.symbol_contract import (NO_FRAMES, OTHER, ONE, SIDE, SYNC, ZERO, assert_same_survey, frames_dict, py_chain,
                                   survey_of)
from tests.tuned_contract import golden_capture, moved

pytestmark = pytest.mark.gpu

ON = 2047                       # I of an "on" sample (no filter: |x| = 2047 / 2048 against the threshold 0.1)
TILE = 1024                     # symbols a workgroup takes per step (kSymTile)
SCAN = 256                      # tile aggregates the scan kernel takes per step (kSymScanThreads)

# run lengths in samples and their classes: on 2 -> 0, 4..5 -> 1, else none; off 1 -> 0, 3 -> 1, 6..7 -> 2, 8 -> 3
TABLE = dict(lower=[[1, 3, 6, 8], [2, 4]], upper=[[1, 3, 7, 8], [2, 5]])
Z, O, Y = (2, 1), (2, 3), (2, 6)            # zero, one, sync
X, P, N, M = (5, 1), (2, 8), (9, 11), (2, 11)   # OTHERs: another pulse, a pause, no class on both levels / on one
ROLES = np.zeros((SIDE, SIDE), dtype=np.uint8)
ROLES[0, 0], ROLES[0, 1], ROLES[0, 2] = ZERO, ONE, SYNC
DURATIONS = ("sync_on_us", "sync_off_us", "bit_on_us", "zero_off_us", "one_off_us")


@pytest.fixture(scope="module")
def ok():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from ookiedokie_amd import build as okbuild
    okbuild.build()
    import ookiedokie_amd as okm
    okm.lib()
    return okm


def lay(pairs, lead=3, ending="low", n=None):
    """I,Q of a capture without a filter that holds the (on, off) symbols `pairs` after `lead` off samples, every one
    of them closed: behind the last off-run comes one more pulse -- of 2 samples and then off to the end ("low": E =
    2 S + 2), or up to the end of the last whole buffer ("high": E = 2 S + 1, no falling edge in the padding).
    n: samples of the capture (a whole number of buffers), default the fewest."""
    runs = np.array([d for p in pairs for d in p], dtype=np.int64)
    used = lead + int(runs.sum())
    if n is None:
        n = -(-(used + 4) // SPB) * SPB
    assert n % SPB == 0 and used + 4 <= n
    lv = np.zeros(runs.size + 1, dtype=np.int16)
    lv[0::2] = ON
    i = np.zeros(n, dtype=np.int16)
    i[lead:used + (2 if ending == "low" else n - used)] = np.repeat(lv, np.append(runs, 2 if ending == "low" else n - used))
    iq = np.zeros(2 * n, dtype=np.int16)
    iq[0::2] = i
    return iq


def check(rx, capture=0, table=TABLE, roles=ROLES, symbols=None, what=""):
    """capture's survey with and without roles against the restatement over its own edge list"""
    e = rx.edges(capture)
    got = rx.symbol_survey(table, roles, capture)
    assert_same_survey(got, survey_of(e, table, roles), what)
    kinds = rx.symbol_survey(table, None, capture)
    assert_same_survey(kinds, survey_of(e, table), what + " (roles=None)")
    assert (kinds["kinds"] == got["kinds"]).all() and kinds["num_symbols"] == got["num_symbols"]
    assert not kinds["frames"].any() and (kinds["num_syncs"], kinds["head_symbols"], kinds["tail_symbols"]) == (0, 0, 0)
    if symbols is not None:
        assert got["num_symbols"] == symbols, (what, e.size)
    return got


def data(rng, n):
    return [Z if b else O for b in rng.integers(0, 2, size=n).tolist()]


# ------------------------------------------------------------------------------------ 1. edge counts ----

def test_edge_counts_zero_to_five(ok):
    rx = ok.Receiver(None, None, max_samples=SPB, threshold=THR)
    for E, (pairs, ending) in enumerate([(None, None), ([], "high"), ([], "low"), ([Y], "high"), ([Y], "low"), ([Y, Y], "high")]):
        iq = np.zeros(2 * SPB, dtype=np.int16) if pairs is None else lay(pairs, ending=ending)
        rx.rx(iq)
        assert rx.edges().size == E
        got = check(rx, symbols=(E - 1) // 2 if E >= 3 else 0, what="E=%d" % E)
        assert got["num_syncs"] == got["num_symbols"] and got["head_symbols"] == 0
        assert got["tail_symbols"] == (1 if E >= 3 else 0)
        assert frames_dict(got, 1) == ({1: 1} if E == 5 else {})
    rx.close()


# ------------------------------------------------------------------------------------- 2. the frames ----

@pytest.mark.parametrize("ending", ["low", "high"])
def test_hand_laid_frames(ok, ending):
    """a sync at symbol 0 and at S - 1; D = 1, 2, 3; an OTHER at p - 1 (clean) and at p - 2 (not); class 16 on either
    level; D = 510, 511, 512 and 5000 -- the last one crosses four whole tiles without a sync"""
    rng = np.random.default_rng(3)
    pairs = [Y, Y, Z, Y, Z, O, Y]                               # D = 1, 2, 3
    pairs += [Z, Z, X, Y, Z, X, Z, Y]                           # D = 4 clean (X at p - 1), D = 4 not clean (X at p - 2)
    pairs += [O, N, Y, O, M, O, Y, P, Y, P, Z, Y]               # none-classes: D = 3 clean, D = 4 not, D = 2 clean, D = 3 not
    for d in (510, 511, 512, 5000):
        pairs += data(rng, d - 1) + [Y]
    iq = lay(pairs, lead=0 if ending == "high" else 5, ending=ending)
    rx = ok.Receiver(None, None, max_samples=iq.size // 2, threshold=THR, edge_capacity=iq.size // 2)
    rx.rx(iq)
    got = check(rx, symbols=len(pairs), what=ending)
    rx.close()
    assert got["head_symbols"] == 0 and got["tail_symbols"] == 1 and got["num_syncs"] == 14
    assert frames_dict(got, 1) == {1: 1, 2: 2, 3: 2, 4: 1, 510: 1, 511: 3}
    assert frames_dict(got, 0) == {3: 1, 4: 2}
    assert got["kinds"][16, 16] == 1 and got["kinds"][0, 16] == 1 and got["kinds"][1, 0] == 2 and got["kinds"][0, 3] == 2


def test_no_sync_at_all(ok):
    rng = np.random.default_rng(4)
    pairs = data(rng, 3 * TILE + 17) + [X, P]
    rx = ok.Receiver(None, None, max_samples=4 * SPB, threshold=THR, edge_capacity=4 * SPB)
    rx.rx(lay(pairs))
    got = check(rx, symbols=len(pairs))
    assert (got["num_syncs"], got["head_symbols"], got["tail_symbols"]) == (0, len(pairs), 0) and not got["frames"].any()
    # the same symbols, every kind a sync: frames of one symbol throughout, and every one clean
    got = check(rx, roles=np.full((SIDE, SIDE), SYNC, dtype=np.uint8), symbols=len(pairs))
    assert got["num_syncs"] == len(pairs) and frames_dict(got, 1) == {1: len(pairs) - 1}
    rx.close()


# --------------------------------------------------------------------- 3. waves, tiles and scan steps ----

@pytest.mark.parametrize("S", [63, 64, 65, 255, 256, 257, TILE - 1, TILE, TILE + 1, 2 * TILE, 2 * TILE + 1])
def test_symbol_counts_around_the_wave_and_the_tile(ok, S):
    """syncs on both sides of every boundary: the frames cross lanes, waves and tiles"""
    rng = np.random.default_rng(S)
    pairs = data(rng, S)
    for j in {0, 62, 63, 64, 255, 256, TILE - 2, TILE - 1, TILE, TILE + 1, 2 * TILE - 1, 2 * TILE, S - 1}:
        if j < S:
            pairs[j] = Y
    for j in (61, 254, TILE - 3, 2 * TILE - 2):                 # an OTHER just before a sync, and one inside a frame
        if j < S - 1:
            pairs[j] = X
    if S > 300:
        pairs[130] = X
    rx = ok.Receiver(None, None, max_samples=2 * SPB, threshold=THR, edge_capacity=2 * SPB)
    rx.rx(lay(pairs, ending="high" if S % 2 else "low"))
    got = check(rx, symbols=S, what="S=%d" % S)
    rx.close()
    assert got["head_symbols"] == 0 and got["tail_symbols"] == 1
    if S > 300:
        assert frames_dict(got, 0) == {255 - 64: 1}


@pytest.mark.parametrize("S", [SCAN * TILE - 1, SCAN * TILE, SCAN * TILE + 1, (SCAN + 1) * TILE + 5])
def test_symbol_counts_around_a_second_scan_step(ok, S):
    """256 tile aggregates are one step of the scan kernel.  One frame runs from symbol 5 to beyond the last tile of the
    first step, with OTHERs along the way: the position and the count pass through the tile aggregates and from the
    scan's first step into its second; further frames follow in the tiles behind."""
    rng = np.random.default_rng(S & 0xffff)
    pairs = data(rng, S)
    pairs[5] = Y
    others = sorted(rng.choice(np.arange(6, S - 3000), size=37, replace=False).tolist())
    for j in others:
        pairs[j] = X
    syncs = [5, S - 2900, S - 2900 + 38, S - 1100, S - 1100 + TILE, S - 1]
    for j in syncs[1:]:
        pairs[j] = Y
    pairs[S - 1050] = P                                         # inside the frame that crosses the last tile boundary
    iq = lay(pairs)
    n = iq.size // 2
    rx = ok.Receiver(None, None, max_samples=n, threshold=THR, edge_capacity=2 * S + 64)
    rx.rx(iq)
    got = check(rx, symbols=S, what="S=%d" % S)
    rx.close()
    assert (got["num_syncs"], got["head_symbols"], got["tail_symbols"]) == (6, 5, 1)
    assert frames_dict(got, 0) == {511: 2} and frames_dict(got, 1) == {38: 1, 75: 1, 511: 1}
    assert got["kinds"][1, 0] == 37 and got["kinds"][0, 3] == 1


# ----------------------------------------------------------------------------------- 4. batched run ----

def test_batch_of_three_captures(ok):
    """the middle capture empty; the first has an odd number of edges, so the third starts at an odd index of the
    run's edge array"""
    import torch
    rng = np.random.default_rng(8)
    n = 2 * SPB
    first = [Y] + data(rng, 40) + [X, Y] + data(rng, 1100) + [Y, P]
    third = data(rng, 7) + [Y] + data(rng, 36) + [P, Y] + data(rng, TILE + 3) + [N, O, Y, Z]
    host = np.zeros((3, 2 * n), dtype=np.int16)
    host[0] = lay(first, lead=0, ending="high", n=n)
    host[2] = lay(third, lead=9, ending="low", n=n)
    rx = ok.Receiver(None, None, max_samples=n, max_captures=3, threshold=THR, edge_capacity=3 * n)
    dev_t = torch.from_numpy(host).cuda()
    rx.rx_device(dev_t.data_ptr(), n, num_captures=3)
    assert [rx.edges(c).size for c in range(3)] == [2 * len(first) + 1, 0, 2 * len(third) + 2]
    a = check(rx, 0, symbols=len(first), what="first")
    b = check(rx, 1, symbols=0, what="middle")
    c = check(rx, 2, symbols=len(third), what="third")
    assert frames_dict(a, 1) == {42: 1, 511: 1} and not a["frames"][0].any()
    assert not b["kinds"].any() and (b["num_syncs"], b["head_symbols"], b["tail_symbols"]) == (0, 0, 0)
    assert (c["num_syncs"], c["head_symbols"], c["tail_symbols"]) == (3, 7, 2)
    assert frames_dict(c, 1) == {38: 1} and frames_dict(c, 0) == {511: 1}
    with pytest.raises(ok.OokdError) as e:
        rx.symbol_survey(TABLE, ROLES, 3)
    assert e.value.code == -1
    rx.close()


# ------------------------------------------------------------------------ 5. classes, sixteen a level ----

def test_sixteen_classes_per_level_and_random_roles(ok):
    """run lengths 1 .. 18 against sixteen one-length classes per level (17 and 18 have class 16 on either level), and
    a role drawn for every kind: all 289 kinds occur, a quarter of them syncs"""
    rng = np.random.default_rng(16)
    table = dict(lower=[list(range(1, 17)), list(range(1, 17))], upper=[list(range(1, 17)), list(range(1, 17))])
    pairs = [(int(a), int(b)) for a, b in rng.integers(1, 19, size=(6000, 2))]
    roles = rng.integers(0, 4, size=(SIDE, SIDE)).astype(np.uint8)
    iq = lay(pairs)
    rx = ok.Receiver(None, None, max_samples=iq.size // 2, threshold=THR, edge_capacity=iq.size // 2)
    rx.rx(iq)
    got = check(rx, table=table, roles=roles, symbols=len(pairs))
    assert np.count_nonzero(got["kinds"]) == SIDE * SIDE and got["kinds"][16].sum() > 0 and got["kinds"][:, 16].sum() > 0
    assert got["num_syncs"] > 500 and got["frames"][0].any() and got["frames"][1].any()
    # ranges wider than one length, a gap between them, and unequal counts on the two levels
    table = dict(lower=[[2, 9, 15], [1, 4, 5, 12]], upper=[[3, 13, (1 << 64) - 1], [3, 4, 11, 12]])
    check(rx, table=table, roles=roles, symbols=len(pairs))
    check(rx, table=dict(lower=[[], []], upper=[[], []]), roles=roles, symbols=len(pairs))
    rx.close()


# --------------------------------------------------------------------------------------- 6. carriers ----

def test_carrier_surveys_are_the_tuned_contexts(ok):
    nu1, nu2 = 600e3 / RATE, -900e3 / RATE
    g1, _ = golden_capture("G1")
    g2, _ = golden_capture("G2")
    ext = np.zeros_like(g1)
    ext[:g2.size] = g2
    # both transmitters at half level (tests/test_gpu_pulses.py: carriers)
    z = moved(g1, nu1, scale=0.5).astype(np.int32) + moved(ext, nu2, 400.0 * (1 + 0.5j), 40, seed=11, scale=0.5).astype(np.int32)
    iq = np.clip(z, -32768, 32767).astype(np.int16)
    n = iq.size // 2
    f = ok.Filter.load(golden_path("filters", "fs32_fs4"))
    carriers = [(nu1, 0.1), (nu2, 0.12)]
    rx = ok.Receiver(f, None, max_samples=n, carriers=carriers)
    rx.rx(iq)
    for k, (nu, thr) in enumerate(carriers):
        pulses = ok.suggest_pulses(rx.pulse_hist(k), RATE)
        table = ok.symbol_table_from_pulses(pulses)
        coding = ok.suggest_coding(pulses, rx.symbol_survey(table, None, k))
        assert coding["found"] == 1
        got = check(rx, k, table=table, roles=coding["roles"], what="carrier %d" % k)
        one = ok.Receiver(f, None, max_samples=n, threshold=thr, tune=nu)
        one.rx(iq)
        assert one.edges().tolist() == rx.edges(k).tolist()
        assert_same_survey(check(one, 0, table=table, roles=coding["roles"]), got, "carrier %d against its tuned context" % k)
        s = one.suggest_device(RATE)
        assert s == rx.suggest_device(RATE, k) and (s["found"], s["num_bits"]) == (1, (36, 32)[k])
        one.close()
        assert frames_dict(got, 1) == ({38: 2}, {34: 1})[k]
    rx.close()


# ------------------------------------------------------------------------------------------ 7. reuse ----

def test_one_context_dense_sparse_empty(ok):
    rng = np.random.default_rng(6)
    dense = lay([Y if k % 40 == 0 else p for k, p in enumerate(data(rng, 6 * TILE))])
    sparse = lay([Y, Z, O, Y, X], lead=1000)
    empty = np.zeros(2 * 5000, dtype=np.int16)
    n = dense.size // 2
    rx = ok.Receiver(None, None, max_samples=n, threshold=THR, edge_capacity=n)
    assert rx.symbol_kernel_ms == 0.0
    seen = []
    for label, iq in (("dense", dense), ("sparse", sparse), ("empty", empty), ("dense", dense)):
        rx.rx(iq)
        assert rx.symbol_kernel_ms == 0.0, label               # nobody has asked about this run yet
        got = rx.symbol_survey(TABLE, ROLES)
        assert rx.symbol_kernel_ms > 0.0, label
        assert_same_survey(got, survey_of(rx.edges(), TABLE, ROLES), label)
        seen.append(check(rx, what=label))
    assert seen[0]["num_symbols"] == 6 * TILE and frames_dict(seen[0], 1) == {40: 6 * TILE // 40}
    assert seen[1]["num_symbols"] == 5 and frames_dict(seen[1], 1) == {3: 1} and seen[1]["tail_symbols"] == 2
    assert seen[2]["num_symbols"] == 0 and not seen[2]["kinds"].any() and not seen[2]["frames"].any()
    assert_same_survey(seen[3], seen[0])
    # a refused call leaves no time behind
    with pytest.raises(ok.OokdError):
        rx.symbol_survey(dict(lower=[[5, 4], []], upper=[[6, 6], []]))
    assert rx.symbol_kernel_ms == 0.0
    rx.close()
    # a capture of no samples at all: a valid run with an empty survey, and nothing to launch
    rx = ok.Receiver(None, None, max_samples=n, threshold=THR)
    rx.rx(np.zeros(0, dtype=np.int16))
    got = rx.symbol_survey(TABLE, ROLES)
    assert_same_survey(got, survey_of([], TABLE, ROLES))
    assert rx.symbol_kernel_ms == 0.0
    rx.close()


def test_both_passes_on_one_context(ok):
    """the pulse and the symbol pass share a base on the host: a 1-capture run, then a 3-capture run (the pulse result
    buffer grows) on one context, each asked pulse_hist, symbol_survey, pulse_hist -- a symbol pass must not disturb
    the pulse cache or its time, nor a refused one; the context is closed with both passes alive"""
    import torch
    rng = np.random.default_rng(12)
    n = 2 * SPB
    host = np.zeros((3, 2 * n), dtype=np.int16)
    host[0] = lay([Y] + data(rng, 30) + [X, Y] + data(rng, TILE + 40) + [Y, P], lead=0, ending="high", n=n)
    host[1, :2 * SPB] = lay(data(rng, 5) + [Y, Z, O, Y, N], lead=700)
    host[2] = lay([Y if k % 36 == 0 else p for k, p in enumerate(data(rng, 600))], lead=9, n=n)
    dev_t = torch.from_numpy(host).cuda()
    rx = ok.Receiver(None, None, max_samples=n, max_captures=3, threshold=THR, edge_capacity=3 * n)
    for caps, samples in ((1, SPB), (3, n)):
        rx.rx_device(dev_t[1].data_ptr() if caps == 1 else dev_t.data_ptr(), samples, num_captures=caps)
        assert rx.pulse_kernel_ms == 0.0 and rx.symbol_kernel_ms == 0.0, caps   # nobody has asked about this run yet
        n_out = rx.stats()["decimated_samples"]
        edges = [rx.edges(c) for c in range(caps)]
        assert all(e.size >= 3 for e in edges)
        first = [rx.pulse_hist(c) for c in range(caps)]
        ms = rx.pulse_kernel_ms
        assert ms > 0.0 and rx.symbol_kernel_ms == 0.0, caps
        for c in range(caps):
            assert_same_hist(first[c], hist_of(edges[c], n_out), "run of %d, capture %d" % (caps, c))
            got = rx.symbol_survey(TABLE, ROLES, c)
            assert rx.symbol_kernel_ms > 0.0, (caps, c)
            assert_same_survey(got, survey_of(edges[c], TABLE, ROLES), "run of %d, capture %d" % (caps, c))
        for c in range(caps):
            assert_same_hist(rx.pulse_hist(c), first[c], "run of %d, capture %d again" % (caps, c))
        assert rx.pulse_kernel_ms == ms, caps                   # answered from host memory: nothing was launched
    with pytest.raises(ok.OokdError) as e:
        rx.symbol_survey(TABLE, ROLES, 3)
    assert e.value.code == -1 and "capture 3 of 3" in str(e.value)
    assert rx.symbol_kernel_ms == 0.0 and rx.pulse_kernel_ms == ms
    assert_same_survey(rx.symbol_survey(TABLE, None, 2), survey_of(edges[2], TABLE), "the last pass")
    assert rx.symbol_kernel_ms > 0.0
    rx.close()


# -------------------------------------------------------------------------------------- 8. refusals ----

def test_refusals(ok, vectors):
    import torch
    n = 1 << 15
    iq = lay([Z] * 2000)
    rx = ok.Receiver(None, None, max_samples=n, threshold=THR, edge_capacity=256)
    with pytest.raises(ok.OokdError) as e:
        rx.symbol_survey(TABLE, ROLES)
    assert e.value.code == -1 and "no finished run" in str(e.value)
    with pytest.raises(ok.OokdError) as e:
        rx.rx(iq)
    assert e.value.code == -5
    with pytest.raises(ok.OokdError) as e:
        rx.symbol_survey(TABLE, ROLES)
    assert e.value.code == -5 and "overflow" in str(e.value)
    assert rx.symbol_kernel_ms == 0.0
    rx.rx(lay([Z] * 100))                                       # the next run fits, and is answered
    assert check(rx, symbols=100)["kinds"][0, 0] == 100
    for bad in (dict(lower=[[1, 3], [2]], upper=[[3, 4], [2]]), dict(lower=[list(range(17)), []], upper=[list(range(17)), []])):
        with pytest.raises(ok.OokdError) as e:
            rx.symbol_survey(bad, ROLES)
        assert e.value.code == -1 and "class table" in str(e.value)
    with pytest.raises(ok.OokdError) as e:
        rx.symbol_survey(TABLE, np.full((SIDE, SIDE), 4, dtype=np.uint8))
    assert e.value.code == -1 and "role" in str(e.value)
    with pytest.raises(ok.OokdError) as e:
        rx.symbol_survey(TABLE, ROLES, 1)
    assert e.value.code == -1
    rx.close()
    # a shard run
    rx = ok.Receiver(None, None, max_samples=n, threshold=THR)
    dev_t = torch.from_numpy(iq).cuda()
    rx.shard_begin(dev_t.data_ptr(), iq.size // 2, None, True, None)
    with pytest.raises(ok.OokdError) as e:
        rx.symbol_survey(TABLE, ROLES)
    assert e.value.code == -1 and "shard" in str(e.value)
    rx.rx(iq)                                                   # a whole run on the same context is answered again
    assert check(rx, symbols=2000)["num_syncs"] == 0
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
        rx.symbol_survey(TABLE, ROLES)
    assert e.value.code == -1 and "pipelined" in str(e.value)
    with pytest.raises(ok.OokdError):
        rx.suggest_device(RATE // f.total_decimation)
    rx.close()


# ------------------------------------------------------------------------------------ 9. end to end ----

GOLDEN = {"G1": (36, {38: 2}, (501, 8699, 501, 1999, 3999)), "G2": (32, {34: 1}, (8901, 4399, 551, 549, 1699))}


def same_messages(ok, filt, iq_or_ptr, n, suggestion, device_name, rate):
    """a Receiver with Device.from_suggestion against a Receiver with the device file: count, sample indices, payloads"""
    out = []
    for dev in (ok.Device.from_suggestion(suggestion, rate), ok.Device.load(golden_path("devices", device_name), rate)):
        rx = ok.Receiver(filt, dev, max_samples=n, threshold=THR)
        out.append(rx.rx(iq_or_ptr) if isinstance(iq_or_ptr, np.ndarray) else rx.rx_device(iq_or_ptr, n))
        rx.close()
        dev.close()
    mine, want = out
    assert mine.msg_samples.tolist() == want.msg_samples.tolist()
    assert mine.payloads.shape == want.payloads.shape and (mine.payloads == want.payloads).all()
    return len(want.msg_samples)


@pytest.mark.parametrize("filt", ["fs32_fs4", "fs128_fs16_dec4"])
@pytest.mark.parametrize("name", ["G1", "G2"])
def test_suggest_device_on_the_golden_captures(ok, vectors, name, filt):
    iq = golden_iq(vectors, name, noise_seed=7)
    n = iq.size // 2
    f = ok.Filter.load(golden_path("filters", filt))
    rate = RATE // f.total_decimation
    rx = ok.Receiver(f, None, max_samples=n, threshold=THR)
    rx.rx(iq)
    s = rx.suggest_device(rate)
    want, coding, survey, _ = py_chain(rx.edges(), rx.stats()["decimated_samples"], rate)
    assert s == want
    rx.close()
    bits, frames, us = GOLDEN[name]
    assert (s["found"], s["num_bits"], s["num_syncs"]) == (1, bits, sum(frames.values()) + 1)
    assert frames_dict(survey, 1) == frames and s["frames_seen"] == s["frames_clean"] == sum(frames.values())
    if filt == "fs32_fs4":
        assert tuple(s[k] for k in DURATIONS) == us
    assert same_messages(ok, f, iq, n, s, vectors[name]["device"], rate) == sum(frames.values()) + 1


@pytest.mark.parametrize("filt", ["fs32_fs4", "fs128_fs16_dec4"])
@pytest.mark.parametrize("device", ["p3l-nexa2012", "unknown-remote1"])
def test_suggest_device_on_synthetic_captures(ok, device, filt):
    """2^24 samples at 3 Msps, seed 5, pauses of 30 .. 60 ms, no glitches, made on the GPU"""
    import torch
    n = 1 << 24
    f = ok.Filter.load(golden_path("filters", filt))
    rate = RATE // f.total_decimation
    d = ok.Device.load(golden_path("devices", device), RATE)
    syn = ok.Synth(d, n, seed=5, sample_rate=RATE, gap_us=(30000, 60000), glitch_every=0)
    cap = torch.empty(2 * n + 64, dtype=torch.int16, device="cuda")
    syn.fill_device(cap.data_ptr())
    torch.cuda.synchronize()
    sent = syn.num_messages
    syn.close()
    d.close()
    rx = ok.Receiver(f, None, max_samples=n, threshold=THR)
    rx.rx_device(cap.data_ptr(), n)
    s = rx.suggest_device(rate)
    assert s == py_chain(rx.edges(), rx.stats()["decimated_samples"], rate)[0]
    rx.close()
    assert (s["found"], s["num_bits"]) == (1, {"p3l-nexa2012": 36, "unknown-remote1": 32}[device])
    assert s["frames_seen"] == s["frames_clean"] == s["num_syncs"] - 1
    got = same_messages(ok, f, cap.data_ptr(), n, s, device, rate)
    assert 28 <= got <= 70 and got <= sent


def test_suggest_device_says_why_not(ok):
    """two kinds of symbols only: found = 0 with the reason, and no second pass"""
    rx = ok.Receiver(None, None, max_samples=SPB, threshold=THR)
    rx.rx(lay([Z, O] * 50))
    s = rx.suggest_device(RATE)
    assert (s["found"], s["reason"]) == (0, ok.CODING_KINDS)
    with pytest.raises(ok.OokdError):
        ok.Device.from_suggestion(s, RATE)
    # syncs, but no two frames alike
    rng = np.random.default_rng(2)
    pairs = []
    for k in range(5, 25):
        pairs += [Y] + data(rng, k)
    rx.rx(lay(pairs))
    s = rx.suggest_device(RATE)
    assert (s["found"], s["reason"], s["frames_seen"], s["frames_counted"], s["frames_clean"]) == (0, NO_FRAMES, 19, 19, 1)
    rx.close()
