"""The pulse survey on the GPU (ookd_rx_pulse_hist; pulse_hist_kernel in pulses.hip).  The histogram is an exact
integer function of a run's edge list, so every comparison is equality of all members against the numpy restatement
of the contract (tests/pulse_contract.py) fed with `rx.edges(c)` -- and with the oracle's edges where an oracle run
exists."""
import numpy as np
import pytest

from tests.helpers import golden_path
from tests.pulse_contract import RATE, SPB, THR, assert_same_hist, golden_iq, hist_of, oracle_edges, py_bin
from tests.tuned_contract import golden_capture, moved

pytestmark = pytest.mark.gpu

ON = 2047                       # I of an "on" sample (no filter: |x| = 2047 / 2048 against the threshold 0.1)
STEP = 512                      # edges a workgroup takes per step (kPulseEdgesPerStep)
GROUP = 16 * STEP               # edges a workgroup is sized for: the grid grows beyond


@pytest.fixture(scope="module")
def ok():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from ookiedokie_amd import build as okbuild
    okbuild.build()
    import ookiedokie_amd as okm
    okm.lib()
    return okm


def laid(lead, runs, tail=0):
    """a capture without a filter: `lead` off samples, then runs of the given lengths, on first, then `tail` more
    samples of the level the last run left (none: the capture ends with the last run)"""
    lv = np.zeros(len(runs), dtype=np.int16)
    lv[0::2] = ON
    i = np.concatenate([np.zeros(lead, np.int16), np.repeat(lv, runs)])
    iq = np.zeros(2 * (i.size + tail), dtype=np.int16)
    iq[0:2 * i.size:2] = i
    return iq


def laid_edges(lead, runs, n, spb=SPB):
    """the edge list `laid` has by construction: every run starts with an edge; an even number of runs ends with an
    off run, which what follows continues; an odd number ends high, and falls at the first padded sample when the
    capture is no whole number of buffers"""
    e = (lead + np.concatenate([[0], np.cumsum(runs)])[:-1]).astype(np.uint64)
    if len(runs) % 2 and n % spb:
        e = np.concatenate([e, [n]]).astype(np.uint64)
    return e


def with_edges(E, n, rng):
    """I,Q of n samples, n a whole number of buffers, with exactly E edges; and the edges.  E - 1 closed runs of 1 ..
    29 samples; an odd E ends high (a last on-run up to the capture's end), an even one low"""
    iq = np.zeros(2 * n, dtype=np.int16)
    if E == 0:
        return iq, np.zeros(0, dtype=np.uint64)
    assert n % SPB == 0
    lead = int(rng.integers(0, 9))
    runs = rng.integers(1, 30, size=E - 1).tolist()
    if E % 2:
        runs = runs + [n - lead - sum(runs)]
    one = laid(lead, runs)
    iq[:one.size] = one
    e = laid_edges(lead, runs + ([] if E % 2 else [1]), n)
    assert e.size == E
    return iq, e


def check(rx, capture, want_edges=None, what=""):
    """capture's histogram against the restatement over its own edge list (and over want_edges)"""
    n_out = rx.stats()["decimated_samples"]
    e = rx.edges(capture)
    if want_edges is not None:
        assert e.tolist() == np.asarray(want_edges).tolist(), what
    got = rx.pulse_hist(capture)
    assert_same_hist(got, hist_of(e, n_out), what)
    return got


# ------------------------------------------------------------------------------ 1. golden captures ----

@pytest.mark.parametrize("filt", ["fs32_fs4", "fs128_fs16_dec4", None])
@pytest.mark.parametrize("name", ["G1", "G2"])
def test_golden_captures(ok, oracle, vectors, name, filt):
    iq = golden_iq(vectors, name, noise_seed=5)
    n = iq.size // 2
    want_e, want_n = oracle_edges(oracle, iq, filt)
    f = ok.Filter.load(golden_path("filters", filt)) if filt else None
    dec = f.total_decimation if f else 1
    d = ok.Device.load(golden_path("devices", vectors[name]["device"]), RATE // dec)
    hists = []
    for dev in (None, d):
        rx = ok.Receiver(f, dev, max_samples=n, threshold=THR)
        assert rx.pulse_kernel_ms == 0.0
        res = rx.rx(iq)
        assert res.stats["decimated_samples"] == want_n
        h = check(rx, 0, want_e, "%s %s device=%s" % (name, filt, dev is not None))
        assert_same_hist(h, hist_of(want_e, want_n))
        assert rx.pulse_kernel_ms > 0.0
        # the run's own results are what they were without the call
        after = rx.result()
        assert after.stats == res.stats
        assert (after.msg_samples == res.msg_samples).all() and (after.payloads == res.payloads).all()
        if dev is not None and filt == vectors[name]["filter"]:
            assert len(res.msg_samples) > 0
        hists.append(h)
        rx.close()
    assert_same_hist(hists[0], hists[1])
    s = ok.suggest_pulses(hists[0], RATE / dec)
    assert s["found"] == 1


# ------------------------------------------------------------------------------- 2. hand-laid runs ----

LENGTHS = [1, 2, 31, 32, 33] + [(1 << k) + j for k in range(6, 21) for j in (-1, 0, 1)]


@pytest.mark.parametrize("case", ["edge-at-0-ends-high", "edge-later-ends-low", "ends-high-on-a-whole-buffer"])
def test_hand_laid_runs(ok, case):
    if case == "edge-at-0-ends-high":
        lead, runs, tail = 0, LENGTHS + [77], 0                 # 51 runs: the last one is on
    elif case == "edge-later-ends-low":
        lead, runs, tail = 5, [7] + LENGTHS + [100], 1234       # every length on the other level; ends low
    else:
        runs = LENGTHS[:20]
        lead, tail = 3, 0
        runs = runs + [SPB - (lead + sum(runs)) % SPB]          # 21 runs, the last one on, up to the buffer's end
    iq = laid(lead, runs, tail)
    n = iq.size // 2
    assert (n % SPB == 0) == (case == "ends-high-on-a-whole-buffer")
    n_out = -(-n // SPB) * SPB
    want_e = laid_edges(lead, runs, n)
    rx = ok.Receiver(None, None, max_samples=n, threshold=THR)
    rx.rx(iq)
    h = check(rx, 0, want_e, case)
    rx.close()
    assert h["samples"] == n_out and h["open_head"] == lead
    closed = runs[:len(want_e) - 1]
    for i, d in enumerate(closed):
        assert h["count"][1 - (i & 1), py_bin(d)] >= 1, (i, d)
    assert int(h["runs"].sum()) == len(closed) and int(h["sum"].sum()) == sum(closed)
    if case == "edge-at-0-ends-high":
        assert h["tail_level"] == 0 and h["open_tail"] == n_out - n     # fell at the first padded sample
    elif case == "edge-later-ends-low":
        assert h["tail_level"] == 0 and h["open_tail"] == n_out - n + tail + runs[-1]     # the last off-run is open
    else:
        assert h["tail_level"] == 1 and h["open_tail"] == runs[-1]


# ------------------------------------------------------------------------------------ 3. edge counts ----

EDGE_COUNTS = [0, 1, 2, 3, 63, 64, 65, 127, 128, 129, STEP - 1, STEP, STEP + 1, 2 * STEP + 1,
               GROUP - 1, GROUP, GROUP + 1, 2 * GROUP + 1]


def test_edge_counts_around_the_wave_and_the_grid(ok):
    rng = np.random.default_rng(99)
    n = -(-30 * (2 * GROUP + 2) // SPB) * SPB
    rx = ok.Receiver(None, None, max_samples=n, threshold=THR, edge_capacity=n)
    for E in EDGE_COUNTS:
        m = n if E > STEP + 1 else 4 * SPB                      # (short lists in short captures)
        iq, want_e = with_edges(E, m, rng)
        rx.rx(iq)
        h = check(rx, 0, want_e, "E=%d" % E)
        assert h["num_edges"] == E and int(h["runs"].sum()) == max(E - 1, 0) and h["tail_level"] == E % 2
    rx.close()


# ----------------------------------------------------------------------------------- 4. batched run ----

@pytest.mark.parametrize("counts", [[1, 64, 0, 65, 1000], [GROUP + 700, 0, 3, STEP + 1, 2 * GROUP]],
                         ids=["small", "across-steps"])
def test_batched_run_keeps_the_captures_apart(ok, counts):
    import torch
    rng = np.random.default_rng(len(counts) + counts[0])
    n = -(-(30 * max(counts) + 100) // SPB) * SPB
    caps = len(counts)
    host = np.zeros((caps, 2 * n), dtype=np.int16)
    want = []
    for c, E in enumerate(counts):
        host[c], e = with_edges(E, n, rng)
        want.append(e)
    rx = ok.Receiver(None, None, max_samples=n, max_captures=caps, threshold=THR, edge_capacity=caps * n + 64)
    dev_t = torch.from_numpy(host).cuda()
    rx.rx_device(dev_t.data_ptr(), n, num_captures=caps)
    total = 0
    for c in range(caps):
        h = check(rx, c, want[c], "capture %d of %s" % (c, counts))
        total += h["num_edges"]
        # no run spans two lists: the closed runs of a capture lie between its own first and last edge
        if h["num_edges"]:
            assert int(h["sum"].sum()) == int(want[c][-1]) - int(want[c][0])
        else:
            assert not h["count"].any() and h["open_head"] == h["samples"]
    assert total == rx.stats()["num_edges"]
    with pytest.raises(ok.OokdError) as e:
        rx.pulse_hist(caps)
    assert e.value.code == -1
    rx.close()


# ------------------------------------------------------------------------ 5. contention and spread ----

def test_every_sample_alternating(ok):
    n = 1 << 16
    iq = np.zeros(2 * n, dtype=np.int16)
    iq[0::4] = ON                                               # samples 0, 2, 4, ... on
    rx = ok.Receiver(None, None, max_samples=n, threshold=THR, edge_capacity=n + 64)
    rx.rx(iq)
    h = check(rx, 0, np.arange(n, dtype=np.uint64), "alternating")
    rx.close()
    assert h["num_edges"] == n and h["count"][1, 1] == n // 2 and h["count"][0, 1] == n // 2 - 1
    assert h["sum"][1, 1] == n // 2 and h["open_tail"] == 1 and h["tail_level"] == 0
    assert int(h["count"].sum()) == n - 1


def test_geometric_random_runs_touch_many_bins(ok):
    n = 1 << 22
    rng = np.random.default_rng(20)
    runs = rng.geometric(1.0 / 20.0, size=n // 16)
    runs = runs[:np.searchsorted(np.cumsum(runs), n - 50)].tolist()
    iq = laid(0, runs)
    rx = ok.Receiver(None, None, max_samples=n, threshold=THR)
    rx.rx(iq)
    h = check(rx, 0, None, "geometric")
    rx.close()
    assert h["num_edges"] >= n // 24
    assert np.count_nonzero(h["count"]) >= 2 * 60               # 1 .. 31 and two octaves beyond, on both levels


# ------------------------------------------------------------------------------------------ 6. reuse ----

def test_one_context_dense_sparse_empty(ok):
    n = 1 << 16
    rng = np.random.default_rng(6)
    dense = laid(0, rng.integers(1, 4, size=n // 4).tolist())
    sparse = laid(1000, [300, 5000, 300, 7000, 300])
    empty = np.zeros(2 * 5000, dtype=np.int16)
    rx = ok.Receiver(None, None, max_samples=n, threshold=THR, edge_capacity=n + 64)
    assert rx.pulse_kernel_ms == 0.0
    seen = []
    for label, iq in (("dense", dense), ("sparse", sparse), ("empty", empty), ("dense", dense)):
        rx.rx(iq)
        assert rx.pulse_kernel_ms == 0.0, label                 # nobody has asked about this run yet
        h = check(rx, 0, None, label)
        ms = rx.pulse_kernel_ms
        assert ms > 0.0, label
        again = rx.pulse_hist(0)
        assert_same_hist(again, h, label)
        assert rx.pulse_kernel_ms == ms, label                  # answered from host memory: nothing was launched
        seen.append(h)
    rx.close()
    assert seen[0]["num_edges"] > 10000 and seen[1]["num_edges"] == 6 and seen[2]["num_edges"] == 0
    assert seen[1]["runs"].tolist() == [2, 3] and not seen[2]["count"].any()
    assert seen[2]["open_head"] == seen[2]["samples"] == 8192
    assert_same_hist(seen[3], seen[0])
    # a capture of no samples at all: a valid run with an empty histogram, and nothing to launch
    rx = ok.Receiver(None, None, max_samples=n, threshold=THR)
    rx.rx(np.zeros(0, dtype=np.int16))
    h = rx.pulse_hist(0)
    assert_same_hist(h, hist_of([], 0))
    assert rx.pulse_kernel_ms == 0.0
    rx.close()


# --------------------------------------------------------------------------------------- 7. carriers ----

def test_carrier_histograms_are_the_tuned_contexts(ok):
    nu1, nu2 = 600e3 / RATE, -900e3 / RATE
    g1, _ = golden_capture("G1")
    g2, _ = golden_capture("G2")
    ext = np.zeros_like(g1)
    ext[:g2.size] = g2
    # both transmitters at half level: at full level the other one's keying transients cross the threshold
    # (tests/test_gpu_carriers.py: two_carriers)
    z = moved(g1, nu1, scale=0.5).astype(np.int32) + moved(ext, nu2, 400.0 * (1 + 0.5j), 40, seed=11, scale=0.5).astype(np.int32)
    iq = np.clip(z, -32768, 32767).astype(np.int16)
    n = iq.size // 2
    f = ok.Filter.load(golden_path("filters", "fs32_fs4"))
    carriers = [(nu1, 0.1), (nu2, 0.12)]
    rx = ok.Receiver(f, None, max_samples=n, carriers=carriers)
    rx.rx(iq)
    for k, (nu, thr) in enumerate(carriers):
        h = check(rx, k, None, "carrier %d" % k)
        one = ok.Receiver(f, None, max_samples=n, threshold=thr, tune=nu)
        one.rx(iq)
        assert one.edges().tolist() == rx.edges(k).tolist()
        assert_same_hist(check(one, 0), h, "carrier %d against its tuned context" % k)
        one.close()
        assert h["num_edges"] == (228, 136)[k]
    with pytest.raises(ok.OokdError):
        rx.pulse_hist(2)
    rx.close()


# -------------------------------------------------------------------------------------- 8. refusals ----

def test_refusals(ok, vectors):
    import torch
    n = 1 << 15
    iq = laid(10, [3] * 2000)
    # no run yet
    rx = ok.Receiver(None, None, max_samples=n, threshold=THR, edge_capacity=256)
    with pytest.raises(ok.OokdError) as e:
        rx.pulse_hist(0)
    assert e.value.code == -1 and "no finished run" in str(e.value)
    # an overflowed edge list
    with pytest.raises(ok.OokdError) as e:
        rx.rx(iq)
    assert e.value.code == -5
    with pytest.raises(ok.OokdError) as e:
        rx.pulse_hist(0)
    assert e.value.code == -5 and "overflow" in str(e.value)
    assert rx.pulse_kernel_ms == 0.0
    # the next run fits, and is answered
    rx.rx(laid(10, [3] * 100))
    assert check(rx, 0)["num_edges"] == 100               # an even number of runs: the last one is off
    rx.close()
    # a shard run
    rx = ok.Receiver(None, None, max_samples=n, threshold=THR)
    dev_t = torch.from_numpy(iq).cuda()
    rx.shard_begin(dev_t.data_ptr(), iq.size // 2, None, True, None)
    with pytest.raises(ok.OokdError) as e:
        rx.pulse_hist(0)
    assert e.value.code == -1 and "shard" in str(e.value)
    rx.rx(iq)                                                   # a whole run on the same context is answered again
    assert check(rx, 0)["num_edges"] == 2000
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
        rx.pulse_hist(0)
    assert e.value.code == -1 and "pipelined" in str(e.value)
    rx.close()
    rx = ok.Receiver(f, d, max_samples=giq.size // 2, pipeline_chunk_samples=4 * SPB, pipeline=False)
    rx.rx(giq)
    assert check(rx, 0)["num_edges"] == 228
    rx.close()
