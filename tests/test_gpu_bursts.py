"""Burst extraction on the GPU (ookd_rx_bursts, ookd_rx_copy_bursts_*; bursts.hip).  Table and cut are exact functions of
the edge list and the capture's bytes, so every comparison is equality against the restatement of the contract
(tests/bursts_contract.py) applied to `rx.edges(c)` and the capture.

The table tests use no filter: D = 1 and the edges lie where the samples put them.  Of the host test's designed cases
a capture without a filter cannot make a burst that lies wholly in the padding (a rise needs a sample): that case
stays with tests/test_bursts_host.py."""
import numpy as np
import pytest

from tests.bursts_contract import (FIELDS, RATE, SPB, THR, assert_table, bursts_of, cut_of, mapped_samples, margins,
                                   total_of)
from tests.helpers import golden_path
from tests.pulse_contract import golden_iq

pytestmark = pytest.mark.gpu

PER_VEC = {"sc16q11": 4, "cs8": 8, "cu8": 8}                    # samples of a 16-byte vector
COPY_SPAN_VECTORS = 4096                                        # vectors of one workgroup of the copy


@pytest.fixture(scope="module")
def ok():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from ookiedokie_amd import build as okbuild
    okbuild.build()
    import ookiedokie_amd as okm
    okm.lib()
    return okm


def capture_of(edges, n, fmt="sc16q11"):
    """n samples, [n, 2] in fmt's dtype, that are on exactly in the runs of `edges` at threshold 0.1, and whose bytes
    all differ from their neighbours' (a sample copied from the wrong place shows)"""
    i = np.arange(n, dtype=np.int64)
    on = np.zeros(n, dtype=bool)
    e = [int(x) for x in edges]
    for a, f in zip(e[0::2], e[1::2] + [n] * (len(e) % 2)):
        on[a:f] = True
    # (the slicer compares the magnitude: an off sample stays below 0.1 * 2048 = 204 LSB, 16 * 5 + 15 on either rail)
    v = np.stack([np.where(on, 118 + i % 9, (i * 5) % 11 - 5), (i * 3) % 11 - 5], axis=1)
    if fmt == "sc16q11":
        return (v * 16 + (i % 16)[:, None]).astype(np.int16)
    return v.astype(np.int8) if fmt == "cs8" else (v + 128).astype(np.uint8)


def edges_from(on_lengths, off_lengths, first=5):
    """on_lengths[r], then off_lengths[r] behind it"""
    e, pos = [], first
    for on, off in zip(on_lengths, off_lengths):
        e += [pos, pos + on]
        pos += on + off
    return e


def closed(e, n):
    """the run's own list of a capture designed with edges e: a capture that ends high falls at n, where the zero
    padding begins -- unless n is whole buffers and there is no padding"""
    return list(e) + ([n] if len(e) % 2 and n % SPB else [])


def run(ok, rx, cap):
    rx.rx(np.ascontiguousarray(cap).reshape(-1))
    return rx.stats()["decimated_samples"]


def check(ok, rx, cap, c, pre, post, max_gap, clean=False, what="", tables=None):
    """capture c's table and cut against the restatement over its own edge list -> (table entry, bursts, edges)"""
    n_out = rx.stats()["decimated_samples"]
    e = rx.edges(c, clean)
    t = (tables or rx.bursts(pre, post, max_gap, clean))[c]
    D = rx.total_decimation
    cap = np.asarray(cap).reshape(-1, 2)
    want = bursts_of(e, n_out, D, cap.shape[0], pre, post, max_gap)
    assert_table(t, want, what)
    assert t["num_runs"] == (e.size + 1) // 2 and (t["pre"], t["post"], t["max_gap"]) == (pre, post, max_gap), what
    assert t["decimation"] == D and t["sample_bytes"] == cap.dtype.itemsize * 2 and t["flags"] == (1 if clean else 0), what
    got = rx.burst_samples(c)
    expect = cut_of(cap, want)
    assert got.dtype == cap.dtype and got.shape == expect.shape, (what, got.shape, expect.shape)
    bad = np.nonzero((got != expect).any(axis=1))[0]
    assert bad.size == 0, (what, bad[:8].tolist(), got[bad[:4]].tolist(), expect[bad[:4]].tolist())
    return t, want, e


# --------------------------------------------------------------------------- 1. the table pass ----

def _tile(ok):
    rx = ok.Receiver(None, None, max_samples=SPB, threshold=THR)
    run(ok, rx, capture_of([10, 20], 100))
    tile = rx.bursts(1, 1, 2)[0]["tile_edges"]
    rx.close()
    assert tile >= 64 and tile % 2 == 0
    return tile


@pytest.mark.parametrize("which", ["T-1", "T", "T+1", "2T+1"])
def test_lists_around_the_tile(ok, which):
    T = _tile(ok)
    E = {"T-1": T - 1, "T": T, "T+1": T + 1, "2T+1": 2 * T + 1}[which]
    rng = np.random.default_rng(E)
    R = (E + 1) // 2
    e = edges_from(rng.integers(1, 6, R).tolist(), rng.integers(1, 13, R).tolist())
    n = e[-1] + 37
    if E % 2:
        e = e[:-1]                                              # the capture ends high, at whole buffers: the last run
        n = -(-n // SPB) * SPB                                  # stays open
    cap = capture_of(e, n)
    rx = ok.Receiver(None, None, max_samples=n, threshold=THR)
    run(ok, rx, cap)
    assert rx.bursts_kernel_ms == 0.0 and rx.burst_copy_kernel_ms == 0.0    # nobody has asked about this run yet
    t, want, got_e = check(ok, rx, cap, 0, 2, 3, 6, what=which)
    assert got_e.tolist() == e and got_e.size == E
    assert 10 < len(want) < R and any(b["burst_runs"] > 1 for b in want) and any(b["burst_runs"] == 1 for b in want)
    assert rx.bursts_kernel_ms > 0.0 and rx.burst_copy_kernel_ms > 0.0
    rx.close()


@pytest.mark.parametrize("which", ["across a boundary", "over more than a tile"])
def test_bursts_and_tile_boundaries(ok, which):
    T = _tile(ok)
    R = 2 * T                                                   # four tiles of runs
    off = np.full(R, 20)
    lo, hi = (T // 2 - 3, T // 2 + 3) if which == "across a boundary" else (T // 2 - 40, T + T // 2 + 40)
    off[lo:hi] = 2                                              # runs lo .. hi join
    e = edges_from([3] * R, off.tolist())
    n = e[-1] + 50
    cap = capture_of(e, n)
    rx = ok.Receiver(None, None, max_samples=n, threshold=THR)
    run(ok, rx, cap)
    t, want, got_e = check(ok, rx, cap, 0, 4, 5, 9, what=which)
    assert got_e.tolist() == e
    long = [b for b in want if b["burst_runs"] > 1]
    assert len(long) == 1 and long[0]["first_run"] == lo and long[0]["burst_runs"] == hi - lo + 1
    tile_runs = T // 2
    assert long[0]["first_run"] // tile_runs < (long[0]["first_run"] + long[0]["burst_runs"] - 1) // tile_runs
    if which != "across a boundary":
        assert long[0]["burst_runs"] > tile_runs + 2            # a whole tile lies inside the burst
    rx.close()


DESIGNED = [
    # name, edges, n, pre, post, max_gap
    ("no edge", [], 500, 3, 4, 10),
    ("ends high from one rise", [40], 500, 3, 4, 10),
    ("one run", [40, 50], 500, 3, 4, 10),
    ("odd, ends high", [40, 50, 100, 120, 450], 500, 3, 4, 10),
    ("open last run", [40, 50, 100, 120, 8000], SPB, 3, 4, 10),
    ("gap of exactly max_gap joins", [40, 50, 60, 70], 500, 3, 4, 10),
    ("gap of max_gap + 1 splits", [40, 50, 61, 70], 500, 3, 4, 10),
    ("pre beyond the first rise", [2, 50], 500, 30, 4, 40),
    ("rise at 0", [0, 50, 400, 410], 500, 30, 4, 40),
    ("post beyond the capture's end", [40, 50, 480, 495], 500, 3, 40, 50),
    ("every run its own burst", [10 + 50 * k + d for k in range(9) for d in (0, 5)], 500, 2, 3, 5),
    ("all runs one burst", [10 + 50 * k + d for k in range(9) for d in (0, 5)], 500, 20, 20, 45),
    ("zero margins, adjacent bursts", [10, 20, 21, 30, 31, 40], 500, 0, 0, 0),
]


def test_designed_cases(ok):
    rx = ok.Receiver(None, None, max_samples=SPB, threshold=THR)
    for name, e, n, pre, post, max_gap in DESIGNED:
        cap = capture_of(e, n)
        run(ok, rx, cap)
        t, want, got_e = check(ok, rx, cap, 0, pre, post, max_gap, what=name)
        assert got_e.tolist() == closed(e, n), name
        if name == "open last run":
            assert got_e.size % 2 == 1 and want[-1]["hi"] == n
        if name == "no edge":
            assert t["num_bursts"] == 0 and t["total_samples"] == 0 and rx.burst_samples(0).shape == (0, 2)
        if name == "gap of exactly max_gap joins":
            assert len(want) == 1
        if name == "gap of max_gap + 1 splits":
            assert len(want) == 2
        if name == "post beyond the capture's end":
            assert want[-1]["first_sample"] + want[-1]["num_samples"] == n      # clipped at n, not at n_out
        if name == "every run its own burst":
            assert len(want) == 9
        if name == "all runs one burst":
            assert len(want) == 1
    rx.close()


def test_batch_middle_empty_last_ends_high(ok):
    import torch
    rng = np.random.default_rng(5)
    n, stride = 6000, 7000
    lists = [edges_from(rng.integers(1, 9, 300).tolist(), rng.integers(1, 25, 300).tolist()), [],
             edges_from(rng.integers(1, 9, 200).tolist(), rng.integers(1, 25, 200).tolist())[:-1]]
    lists[0] = [x for x in lists[0] if x < n - 10]
    lists[0] = lists[0][:len(lists[0]) // 2 * 2]
    lists[2] = [x for x in lists[2] if x < n - 10]
    lists[2] = lists[2][:(len(lists[2]) - 1) // 2 * 2 + 1]      # odd: ends high
    caps = [capture_of(e, n) for e in lists]
    host = np.full((3, stride, 2), 30000, dtype=np.int16)       # the gaps between the captures are loud
    for c in range(3):
        host[c, :n] = caps[c]
    dev_t = torch.from_numpy(host).cuda()
    rx = ok.Receiver(None, None, max_samples=n, max_captures=3, threshold=THR)
    rx.rx_device(dev_t.data_ptr(), n, num_captures=3, stride=stride)
    tables = rx.bursts(3, 4, 9)
    assert len(tables) == 3
    ms = rx.bursts_kernel_ms
    assert ms > 0.0
    for c in (2, 0, 1):
        t, want, e = check(ok, rx, caps[c], c, 3, 4, 9, what="capture %d" % c, tables=tables)
        assert e.tolist() == lists[c] + ([n] if c == 2 else [])
    assert tables[1]["num_bursts"] == 0 and tables[0]["num_bursts"] > 20 and tables[2]["num_bursts"] > 20
    assert tables[2]["first_sample"][-1] + tables[2]["num_samples"][-1] == n
    assert rx.bursts_kernel_ms == ms                            # one pass answered all captures
    with pytest.raises(ok.OokdError) as err:
        rx.burst_samples(3)
    assert err.value.code == -1
    rx.close()


# ----------------------------------------------------------------------------------- 2. the copy ----

def _copy_layout(fmt):
    """edges (pre = post = max_gap = 0: a burst is a run) for the copy's cases -> (edges, n)"""
    V = PER_VEC[fmt]
    on, off = [], []
    # bursts of 1, 3, 4 and 5 samples in a row: vectors straddle them and swallow them
    for k in range(24):
        on.append((1, 3, 4, 5)[k % 4])
        off.append(1 + k % 3)
    e = edges_from(on, off, first=3)
    pos = e[-1] + 7
    # a source that begins one sample behind a vector boundary, against every phase of the destination
    total = sum(on)
    for phase in range(V):
        fill = (phase - total) % V
        if fill:
            e += [pos, pos + fill]
            pos += fill + 2
            total += fill
        pos += (1 - pos) % V                                    # first % V == 1: first * bytes is 4 (or 2) mod 16
        e += [pos, pos + 5 * V + 3]
        total += 5 * V + 3
        pos += 5 * V + 3 + 4
    # one burst longer than a workgroup's span, from an odd sample
    pos += (3 - pos) % V
    long = COPY_SPAN_VECTORS * V + 2 * V + 1
    e += [pos, pos + long]
    pos += long + 9
    total += long
    # ... and the total is not a multiple of a vector
    tail = 1 if (total + 1) % V else 2
    e += [pos, pos + tail]
    return e, pos + tail + 20


@pytest.mark.parametrize("fmt", ["sc16q11", "cs8", "cu8"])
def test_copy_cases(ok, fmt):
    import torch
    V = PER_VEC[fmt]
    e, n = _copy_layout(fmt)
    cap = capture_of(e, n, fmt)
    rx = ok.Receiver(None, None, max_samples=n, threshold=THR, sample_format=fmt)
    run(ok, rx, cap)
    t, want, got_e = check(ok, rx, cap, 0, 0, 0, 0, what=fmt)   # (the host copy: a device buffer of exactly `total`)
    assert got_e.tolist() == e
    total = t["total_samples"]
    assert total % V != 0 and t["sample_bytes"] == 16 // V
    lengths = [b["num_samples"] for b in want]
    assert {1, 3, 4, 5} <= set(lengths) and max(lengths) > COPY_SPAN_VECTORS * V
    phases = {b["offset"] % V for b in want if b["num_samples"] == 5 * V + 3 and b["first_sample"] % V == 1}
    assert phases == set(range(V))
    # into a larger device buffer filled with 0xA5: nothing beyond `total` is touched
    sb = t["sample_bytes"]
    room = total + 3 * V + 1
    buf = torch.full((room * sb,), 0xA5, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    assert rx.burst_samples_device(0, buf.data_ptr(), room) == total
    assert rx.burst_copy_kernel_ms > 0.0
    out = buf.cpu().numpy()
    expect = cut_of(cap, want)
    assert out[:total * sb].tobytes() == expect.tobytes()
    assert (out[total * sb:] == 0xA5).all()
    # one sample short: refused, and nothing is written
    buf.fill_(0xA5)
    with pytest.raises(ok.OokdError) as err:
        rx.burst_samples_device(0, buf.data_ptr(), total - 1)
    assert err.value.code == -5
    torch.cuda.synchronize()
    assert (buf.cpu().numpy() == 0xA5).all()
    # a destination that is only sample-aligned: the same bytes, sample by sample
    buf.fill_(0xA5)
    assert rx.burst_samples_device(0, buf.data_ptr() + sb, total) == total
    out = buf.cpu().numpy()
    assert out[sb:(total + 1) * sb].tobytes() == expect.tobytes()
    assert (out[:sb] == 0xA5).all() and (out[(total + 1) * sb:] == 0xA5).all()
    rx.close()


# ---------------------------------------------------------------------------- 3. the whole path ----

@pytest.mark.parametrize("filt", ["fs32_fs4", "fs128_fs16_dec4"])
@pytest.mark.parametrize("name", ["G1", "G2"])
def test_golden_round_trip(ok, vectors, name, filt):
    g = vectors[name]
    iq = golden_iq(vectors, name)
    n = iq.size // 2
    f = ok.Filter.load(golden_path("filters", filt))
    D = f.total_decimation
    d = ok.Device.load(golden_path("devices", g["device"]), RATE // D)
    rx = ok.Receiver(f, d, max_samples=n, threshold=THR, pipeline=False)
    whole = rx.rx(iq)
    assert len(whole.msg_samples) >= 1 and whole.stats["num_errors"] == 0
    pre, post, max_gap = margins(D)
    t, want, e = check(ok, rx, iq, 0, pre, post, max_gap, what="%s %s" % (name, filt))
    assert 1 <= len(want) and 0 < t["total_samples"] < n
    which = rx.message_bursts(whole)
    mapped, expect_which = mapped_samples(whole.msg_samples, want, D)
    assert which.dtype == np.int64 and which.tolist() == expect_which and (which >= 0).all()
    assert rx.message_bursts(whole, capture=1).tolist() == [-1] * len(which)
    cut = rx.burst_samples(0)
    again = rx.rx(cut.reshape(-1))
    assert again.payloads.tolist() == whole.payloads.tolist()
    assert again.msg_samples.tolist() == mapped
    assert again.stats["num_errors"] == whole.stats["num_errors"]
    rx.close()


def test_carrier_context_cuts_the_one_capture(ok):
    from tests.test_gpu_run_levels import _two_carriers
    iq, carriers = _two_carriers()
    n = iq.size // 2
    f = ok.Filter.load(golden_path("filters", "fs32_fs4"))
    rx = ok.Receiver(f, None, max_samples=n, carriers=[carriers[0][0], carriers[1]], threshold=carriers[0][1])
    rx.rx(iq)
    pre, post, max_gap = margins(f.total_decimation)
    tables = rx.bursts(pre, post, max_gap)
    assert len(tables) == 2
    for k in range(2):
        t, want, e = check(ok, rx, iq, k, pre, post, max_gap, what="carrier %d" % k, tables=tables)
        assert e.size > 100 and t["num_bursts"] >= 1
    assert tables[0]["num_runs"] != tables[1]["num_runs"]        # two lists, one capture
    rx.close()


@pytest.mark.parametrize("debounced", [False, True], ids=["clean_edges", "debounced-context"])
def test_clean_list(ok, debounced):
    from tests.test_gpu_run_levels import _glitched
    iq = _glitched()
    n = iq.size // 2
    rx = ok.Receiver(None, None, max_samples=n, threshold=THR, min_off=5 if debounced else 0)
    rx.rx(iq)
    if not debounced:
        with pytest.raises(ok.OokdError) as err:
            rx.bursts(0, 0, 0, clean=True)
        assert err.value.code == -1 and "cleaned list" in str(err.value)
        rx.clean_edges(0, 5)
    # with no margins a burst is a run: the raw list's dropouts split two of them, the cleaned list's do not
    t, want, e = check(ok, rx, iq, 0, 0, 0, 0, clean=True, what="cleaned list")
    assert e.tolist() == [1000, 1100, 3000, 3400, 5000, 5100, 9000, 9700]
    assert t["first_sample"].tolist() == [1000, 3000, 5000, 9000] and t["num_samples"].tolist() == [100, 400, 100, 700]
    ms_clean = rx.bursts_kernel_ms
    raw, _, e_raw = check(ok, rx, iq, 0, 0, 0, 0, what="raw list")
    assert e_raw.size == 12 and raw["num_bursts"] == 6
    # the copy follows the form last asked about
    rx.bursts(0, 0, 0, clean=True)
    assert rx.bursts_kernel_ms == ms_clean and rx.burst_samples(0).shape[0] == 1300
    rx.bursts(0, 0, 0)
    assert rx.burst_samples(0).shape[0] == 1294
    # other minimums on the same run: another cleaned list, and a new table about that one
    rx.clean_edges(0, 2000)
    t2, want2, e2 = check(ok, rx, iq, 0, 0, 0, 0, clean=True, what="cleaned again")
    assert e2.tolist() == [1000, 5100, 9000, 9700] and t2["num_samples"].tolist() == [4100, 700]
    check(ok, rx, iq, 0, 0, 0, 0, what="raw list afterwards")
    rx.close()


def test_refusals(ok, vectors):
    import torch
    n = 1 << 14
    e = edges_from([3] * 500, [8] * 500)
    cap = capture_of(e, n)
    iq = np.ascontiguousarray(cap).reshape(-1)
    rx = ok.Receiver(None, None, max_samples=n, threshold=THR)
    # no run yet
    with pytest.raises(ok.OokdError) as err:
        rx.bursts(1, 1, 2)
    assert err.value.code == -1 and "no finished run" in str(err.value)
    with pytest.raises(ok.OokdError) as err:
        rx.burst_samples(0)
    assert err.value.code == -1 and "ookd_rx_bursts first" in str(err.value)
    # a run in flight
    dev_t = torch.from_numpy(iq).cuda()
    rx.submit_device(dev_t.data_ptr(), n)
    with pytest.raises(ok.OokdError) as err:
        rx.bursts(1, 1, 2)
    assert err.value.code == -1 and "ookd_rx_wait first" in str(err.value)
    rx.wait()
    # the copy before the table; max_gap below pre + post; a capture out of range
    with pytest.raises(ok.OokdError) as err:
        rx.burst_samples(0)
    assert err.value.code == -1 and "ookd_rx_bursts first" in str(err.value)
    with pytest.raises(ok.OokdError) as err:
        rx.bursts(3, 4, 6)
    assert err.value.code == -1 and "max_gap" in str(err.value)
    assert rx.bursts_kernel_ms == 0.0
    assert rx.bursts(3, 4, 7)[0]["num_bursts"] == 500
    with pytest.raises(ok.OokdError) as err:
        rx.burst_samples(1)
    assert err.value.code == -1 and "capture 1 of 1" in str(err.value)
    # a new run: the table was the last run's
    rx.rx_device(dev_t.data_ptr(), n)
    assert rx.bursts_kernel_ms == 0.0
    with pytest.raises(ok.OokdError) as err:
        rx.burst_samples(0)
    assert err.value.code == -1
    # a shard run
    rx.shard_begin(dev_t.data_ptr(), n, None, True, None)
    with pytest.raises(ok.OokdError) as err:
        rx.bursts(1, 1, 2)
    assert err.value.code == -1 and "shard" in str(err.value)
    rx.rx(iq)                                                   # a whole run on the same context is answered again
    assert rx.bursts(1, 1, 2)[0]["num_bursts"] == 500
    rx.close()
    # a pipelined run (needs a state machine behind the front end)
    g = vectors["G1"]
    giq = golden_iq(vectors, "G1")
    f = ok.Filter.load(golden_path("filters", g["filter"]))
    d = ok.Device.load(golden_path("devices", g["device"]), RATE // f.total_decimation)
    rx = ok.Receiver(f, d, max_samples=giq.size // 2, pipeline_chunk_samples=4 * SPB)
    res = rx.rx(giq)
    assert res.stats["pipeline_chunks"] >= 2
    with pytest.raises(ok.OokdError) as err:
        rx.bursts(1, 1, 2)
    assert err.value.code == -1 and "pipelined" in str(err.value)
    rx.close()


def test_same_parameters_launch_nothing_and_an_unasked_run_costs_nothing(ok):
    e = edges_from([3] * 300, [7, 30] * 150)
    n = e[-1] + 100
    cap = capture_of(e, n)
    rx = ok.Receiver(None, None, max_samples=n, threshold=THR)
    run(ok, rx, cap)
    assert rx.bursts_kernel_ms == 0.0 and rx.burst_copy_kernel_ms == 0.0
    before = (rx.result(), rx.edges(0), rx.stats(), rx.bits(0))
    first = rx.bursts(2, 3, 10)
    ms = rx.bursts_kernel_ms
    assert ms > 0.0 and first[0]["num_bursts"] == 150
    again = rx.bursts(2, 3, 10)
    assert rx.bursts_kernel_ms == ms                            # the same float: no second pass was timed
    for k in FIELDS:
        assert again[0][k].tolist() == first[0][k].tolist()
    other = rx.bursts(2, 3, 40)                                 # other parameters: a new table
    assert other[0]["num_bursts"] == 1
    check(ok, rx, cap, 0, 2, 3, 40)
    after = (rx.result(), rx.edges(0), rx.stats(), rx.bits(0))
    assert after[1].tolist() == before[1].tolist() and after[2] == before[2] and np.array_equal(after[3], before[3])
    assert after[0].msg_samples.tolist() == before[0].msg_samples.tolist()
    # the next run nobody asks about reports both times 0
    run(ok, rx, cap)
    assert rx.bursts_kernel_ms == 0.0 and rx.burst_copy_kernel_ms == 0.0
    rx.close()


# ---------------------------------------------------------------------------------- 4. the example ----

def test_c_example_bursts(ok, vectors, tmp_path):
    """examples/ookd_rx.c --bursts: stdout is what it is without the option (but for the wall clock in the first
    column), the file is Python's cut, its .idx the table, and the file decodes like the input"""
    import subprocess
    from tests.test_host import _build_c_example
    exe = _build_c_example(tmp_path)
    g = vectors["G1"]
    iq = golden_iq(vectors, "G1")
    cap = tmp_path / "g1.sc16q11"
    iq.tofile(str(cap))
    cut_path = tmp_path / "cut.sc16q11"
    tail = [golden_path("devices", g["device"]), golden_path("filters", "fs32_fs4"), str(RATE), "csv"]
    plain = subprocess.run([exe, str(cap)] + tail, capture_output=True, text=True, timeout=120)
    us = dict(pre=200, post=18400, gap=18600)
    cutting = subprocess.run([exe, "--bursts", str(cut_path), "--burst-pre-us", str(us["pre"]), "--burst-post-us", str(us["post"]),
                              "--burst-gap-us", str(us["gap"]), str(cap)] + tail, capture_output=True, text=True, timeout=120)
    assert plain.returncode == 0 and cutting.returncode == 0, (plain.stderr, cutting.stderr)
    fields = lambda text: [ln.split(",", 1)[1:] for ln in text.split("\n")]         # (the first is the wall clock)
    assert fields(cutting.stdout) == fields(plain.stdout) and len(plain.stdout.strip().split("\n")) == 4
    assert "bursts" not in plain.stderr and "bursts: " in cutting.stderr
    f = ok.Filter.load(golden_path("filters", "fs32_fs4"))
    D = f.total_decimation
    d = ok.Device.load(golden_path("devices", g["device"]), RATE // D)
    rx = ok.Receiver(f, d, max_samples=iq.size // 2, threshold=THR)
    rx.rx(iq)
    pre, post, max_gap = (us[k] * (RATE // D) // 1000000 for k in ("pre", "post", "gap"))
    t = rx.bursts(pre, post, max_gap)[0]
    want = rx.burst_samples(0)
    rx.close()
    got = np.fromfile(str(cut_path), dtype=np.int16)
    assert got.tobytes() == want.tobytes() and got.size == 2 * t["total_samples"] > 0
    idx = [[int(x) for x in ln.split()] for ln in open(str(cut_path) + ".idx").read().strip().split("\n")]
    assert idx == [[int(t["first_sample"][b]), int(t["num_samples"][b]), int(t["offset"][b])] for b in range(t["num_bursts"])]
    again = subprocess.run([exe, str(cut_path)] + tail, capture_output=True, text=True, timeout=120)
    assert again.returncode == 0, again.stderr
    assert fields(again.stdout) == fields(plain.stdout)
