"""The scan's result stage -- leaf records, finish kernels, append pool, message and error lists, the merge of refused
captures -- on the designed devices of tests/dense_devices.py, which fill a span, a finish block, a payload and the
lists to their limits and one beyond (the shipped devices stay far inside all of them).  Everything is bit-exact
against the CPU oracle; what the inputs hold is checked without a GPU in test_dense_results_host.py.

A span (leaf) of the scan holds the samples behind one edge up to and including the next edge.  Expected fsm_path per
case, from the constants (DESIGN 4.6 "limits of a span's record and of the result lists"): 1 = the scan kept the capture,
3 = it refused it and the round form decoded it, 2 = the device is outside the scan's domain (or the rounds were asked
for)."""
import numpy as np
import pytest

from tests import dense_devices as dd
from tests.helpers import edges_of, stream_from_runs
from tests.test_gpu_parity import _sync_walk_forced

pytestmark = pytest.mark.gpu

ERR_CAPACITY = -5           # OOKD_ERR_CAPACITY


@pytest.fixture(scope="module")
def ok():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from ookiedokie_amd import build as okbuild
    okbuild.build()
    import ookiedokie_amd as okm
    okm.lib()
    return okm


# (name, Receiver arguments, walk from synchronising spans forced, pipelined in chunks of 4 buffers)
LEGS = (("tables", dict(), False, False),
        ("sims", dict(scan_sims=True), False, False),
        ("composed", dict(scan_tables=True), False, False),
        ("walk", dict(), True, False),
        ("pipelined", dict(), False, True),
        ("pipelined+walk", dict(), True, True),
        ("rounds", dict(fsm_rounds=True, quiet_skip=False), False, False))


def _same(rx, got, want, tag):
    assert list(got.msg_samples) == list(want.msg_samples), tag
    assert got.payloads.shape == want.payloads.shape and (got.payloads == want.payloads).all(), tag
    errs, nerr = rx.errors(len(want.err_samples) + 8)
    assert nerr == len(want.err_samples) == got.stats["num_errors"], tag
    assert list(errs) == list(want.err_samples), tag


def _legs(ok, oracle, dev, iq, spb, path, legs=None, reason=0, pipelined=None, segment_buffers=None):
    """The capture through every form of the state machine, each against the oracle: message samples, payloads, the
    error count and every error position, num_edges, and fsm_path -- `path` on the scan legs (2 wherever the device is
    outside the scan's domain), 2 on the rounds leg.  reason: bits fsm_fallback_reason must hold when path is 3.
    pipelined: the pipelined legs must (True) report two chunks or more.  Returns {leg: stats}."""
    d = dd.ok_device(ok, dev)
    od = dd.fsm_desc(oracle, dev)
    n = iq.size // 2
    want = oracle.rx(iq, None, dd.THR, od, spb, want_bits=True, msg_cap=1 << 17)
    nedges = len(edges_of(want.bits))
    M = len(want.msg_samples)
    nbuf = -(-n // spb)
    if dd.scan_domain(dev) > dd.SCAN_DOMAIN_MAX:
        path = 2
    seen = {}
    for name, kw, walk, chunked in LEGS:
        if legs is not None and name not in legs:
            continue
        # room in a segment for all the messages: on the rounds leg, and wherever the scan hands the capture over
        kw = dict(kw, message_slots=M + 2)
        if chunked:
            kw["pipeline_chunk_samples"] = 4 * spb
        if name == "rounds":
            # segments of an eighth of the capture (whole buffers)
            kw["segment_buffers"] = segment_buffers if segment_buffers is not None else max(1, nbuf // 8)
        with _sync_walk_forced(walk):
            rx = ok.Receiver(None, d, max_samples=max(n, 1), threshold=dd.THR, samples_per_buffer=spb,
                             message_capacity=M + 64, **kw)
        got = rx.rx(iq)
        tag = (dev["name"], spb, name, got.stats["fsm_path"], got.stats["fsm_fallback_reason"])
        print("dense-results %s spb %d leg %-14s fsm_path %d (expected %d) reason %d chunks %d entry %d"
              % (dev["name"], spb, name, got.stats["fsm_path"], 2 if name == "rounds" else path,
                 got.stats["fsm_fallback_reason"], got.stats["pipeline_chunks"], got.stats["scan_entry_form"]))
        _same(rx, got, want, tag)
        assert got.stats["num_edges"] == nedges, tag
        assert got.stats["decimated_samples"] == want.decimated, tag
        assert got.stats["fsm_path"] == (2 if name == "rounds" else path), tag
        if path == 3 and name != "rounds":
            assert got.stats["fsm_fallback_reason"] != 0 and got.stats["fsm_fallback_reason"] & reason == reason, tag
        if path == 1 and name != "rounds":
            # (16: the forced walk from synchronising spans gave up and the scan composed: no refusal of the capture)
            assert got.stats["fsm_fallback_reason"] in ((0, 16) if walk else (0,)), tag
        if chunked and pipelined:
            assert got.stats["pipeline_chunks"] >= 2, tag
        seen[name] = got.stats
        rx.close()
    d.close()
    return want, seen


# ------------------------------------------------------------------------------------------- dense messages ----

@pytest.mark.parametrize("spb", [4096, 1000])
@pytest.mark.parametrize("nbits", dd.BURST_BITS)
def test_dense_messages(ok, oracle, nbits, spb):
    """3000 messages of burst(1 / 8 / 9), one every 0.4 to 0.8 ms: 12 000 to 60 000 leaves in 12 to 59 finish blocks,
    messages across block ends, more than the 2048 of the pinned head; pipelined, the chunk before's totals are where
    a chunk starts resolving.  The scan keeps them all (fsm_path 1)."""
    dev, runs = dd.burst_case(nbits)
    want, seen = _legs(ok, oracle, dev, dd.iq_of(runs), spb, path=1, pipelined=True)
    assert len(want.msg_samples) == dd.BURST_MESSAGES > dd.HOST_MSG_FIRST
    if spb == 4096:
        # message 2047 and message 2048 come from different chunks (of 4 buffers)
        a, b = (int(want.msg_samples[i]) // (4 * spb) for i in (dd.HOST_MSG_FIRST - 1, dd.HOST_MSG_FIRST))
        assert a != b
        assert seen["pipelined"]["pipeline_chunks"] > b


# ------------------------------------------------------------------------------- compact against full record ----

@pytest.mark.parametrize("z", dd.COMPACT_Z)
def test_compact_against_full_record(ok, oracle, z):
    """rle(40) with z appends in one span: up to 8 the one-word record holds the span (and its first 8 append values),
    from 9 on the 48-byte record does.  (put_event with `napp > 9u` loses the ninth value of z = 9; fin_write with
    `j < 8` those of z = 9 and 16: payloads differ.)"""
    dev, runs = dd.rle_case(z)
    want, _ = _legs(ok, oracle, dev, dd.iq_of(runs), 4096, path=1)
    assert len(want.msg_samples) == 20


# ----------------------------------------------------------------------------------------------- span limits ----

@pytest.mark.parametrize("z,path", [(30, 1), (31, 3)])
def test_appends_per_span_limit(ok, oracle, z, path):
    """kMaxLeafApps = 30 appends in one span is the last the record holds; 31 sets `overflow`: the capture goes to the
    round form (fsm_path 3) and comes out as the oracle's all the same"""
    dev, runs = dd.rle_case(z)
    _legs(ok, oracle, dev, dd.iq_of(runs), 4096, path=path)


@pytest.mark.parametrize("outputs,path", [(1, 1), (2, 1), (3, 3), (4, 3)])
def test_outputs_per_span_limit(ok, oracle, outputs, path):
    """ticker: the record holds two outputs of one span; a third refuses the capture"""
    dev, runs = dd.ticker_case(outputs)
    want, _ = _legs(ok, oracle, dev, dd.iq_of(runs), 4096, path=path)
    assert len(want.msg_samples) == 100 * outputs


@pytest.mark.parametrize("fires,path", [(47, 1), (48, 1), (49, 3)])
def test_firings_per_span_limit(ok, oracle, fires, path):
    """pacer: sim_span gives up when it is to go on with more than kMaxFires = 48 firings behind it.  48 time-outs and
    the falling edge's own firing on the span's last sample are still simulated; 49 time-outs are not.  (rle cannot get
    here -- 31 appends refuse first -- nor ticker: three outputs do.)"""
    dev, runs = dd.pacer_case(fires)
    want, _ = _legs(ok, oracle, dev, dd.iq_of(runs), 4096, path=path, legs=("sims", "rounds", "tables", "walk"))
    assert len(want.msg_samples) == 0 and len(want.err_samples) == 0


# ----------------------------------------------------------------------------------------------- append pool ----

def _batch(caps):
    """captures of different lengths as one batch: (host array [captures, 2 * stride], samples, stride)"""
    n = max(x.size // 2 for x in caps)
    n += (-n) % 4
    stride = n + 8
    host = np.zeros((len(caps), 2 * stride), dtype=np.int16)
    for c, x in enumerate(caps):
        host[c, :x.size] = x
    return host, n, stride


def _run_batch(ok, oracle, rx, od, host, n, stride, order, path, spb=8192):
    import torch
    sub = torch.from_numpy(host[list(order)].copy()).cuda()
    torch.cuda.synchronize()            # (the context's stream does not wait for the copy's)
    got = rx.rx_device(sub.data_ptr(), n, num_captures=len(order), stride=stride)
    assert got.stats["fsm_path"] == path, got.stats
    total, errs_want = 0, []
    for i, c in enumerate(order):
        want = oracle.rx(host[c, :2 * n], None, dd.THR, od, spb, msg_cap=1 << 17)
        gc = got.for_capture(i)
        assert list(gc.msg_samples) == list(want.msg_samples), (order, c)
        assert (gc.payloads == want.payloads).all(), (order, c)
        total += len(want.msg_samples)
        errs_want.append(list(want.err_samples))
    assert total == len(got.msg_samples)
    return got, total, errs_want


def test_append_pool_limit(ok, oracle):
    """A capture's append values live in a pool of 2 * (edges + 1) + 512 bytes.  A capture with exactly that many
    appends stays in the scan; with one more it is refused with kFbPool.  In a batch the pool lies in front of the next
    capture's: the refused capture is redone alone, its neighbours keep the scan's result, and the context then runs a
    clean batch."""
    for extra, path in ((0, 1), (1, 3)):
        dev, runs = dd.pool_case(extra)
        _legs(ok, oracle, dev, dd.iq_of(runs), 4096, path=path, reason=dd.FB_POOL,
              legs=("tables", "sims", "walk", "rounds"))
    dev = dd.rle(dd.RLE_BITS)
    d, od = dd.ok_device(ok, dev), dd.fsm_desc(oracle, dev)
    # (the neighbours are rle streams: one device per context, and behind a burst stream rle's `off` would go on
    #  appending through the zeros a capture is padded with, past kMaxLeafApps)
    others = [dd.iq_of(dd.rle_runs(dd.RLE_BITS, 3 + c, 20, seed=900 + c)) for c in range(3)]
    caps = [others[0], dd.iq_of(dd.pool_runs(1)), others[1], others[2]]
    host, n, stride = _batch(caps)
    assert n == caps[1].size // 2 and n % 8192 == 0         # the pool capture is not padded: its appends stay as laid
    rx = ok.Receiver(None, d, max_samples=n, max_captures=len(caps), message_capacity=1024)
    for order in ((0, 1, 2, 3), (0, 2, 3)):
        got, total, _ = _run_batch(ok, oracle, rx, od, host, n, stride, order, 3 if 1 in order else 1)
        assert total >= 40
        if 1 in order:
            assert got.stats["fsm_fallback_reason"] & dd.FB_POOL
    rx.close()
    d.close()


# ------------------------------------------------------------------------- the workspace at its smallest ----

def _tight_batch(captures=3, n=4096):
    """burst(8) messages back to back (some 20 to 40 us apart) in `captures` captures of n samples, and in each
    capture three pulses too short for `on`: an error each, the rest of that buffer dropped"""
    caps = []
    for c in range(captures):
        runs = dd.burst_runs(8, 12, seed=950 + c, lead=30 + 7 * c, gap=(20, 40))
        for at in (41, 101, 161):       # (odd: a pulse) 20 us -> 5 us, the low run behind it takes the rest
            runs[at], runs[at + 1] = 5, runs[at + 1] + 15
        caps.append(dd.iq_of(stream_from_runs(runs)[:n]))
    return caps


@pytest.mark.parametrize("leg", ["tables", "walk", "composed"])
def test_small_batch_in_a_workspace_of_mostly_pads(ok, oracle, leg):
    """Three captures of four buffers of 1024 samples with an edge_capacity of exactly the batch's edges: the scan's
    workspace is a handful of blocks and groups plus its per-capture pads (blocks_cap = edges / leaf_block + captures
    + 8), so cap_first, the sync walk's digests and selections and every per-capture prefix lie as close to the end of
    their allocations as they ever do.  Messages, payloads, every error position and num_edges against the oracle."""
    spb = 1024
    dev = dd.burst(8)
    d, od = dd.ok_device(ok, dev), dd.fsm_desc(oracle, dev)
    host, n, stride = _batch(_tight_batch())
    assert n == 4 * spb
    wants = [oracle.rx(host[c, :2 * n], None, dd.THR, od, spb, want_bits=True) for c in range(len(host))]
    edges = [len(edges_of(w.bits)) for w in wants]
    print("small batch: edges %s messages %s errors %s" % (edges, [len(w.msg_samples) for w in wants],
                                                         [len(w.err_samples) for w in wants]))
    assert all(100 <= e <= 400 for e in edges) and all(len(w.msg_samples) >= 2 and len(w.err_samples) >= 2 for w in wants)
    kw, walk = next((kw, walk) for name, kw, walk, _ in LEGS if name == leg)
    with _sync_walk_forced(walk):
        rx = ok.Receiver(None, d, max_samples=n, max_captures=len(host), threshold=dd.THR, samples_per_buffer=spb,
                         edge_capacity=sum(edges), message_capacity=256, **kw)
    import torch
    dev_iq = torch.from_numpy(host).cuda()
    torch.cuda.synchronize()            # (the context's stream does not wait for the copy's)
    got = rx.rx_device(dev_iq.data_ptr(), n, num_captures=len(host), stride=stride)
    assert got.stats["fsm_path"] == 1 and got.stats["num_edges"] == sum(edges), got.stats
    for c, want in enumerate(wants):
        gc = got.for_capture(c)
        assert list(gc.msg_samples) == list(want.msg_samples), (leg, c)
        assert gc.payloads.shape == want.payloads.shape and (gc.payloads == want.payloads).all(), (leg, c)
    errs_want = [int(e) for w in wants for e in w.err_samples]         # capture-major
    errs, nerr = rx.errors(len(errs_want) + 8)
    assert nerr == len(errs_want) == got.stats["num_errors"] and list(errs) == errs_want, leg
    rx.close()
    d.close()


# --------------------------------------------------------------------------------------------- long payloads ----

LONG_CASES = [(k, n) for n in dd.LONG_BITS for k in ("rle", "burst")] + [("drip", n) for n in dd.DRIP_BITS]


def _long_path(dev):
    return 1 if dd.scan_domain(dev) <= dd.SCAN_DOMAIN_MAX else 2


@pytest.mark.parametrize("kind,nbits", LONG_CASES)
def test_long_payloads(ok, oracle, kind, nbits):
    """Payloads of 63 to 254 bits: fin_msg packs four 64-bit words and masks the last by the payload's bytes.  burst and
    rle have four states: the scan's domain (states * (bits + 2) + 3 <= 384) ends at 93 bits, beyond it the context
    runs the round form (fsm_path 2); drip has two and stays in the scan up to 188 bits -- payload word 2.  No device
    of 189 bits or more fits the domain: word 3 of a payload is never resolved by the scan."""
    dev, runs = dd.long_case(kind, nbits)
    want, _ = _legs(ok, oracle, dev, dd.iq_of(runs), 4096, path=1)
    words = (nbits + 63) // 64
    w = np.zeros((len(want.payloads), 32), np.uint8)
    w[:, :want.payloads.shape[1]] = want.payloads
    assert list((w.view(np.uint64) != 0).any(axis=0)) == [True] * words + [False] * (4 - words)


@pytest.mark.parametrize("kind,nbits", LONG_CASES)
def test_long_payloads_across_a_chunk_boundary(ok, oracle, kind, nbits):
    """The same streams, moved so that a chunk of the pipelined run (4 buffers of 1024) ends inside a message with all
    its bits but one collected: fin_write seeds the next chunk's pool from every word of the carried state.  (Chunks
    need the scan: beyond its domain the run is not pipelined and the round form carries the payload.)"""
    dev, runs = dd.long_case(kind, nbits)
    stream = stream_from_runs(runs)
    moved = dd.moved_to_boundary(oracle, dev, stream, nbits - 1, 4096)
    held = [nb for _, nb in dd.collected_at(oracle, dev, moved, 4096, np.arange(4096, moved.size, 4096))]
    assert max(held) >= nbits - 1
    path = _long_path(dev)
    _legs(ok, oracle, dev, dd.iq_of(moved), 1024, path=path, legs=("pipelined", "pipelined+walk"),
          pipelined=path == 1)


@pytest.mark.parametrize("kind,nbits", LONG_CASES)
def test_long_payloads_across_a_shard_boundary(ok, oracle, kind, nbits):
    """Two shards (ookd_rx_shard_begin / ookd_rx_shard_refine) cut where the first one's message has all its bits but
    one: the carried ookd_fsm_state holds the oracle's state, bit count and payload bytes -- words 1 to 3 for the
    longest --, and the second shard finishes the message."""
    import torch
    spb = 64
    dev, runs = dd.long_case(kind, nbits)
    stream = stream_from_runs(runs)
    stream = np.concatenate([stream, np.zeros(-stream.size % spb, np.uint8)])
    cuts = np.arange(spb, stream.size, spb)
    held = dd.collected_at(oracle, dev, stream, spb, cuts)
    best = max(range(len(cuts)), key=lambda i: held[i][1] if held[i][0] != 0 and held[i][1] < nbits else -1)
    cut = int(cuts[best])
    state, nb, data = dd.carried_at(oracle, dev, stream, cut)
    assert state != 0 and nbits - 8 <= nb < nbits, (nb, nbits)
    iq = dd.iq_of(stream)
    n = stream.size
    d, od = dd.ok_device(ok, dev), dd.fsm_desc(oracle, dev)
    want = oracle.rx(iq, None, dd.THR, od, spb)
    dev_t = torch.from_numpy(iq.copy()).cuda()
    torch.cuda.synchronize()
    for walk in (False, True):
        slots = len(want.msg_samples) + 2
        with _sync_walk_forced(walk):
            rx0 = ok.Receiver(None, d, max_samples=cut, samples_per_buffer=spb, message_slots=slots)
            rx1 = ok.Receiver(None, d, max_samples=n - cut, samples_per_buffer=spb, message_slots=slots)
        assert rx0.halo_samples == 0
        r0, s0 = rx0.shard_begin(dev_t.data_ptr(), cut, None, False, None)
        rx1.shard_begin(dev_t.data_ptr() + 4 * cut, n - cut, None, True, None)
        r1, s1 = rx1.shard_refine(s0)
        tag = (kind, nbits, walk, r0.stats["fsm_path"], r1.stats["fsm_path"], r1.stats["fsm_fallback_reason"])
        print("dense-results shards %s%d walk %s fsm_path %d / %d (expected %d) reason %d / %d carried bits %d"
              % (kind, nbits, walk, r0.stats["fsm_path"], r1.stats["fsm_path"], _long_path(dev),
                 r0.stats["fsm_fallback_reason"], r1.stats["fsm_fallback_reason"], s0.num_bits))
        assert (s0.state, s0.num_bits) == (state, nb), tag
        assert bytes(s0.payload)[:len(data)] == data, tag
        carried = np.frombuffer(bytes(s0.payload)[:32], np.uint64)
        assert [bool(x) for x in carried != 0][:(nb + 63) // 64] == [True] * ((nb + 63) // 64), tag
        # the first shard runs from the reset state as a capture does.  The second one's path is that of its
        # speculative pass from the reset state, begun in the middle of a message (a pulse cut in two, bits without
        # their start): the scan may refuse that and the rounds then also take the refinement (3)
        assert r0.stats["fsm_path"] == _long_path(dev), tag
        assert r1.stats["fsm_path"] in (_long_path(dev), 3), tag
        msgs = [int(x) for x in r0.msg_samples] + [int(x) + cut for x in r1.msg_samples]
        pays = [bytes(p) for p in r0.payloads] + [bytes(p) for p in r1.payloads]
        assert msgs == list(want.msg_samples), tag
        assert pays == [bytes(p) for p in want.payloads], tag
        rx0.close()
        rx1.close()
    d.close()


# ---------------------------------------------------------------------- more than 2048 messages in the merge ----

def _refused_burst_capture(nmsg=30, seed=77):
    """a burst(8) stream with, in one 50 us gap, seven 1 us pulses between two bit windows: fourteen edges on which
    nothing fires, deeper than the scan's stuck codes hold -- the scan refuses the capture"""
    runs = dd.burst_runs(8, nmsg, seed=seed)
    at = next(i for i in range(2, len(runs)) if runs[i] == 50 and runs[i - 1] == 20 and i > 200)
    runs[at:at + 1] = [25] + [1, 1] * 6 + [1] + [50 - 25 - 13]        # low 25, seven pulses of 1 us, low 12
    return runs


def test_more_than_2048_messages_through_the_merge(ok, oracle):
    """Four burst(8) captures of 900 messages and one the scan refuses: redo_refused_captures stitches the pinned
    head (2048 messages) and the device tail of the scan's list together, redoes the refused capture in the round form
    and merges in capture order."""
    dev = dd.burst(8)
    d, od = dd.ok_device(ok, dev), dd.fsm_desc(oracle, dev)
    caps = [dd.iq_of(dd.burst_runs(8, 900, seed=800 + c)) for c in range(4)]
    caps.insert(2, dd.iq_of(_refused_burst_capture()))
    host, n, stride = _batch(caps)
    solo = ok.Receiver(None, d, max_samples=n)
    r = solo.rx(host[2, :2 * n])
    assert r.stats["fsm_path"] == 3 and r.stats["fsm_fallback_reason"] != 0     # (otherwise this test tests nothing)
    solo.close()
    rx = ok.Receiver(None, d, max_samples=n, max_captures=len(caps), message_capacity=4096)
    for order in ((0, 1, 2, 3, 4), (0, 1, 3, 4)):
        got, total, _ = _run_batch(ok, oracle, rx, od, host, n, stride, order, 3 if 2 in order else 1)
        assert total > dd.HOST_MSG_FIRST and total == 3600 + (30 if 2 in order else 0)
        assert list(got.captures) == sorted(got.captures)
    rx.close()
    d.close()


# -------------------------------------------------------------------------------- capacities, clean refusals ----

def _capacity_error(ok, rx, run):
    try:
        got = run()
    except ok.OokdError as e:
        assert e.code == ERR_CAPACITY, e
        return str(e)
    pytest.fail("no capacity error: %d messages, per capture %s, %s"
                % (len(got.msg_samples), np.bincount(got.captures.astype(np.int64)).tolist(), got.stats))


@pytest.mark.parametrize("case", ["burst8", "ticker2"])
@pytest.mark.parametrize("form", ["scan", "rounds"])
def test_message_capacity_is_exact_and_its_overflow_clean(ok, oracle, case, form):
    """message_capacity = M, the oracle's count, decodes; M - 1 fails with the capacity error -- fin_write and gather
    store no slot at or beyond the capacity, collect_results reports the overflow -- and does not decode something or
    touch what lies behind its lists: a context of the right size, run right after, decodes exactly, and the small one
    then decodes a shorter capture that fits.  (3000 messages: the list's device tail; 200: all in the pinned head.)"""
    dev, runs = dd.burst_case(8) if case == "burst8" else dd.ticker_case(2)
    iq = dd.iq_of(runs)
    n = iq.size // 2
    short = iq[:2 * (n // 3)]
    d, od = dd.ok_device(ok, dev), dd.fsm_desc(oracle, dev)
    want = oracle.rx(iq, None, dd.THR, od, 4096)
    want_short = oracle.rx(short, None, dd.THR, od, 4096)
    M = len(want.msg_samples)
    assert 0 < len(want_short.msg_samples) < M - 1
    kw = dict(samples_per_buffer=4096)
    if form == "rounds":
        kw.update(fsm_rounds=True, quiet_skip=False, message_slots=M + 2, segment_buffers=max(1, n // 4096 // 8))
    good = ok.Receiver(None, d, max_samples=n, message_capacity=M, **kw)
    small = ok.Receiver(None, d, max_samples=n, message_capacity=M - 1, **kw)
    for _ in range(2):
        text = _capacity_error(ok, small, lambda: small.rx(iq))
        assert "message list overflow" in text and "capacity %d" % (M - 1) in text, text
        got = good.rx(iq)
        assert got.stats["fsm_path"] == (1 if form == "scan" else 2)
        _same(good, got, want, (case, form))
        got = small.rx(short)
        _same(small, got, want_short, (case, form, "short"))
    good.close()
    small.close()
    d.close()


def test_message_capacity_overflow_in_the_merge_of_a_batch(ok, oracle):
    """the batch-merge form: the scan's part of the list fits the capacity, the refused capture's messages do not"""
    dev = dd.burst(8)
    d, od = dd.ok_device(ok, dev), dd.fsm_desc(oracle, dev)
    caps = [dd.iq_of(dd.burst_runs(8, 40, seed=810)), dd.iq_of(_refused_burst_capture()),
            dd.iq_of(dd.burst_runs(8, 40, seed=811))]
    host, n, stride = _batch(caps)
    M = 40 + 30 + 40
    good = ok.Receiver(None, d, max_samples=n, max_captures=3, message_capacity=M)
    small = ok.Receiver(None, d, max_samples=n, max_captures=3, message_capacity=M - 1)
    import torch
    all3 = torch.from_numpy(host.copy()).cuda()
    torch.cuda.synchronize()
    for it in range(2):
        print("dense-results merge overflow, pass", it)
        text = _capacity_error(ok, small, lambda: small.rx_device(all3.data_ptr(), n, num_captures=3, stride=stride))
        assert "message list overflow" in text, text
        got, total, _ = _run_batch(ok, oracle, good, od, host, n, stride, (0, 1, 2), 3)
        assert total == M
        _run_batch(ok, oracle, small, od, host, n, stride, (0, 2), 1)          # a clean batch that fits
    good.close()
    small.close()
    d.close()


def test_default_message_slots_overflow_names_the_slots(ok, oracle):
    """the round form with its default 32 message slots a segment, on 3000 messages in five segments"""
    dev, runs = dd.burst_case(8)
    iq = dd.iq_of(runs)
    d, od = dd.ok_device(ok, dev), dd.fsm_desc(oracle, dev)
    rx = ok.Receiver(None, d, max_samples=iq.size // 2, samples_per_buffer=4096, fsm_rounds=True,
                     message_capacity=1 << 16)
    text = _capacity_error(ok, rx, lambda: rx.rx(iq))
    assert "message_slots" in text, text
    rx.close()
    good = ok.Receiver(None, d, max_samples=iq.size // 2, samples_per_buffer=4096, fsm_rounds=True,
                       message_slots=1024, message_capacity=1 << 16)
    got = good.rx(iq)
    _same(good, got, oracle.rx(iq, None, dd.THR, od, 4096), "slots")
    good.close()
    d.close()


# ------------------------------------------------------------------------------------------- error positions ----

@pytest.mark.parametrize("name", ["spb64", "spb97", "spb64x2"])
def test_every_error_position(ok, oracle, name):
    """burst(8) with a pulse too short for `on` at the start of every buffer: one error per buffer, the most the
    reference reports (device.c:646 drops the rest of the buffer).  8192 errors in a default segment of 2^19 samples
    (a segment held 32 positions), 66 000 and 132 000 in the run (the scan held 65 536): ookd_rx_get_errors delivers
    every one, in the scan and in the round form."""
    dev, runs, spb = dd.error_case(name)
    iq = dd.iq_of(runs)
    nbuf = dd.ERROR_STREAMS[name][1]
    legs = ("tables", "walk", "pipelined", "rounds") if name != "spb64x2" else ("tables", "rounds")
    # (segment_buffers 0: the default segment)
    want, seen = _legs(ok, oracle, dev, iq, spb, path=1, legs=legs, segment_buffers=0)
    assert len(want.err_samples) == nbuf and len(want.msg_samples) == 0
    if spb == 64:
        assert nbuf > dd.SCAN_ERRS_BEFORE and seen["rounds"]["num_segments"] >= 8
