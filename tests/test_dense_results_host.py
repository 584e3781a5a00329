"""CPU-side checks of the designed devices of tests/dense_devices.py (no GPU): the streams hold what
test_gpu_dense_results.py needs them to hold -- computed from the oracle's result and the edge list --, the oracle decodes
them as the reference's own state machine does (a committed record, and the live reference where it is built), and the
scan's host-built tables accept every device."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from tests import dense_devices as dd
from tests.helpers import GOLDEN, edges_of, stream_from_runs

import ookiedokie_amd as ok
from ookiedokie_amd import build as okbuild


@pytest.fixture(scope="module", autouse=True)
def built_lib():
    okbuild.build()
    return ok.lib()


def _words_set(payloads):
    """per 64-bit payload word: does any message of the stream have a bit in it"""
    w = np.zeros((len(payloads), 32), np.uint8)
    w[:, :payloads.shape[1]] = payloads
    return [bool(x) for x in (w.view(np.uint64) != 0).any(axis=0)]


# ------------------------------------------------------------------------ the inputs hold what they are for ----

@pytest.mark.parametrize("z", dd.COMPACT_Z + dd.LIMIT_Z)
def test_rle_streams_append_z_bits_in_one_span(oracle, z):
    dev, runs = dd.rle_case(z)
    stream = stream_from_runs(runs)
    napp, nout, nerr = dd.leaf_stats(oracle, dev, stream, 4096)
    assert napp.max() == z and (napp == z).sum() >= 20 and nout.max() == 1 and nerr.sum() == 0
    # short captures: the appends stay within the capture's pool
    assert napp.sum() < 2 * (len(edges_of(stream)) + 1) + dd.POOL_EXTRA
    ms, pay, es = oracle.sm_stream(dd.fsm_desc(oracle, dev), stream, 4096)
    assert len(ms) == 20 and len(es) == 0


@pytest.mark.parametrize("outputs", dd.TICKER_OUTPUTS)
def test_ticker_streams_put_out_k_messages_in_one_span(oracle, outputs):
    dev, runs = dd.ticker_case(outputs)
    stream = stream_from_runs(runs)
    napp, nout, nerr = dd.leaf_stats(oracle, dev, stream, 4096)
    high = nout[1::2]                   # leaf 1, 3, ...: the high runs (leaf 0 ends with the first rising edge)
    assert (high[:100] == outputs).all() and nout[0::2].sum() == 0 and nerr.sum() == 0
    assert napp.max() < dd.COMPACT_APPS
    want = oracle.rx(dd.iq_of(runs), None, dd.THR, dd.fsm_desc(oracle, dev), 4096)
    assert len(want.msg_samples) == 100 * outputs
    # by the edge list alone: every message lies inside a high run, `outputs` of them per run
    e = edges_of(stream)
    idx = np.searchsorted(e, want.msg_samples, side="right") - 1
    assert (idx % 2 == 0).all() and (np.bincount(idx // 2) == outputs).all()


@pytest.mark.parametrize("fires", dd.PACER_FIRES)
def test_pacer_streams_fire_without_leaving_anything(oracle, fires):
    """the firings of a span are not in the oracle's result: by construction a high run of 11 f + 5 samples holds f
    time-outs of 10 us (one every eleven samples, the first eleven behind the rising edge), checked on the state
    machine's own counter: in front of the run's last sample it has counted 4 samples since the f-th"""
    dev, runs = dd.pacer_case(fires)
    stream = stream_from_runs(runs)
    napp, nout, nerr = dd.leaf_stats(oracle, dev, stream, 4096)
    assert napp.sum() == 0 and nout.sum() == 0 and nerr.sum() == 0
    e = edges_of(stream)
    assert (np.diff(e)[0::2] == dd.RLE_PERIOD * fires + 5).all()
    fsm = dd.fsm_desc(oracle, dev)
    L = oracle.lib()
    cs = fsm.c_struct()
    h = L.ook_sm_new(C.byref(cs))
    nproc, st, nb, el, pb = C.c_uint(0), C.c_uint32(0), C.c_uint32(0), C.c_double(0), C.c_int(0)
    L.ook_sm_process(h, stream.ctypes.data, int(e[1]), C.byref(nproc))
    L.ook_sm_peek(h, C.byref(st), C.byref(nb), C.byref(el), C.byref(pb))
    L.ook_sm_free(h)
    assert st.value == 2 and el.value == 4.0


@pytest.mark.parametrize("nbits", dd.BURST_BITS)
@pytest.mark.parametrize("spb", [4096, 1000])
def test_burst_streams_cross_the_block_and_the_pinned_head(oracle, nbits, spb):
    dev, runs = dd.burst_case(nbits)
    stream = stream_from_runs(runs)
    ms, pay, es = oracle.sm_stream(dd.fsm_desc(oracle, dev), stream, spb)
    assert len(ms) == dd.BURST_MESSAGES > dd.HOST_MSG_FIRST and len(es) == 0
    e = edges_of(stream)
    per = 2 * nbits + 2                                   # edges of one message
    assert e.size == per * dd.BURST_MESSAGES
    first = np.arange(dd.BURST_MESSAGES) * per           # leaf that ends with a message's first edge
    out_leaf = np.searchsorted(e, ms, side="left")       # leaf its output falls into
    assert (out_leaf - first == per - 1).all()
    # a message that starts in one finish block and ends in the next, one that starts with a block, one that ends one
    blk0, blk1 = first // dd.FIN_BLOCK, out_leaf // dd.FIN_BLOCK
    assert len(set(blk0)) >= 3
    if nbits != 1:              # (4 edges a message: none crosses a block of 1024)
        assert (blk0 != blk1).any()
    if nbits != 8:              # (18 edges a message: 1024 is no multiple)
        assert (first % dd.FIN_BLOCK == 0).sum() >= 2
    # message 2047 and message 2048 -- the pinned head's last, the device tail's first -- in different chunks
    chunk = 4 * 4096
    assert ms[dd.HOST_MSG_FIRST - 1] // chunk + 1 == ms[dd.HOST_MSG_FIRST] // chunk
    # payloads are not all alike
    assert len({bytes(p) for p in pay}) >= (2 if nbits == 1 else 200)


@pytest.mark.parametrize("extra", [0, 1])
def test_pool_streams_sit_on_the_limit(oracle, extra):
    dev, runs = dd.pool_case(extra)
    stream = stream_from_runs(runs)
    napp, nout, nerr = dd.leaf_stats(oracle, dev, stream, 4096)
    limit = 2 * (len(edges_of(stream)) + 1) + dd.POOL_EXTRA
    assert napp.sum() == limit + extra and napp.max() <= dd.MAX_LEAF_APPS and nout.max() == 1 and nerr.sum() == 0


@pytest.mark.parametrize("kind,nbits", [(k, n) for n in dd.LONG_BITS for k in ("rle", "burst")]
                         + [("drip", n) for n in dd.DRIP_BITS])
def test_long_payload_streams_set_bits_in_every_word(oracle, kind, nbits):
    dev, runs = dd.long_case(kind, nbits)
    stream = stream_from_runs(runs)
    ms, pay, es = oracle.sm_stream(dd.fsm_desc(oracle, dev), stream, 4096)
    assert len(ms) >= 12 and len(es) == 0
    words = (nbits + 63) // 64
    assert _words_set(pay) == [True] * words + [False] * (4 - words)
    napp, nout, nerr = dd.leaf_stats(oracle, dev, stream, 4096)
    assert napp.max() <= dd.MAX_LEAF_APPS and napp.sum() < 2 * (len(edges_of(stream)) + 1) + dd.POOL_EXTRA
    # moved by `boundary_shift`, a multiple of 4096 (where a chunk or a shard ends) lies inside a message with all
    # its bits but one collected: every word of the carried payload is in use
    moved = dd.moved_to_boundary(oracle, dev, stream, nbits - 1, 4096)
    assert dd.leaf_stats(oracle, dev, moved, 1024)[0].max() <= dd.MAX_LEAF_APPS
    cuts = np.arange(4096, moved.size, 4096)
    got = [nb for _, nb in dd.collected_at(oracle, dev, moved, 4096, cuts)]
    assert max(got) >= nbits - 1 >= 64 * (words - 1), got
    assert (dd.scan_domain(dev) <= dd.SCAN_DOMAIN_MAX) == (kind == "drip" or nbits <= 93)


@pytest.mark.parametrize("name", sorted(dd.ERROR_STREAMS))
def test_error_streams_overflow_the_old_lists(oracle, name):
    dev, runs, spb = dd.error_case(name)
    stream = stream_from_runs(runs)
    ms, pay, es = oracle.sm_stream(dd.fsm_desc(oracle, dev), stream, spb)
    nbuf = dd.ERROR_STREAMS[name][1]
    # one error per buffer (device.c:646 drops the rest), on the pulse's falling edge
    assert len(ms) == 0 and list(es) == list(np.arange(nbuf) * spb + 8)
    per_segment = np.bincount((es // dd.SEGMENT).astype(np.int64))
    assert per_segment.max() > dd.ERR_SLOTS_BEFORE
    if spb == 64:
        assert len(es) > dd.SCAN_ERRS_BEFORE


# --------------------------------------------------------------------- semantics pinned to the reference ----

def _recorded():
    with open(os.path.join(GOLDEN, "dense_ref_recorded.json")) as f:
        return json.load(f)


def test_oracle_decodes_the_designed_streams_as_the_reference_does(oracle):
    rec = _recorded()
    seen = 0
    for name, dev, runs in dd.recorded_cases():
        stream = stream_from_runs(runs)
        fsm = dd.fsm_desc(oracle, dev)
        for buf in (97, 4096):
            want = rec["%s/%d" % (name, buf)]
            assert want["samples"] == stream.size, name
            ms, pay, es = oracle.sm_stream(fsm, stream, buf)
            got = ([int(x) for x in ms], [bytes(p).hex() for p in pay], [int(x) for x in es])
            assert got == (want["msg_samples"], want["payloads"], want["err_samples"]), (name, buf)
            if oracle.have_ref():
                rm, rp, re_ = oracle.RefSm(fsm).stream(stream, buf)
                live = ([int(x) for x in rm], [bytes(p).hex() for p in rp], [int(x) for x in re_])
                assert live == got, (name, buf)
            # ... and the whole rx path of the oracle (unpack, threshold, buffers) on the same stream as I,Q
            # (which pads the last buffer with zeros, as the file backend does: drip goes on appending in there)
            full = oracle.rx(dd.iq_of(stream), None, dd.THR, fsm, buf)
            keep = full.msg_samples < stream.size
            assert (list(full.msg_samples[keep]), list(full.err_samples)) == (got[0], got[2]), (name, buf)
            assert [bytes(p).hex() for p in full.payloads[keep]] == got[1]
            seen += 1
    assert seen == len(rec)
    # the record is of everything: messages and errors are in it, and every payload word
    assert sum(len(v["msg_samples"]) for v in rec.values()) > 1500
    assert sum(len(v["err_samples"]) for v in rec.values()) >= 300
    assert max(len(v["msg_samples"]) for v in rec.values()) <= 200


@pytest.mark.parametrize("case", ["burst8", "rle30", "ticker4", "errors64"])
def test_full_streams_through_both_oracle_paths(oracle, case):
    """the streams the GPU tests run, whole: the oracle's state machine alone and its whole rx path agree -- and, where
    oracle/_ref is built, so does the reference's own state_machine.c"""
    if case == "errors64":
        dev, runs, spb = dd.error_case("spb64")
    else:
        dev, runs = {"burst8": lambda: dd.burst_case(8), "rle30": lambda: dd.rle_case(30),
                     "ticker4": lambda: dd.ticker_case(4)}[case]()
        spb = 1000
    stream = stream_from_runs(runs)
    fsm = dd.fsm_desc(oracle, dev)
    ms, pay, es = oracle.sm_stream(fsm, stream, spb)
    full = oracle.rx(dd.iq_of(stream), None, dd.THR, fsm, spb, msg_cap=1 << 17)
    assert list(full.msg_samples) == list(ms) and (full.payloads == pay).all() and list(full.err_samples) == list(es)
    assert len(ms) + len(es) >= 20
    if oracle.have_ref():
        rm, rp, re_ = oracle.RefSm(fsm).stream(stream, spb, cap=1 << 17)
        assert list(rm) == list(ms) and (rp == pay).all() and list(re_) == list(es)


# --------------------------------------------------------------- the scan's host tables accept the devices ----

def _domain_info(dev, spb):
    d = dd.ok_device(ok, dev)
    out = (C.c_uint32 * 8)()
    assert ok.lib().ookd_scan_domain_info(d._h, spb, 1, out) == 0
    d.close()
    return list(out)


# device -> (table intervals, intervals that need a simulation) at 4096 and at 97 samples per buffer, as the span
# tables came out when these tests were written (test_host.py records 74 and 0 for the shipped devices)
_SCAN_TABLES = {
    "burst1": ((46, 0), (46, 0)), "burst8": ((46, 0), (46, 0)), "burst9": ((46, 0), (46, 0)),
    "burst93": ((46, 0), (46, 0)), "rle40": ((184, 0), (184, 0)), "rle93": ((184, 0), (184, 0)),
    "ticker": ((77, 0), (77, 0)), "pacer": ((215, 0), (215, 0)), "drip129": ((261, 0), (261, 0)),
    "drip188": ((261, 0), (261, 0)),
}


@pytest.mark.parametrize("name", sorted(_SCAN_TABLES))
def test_scan_tables_build_for_the_designed_devices(name):
    dev = {"burst1": lambda: dd.burst(1), "burst8": lambda: dd.burst(8), "burst9": lambda: dd.burst(9),
           "burst93": lambda: dd.burst(93), "rle40": lambda: dd.rle(40), "rle93": lambda: dd.rle(93),
           "ticker": dd.ticker, "pacer": dd.pacer, "drip129": lambda: dd.drip(129), "drip188": lambda: dd.drip(188)}[name]()
    for spb, (want_intervals, want_sims) in zip((4096, 97), _SCAN_TABLES[name]):
        built, intervals, need_sim, reach, nstuck, stuck_rows, domain, states = _domain_info(dev, spb)
        assert built == 1, (name, spb)
        assert (intervals, need_sim) == (want_intervals, want_sims), (name, spb)
        assert states == len(dev["state_names"])
        assert domain >= dd.scan_domain(dev) and dd.scan_domain(dev) <= dd.SCAN_DOMAIN_MAX
