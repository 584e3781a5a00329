"""CPU-side checks of tests/shard_cut_inputs.py (no GPU): every case's cuts fall where test_gpu_shard_cuts.py needs them
-- computed with the oracle alone --, the reference of a hand-over (`carried_states`) is what the oracle's machine
holds, and no cut is left out of the sweep."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from tests import dense_devices as dd
from tests import shard_cut_inputs as sci
from tests.helpers import GOLDEN, edges_of


def _whole(oracle, c):
    return oracle.sm_stream(sci.oracle_device(oracle, c), c.stream, c.spb)


# ------------------------------------------------------------------------------ the reference of a hand-over ----

def test_elapsed_table_is_the_sequence_of_additions():
    """the table behind `k` against a plain loop, at the shipped device's 3 Msps (1/3 us does not add up exactly) and
    at 1 Msps, where the increment is 1.0 and k == elapsed_us"""
    t = sci.elapsed_table(3000000, 5000)
    inc, e = (1.0 / 3000000.0) * 1e6, 0.0
    for k in range(5001):
        assert t[k] == e
        e += inc
    assert t[3] != 1.0 or t[3000] != 1000.0        # (inexact: the replay is needed)
    assert (sci.elapsed_table(dd.RATE, 5000) == np.arange(5001)).all()
    assert sci.k_of(t, t[1234]) == 1234


@pytest.mark.parametrize("name", sci.CASES)
def test_carried_states_restart_the_machine(oracle, name):
    """What `carried_states` shows in front of a cut is all there is to the machine: a fresh one, put into that state
    field by field (through k additions, as the kernels count), decodes the rest of the stream as the whole run does.
    Checked at a dozen cuts spread over each case."""
    c = sci.case(name)
    fsm = sci.oracle_device(oracle, c)
    held = sci.carried(oracle, c)
    ms, pay, es = _whole(oracle, c)
    cuts = sci.cuts(c)
    assert sorted(held) == cuts + [c.stream.size]       # every multiple of spb, the end included
    table = sci.elapsed_table(fsm.sample_rate, max(h.k for h in held.values()) + 1)
    for p in sorted(set(sci.purity_cuts(oracle, c, 6) + cuts[::max(1, len(cuts) // 6)])):
        h = held[p]
        assert h.last_bit == c.stream[p - 1] and table[h.k] == h.elapsed_us
        assert h.error_before == any(p - c.spb <= e < p for e in es)
        if h.error_before:
            assert h.err_sample in es and h.prev_bit == c.stream[h.err_sample] and h.state == 0 and h.k == 0
        else:
            assert h.prev_bit == h.last_bit
        # bits at and above num_bits are zero whenever the machine is not in the reset state
        if h.state != 0:
            have = np.unpackbits(np.frombuffer(h.payload, np.uint8), bitorder="little")
            assert not have[h.num_bits:].any()
        got_m, got_e = _resume(oracle, fsm, c, h, table)
        assert got_m == [(int(m), bytes(q)) for m, q in zip(ms, pay) if m >= p], (name, p)
        assert got_e == [int(e) for e in es if e >= p], (name, p)


def _resume(oracle, fsm, c, h, table):
    """a fresh machine set to the carried state, run over the stream from the cut on, buffer by buffer"""
    L = oracle.lib()
    cs = fsm.c_struct()
    sm = L.ook_sm_new(C.byref(cs))
    st, nb, el, pb = C.c_uint32(9), C.c_uint32(9), C.c_double(9), C.c_int(9)
    L.ook_sm_poke(sm, h.state, h.num_bits, float(table[h.k]), h.prev_bit, h.payload, len(h.payload))
    L.ook_sm_peek(sm, C.byref(st), C.byref(nb), C.byref(el), C.byref(pb))
    assert (st.value, nb.value, el.value, pb.value) == (h.state, h.num_bits, float(table[h.k]), h.prev_bit)
    bits, spb = c.stream, c.spb
    nproc = C.c_uint(0)
    msgs, errs = [], []
    for base in range(h.pos, bits.size, spb):
        total, r = 0, 0
        while total < spb and r != -1:
            r = L.ook_sm_process(sm, bits[base + total:].ctypes.data, spb - total, C.byref(nproc))
            total += nproc.value
            if r == 1:
                d = L.ook_sm_data(sm)
                msgs.append((base + total - 1, bytes(d[i] for i in range(fsm.payload_bytes))))
            elif r == -1:
                errs.append(base + total - 1)
    L.ook_sm_free(sm)
    return msgs, errs


def _wrong(fsm, h):
    """the carried state with one field wrong, per field"""
    out = {"prev_bit": h._replace(prev_bit=1 - h.prev_bit)}
    if sci.k_matters(fsm, h.state):
        out["k+1"] = h._replace(k=h.k + 1)
        if h.k:
            out["k-1"] = h._replace(k=h.k - 1)
    if h.state != 0 and h.num_bits:
        out["num_bits"] = h._replace(num_bits=h.num_bits - 1)
        out["payload"] = h._replace(payload=bytes([h.payload[0] ^ 1]) + h.payload[1:])
    return out


# every field of a hand-over, and a case in which the REST of the capture decodes differently when a shard is begun with
# that field wrong (a count off by one is forgiven by burst's duration windows of +-15 %: ticker's and drip's time-outs
# move a message by a sample).  Where the rest does not show it -- k in the other cases -- the outgoing bytes of the
# shards in front do: test_gpu_shard_cuts.py compares them at every cut, and behind the one-unit shards in between.
SHOWS = [("prev_bit", "A16"), ("prev_bit", "B"), ("k+1", "E"), ("k-1", "E"), ("k-1", "F_drip129"), ("k+1", "F_drip188"),
         ("k-1", "C1"), ("k-1", "C7"), ("num_bits", "A64"), ("num_bits", "F_drip188"), ("num_bits", "G"),
         ("payload", "D"), ("payload", "F_drip129"), ("payload", "G")]


@pytest.mark.parametrize("field,name", SHOWS)
def test_a_wrong_carried_field_shows_in_the_rest_of_the_capture(oracle, field, name):
    c = sci.case(name)
    fsm = sci.oracle_device(oracle, c)
    held = sci.carried(oracle, c)
    ms, pay, es = _whole(oracle, c)
    table = sci.elapsed_table(fsm.sample_rate, max(h.k for h in held.values()) + 2)
    shown = 0
    for p in sci.cuts(c):
        w = _wrong(fsm, held[p]).get(field)
        if w is not None:
            truth = ([(int(m), bytes(q)) for m, q in zip(ms, pay) if m >= p], [int(e) for e in es if e >= p])
            shown += _resume(oracle, fsm, c, w, table) != truth
    assert shown >= 1, (field, name)


# ------------------------------------------------------------------------ the inputs hold what they are for ----

@pytest.mark.parametrize("name", sci.CASES)
def test_every_case_has_messages_and_all_its_cuts(oracle, name):
    c = sci.case(name)
    ms, pay, es = _whole(oracle, c)
    assert len(ms) >= 2
    n = c.stream.size
    assert sci.cuts(c) == [p for p in range(1, n) if p % c.spb == 0] and len(sci.cuts(c)) >= 8
    assert n % c.spb == 0 and (n <= 30000 or name == "G")
    # the whole-capture run of the oracle is the same machine (it is what the GPU test compares with)
    want = oracle.rx(dd.iq_of(c.stream), None, dd.THR, sci.oracle_device(oracle, c), c.spb, want_bits=True)
    assert list(want.msg_samples) == list(ms) and list(want.err_samples) == list(es)
    assert (want.bits == c.stream).all()
    # ... and so does the reference's own state_machine.c: its committed record (`gated`, the glitch streams and the
    # error streams of case B are in no other), and the live reference where it is built
    with open(os.path.join(GOLDEN, "shard_cuts_ref_recorded.json")) as f:
        rec = json.load(f)[name]
    got = ([int(x) for x in ms], [bytes(p).hex() for p in pay], [int(x) for x in es])
    assert (rec["samples"], rec["spb"]) == (n, c.spb), "the record is of another stream: regenerate it"
    assert got == (rec["msg_samples"], rec["payloads"], rec["err_samples"])
    if oracle.have_ref():
        rm, rp, re_ = oracle.RefSm(sci.oracle_device(oracle, c)).stream(c.stream, c.spb)
        assert list(rm) == list(ms) and (rp == pay).all() and list(re_) == list(es)
    # the cuts of the purity check and the bounds of the several-shards check are cuts of the sweep
    assert set(sci.purity_cuts(oracle, c)) <= set(sci.cuts(c)) and len(set(sci.purity_cuts(oracle, c))) == 5
    if name in sci.MULTI_SHARD_CASES:
        for b in sci.shard_layouts(oracle, c):
            assert 3 <= len(b) - 1 <= 5 and b[0] == 0 and b[-1] == n and b == sorted(b)
            assert all(x % c.spb == 0 for x in b)
            sizes = [hi - lo for lo, hi in zip(b, b[1:])]
            assert c.spb in sizes[:-1] and 0 in sizes[1:-1] and len(set(sizes)) >= 3


@pytest.mark.parametrize("name", ["A16", "A64"])
def test_a_every_phase_of_a_message(oracle, name):
    c = sci.case(name)
    fsm = sci.oracle_device(oracle, c)
    held = [sci.carried(oracle, c)[p] for p in sci.cuts(c)]
    assert {h.state for h in held} >= set(range(1, fsm.num_states))
    assert sum(h.prev_bit for h in held) >= 5
    names = c.tables["state_names"]
    # prev_bit 1 in `on` (a pulse cut in two: the shard behind starts high) and in idle (the last pulse of a message
    # goes on behind its output)
    assert any(names[h.state] == "on" and h.prev_bit for h in held)
    if c.spb == 16:
        assert any(names[h.state] == "idle" and h.prev_bit for h in held)
        # shorter than a pulse: cuts inside pulses and inside both bit gaps (a gap of 20 and one of 50 us)
        off = [h for h in held if names[h.state] == "off"]
        assert any(h.k < 20 for h in off) and any(h.k > 25 for h in off) and all(h.prev_bit == 0 for h in off)


def test_b_errors_at_both_levels_on_both_sides_of_a_cut(oracle):
    c = sci.case("B")
    held = [sci.carried(oracle, c)[p] for p in sci.cuts(c)]
    behind = [h for h in held if h.error_before]
    combos = {(int(c.stream[h.err_sample]), h.last_bit) for h in behind}
    assert combos == {(0, 0), (0, 1), (1, 0), (1, 1)}, combos
    # prev_bit is the level of the error sample, whatever the buffer ends with
    assert all(h.prev_bit == c.stream[h.err_sample] and h.state == 0 for h in behind)
    errs = sorted({h.err_sample // c.spb for h in behind})
    assert any(b >= 1 for b in errs)                    # an error in the buffer BEHIND a cut (the first of a shard)
    assert any(b + 1 in errs for b in errs if b >= 1)   # errors in consecutive buffers: on both sides of a cut
    assert len(errs) >= 6
    ms, _, _ = _whole(oracle, c)
    assert len(ms) >= 2                                 # and messages come through all the same


@pytest.mark.parametrize("glitches", [1, 2, 7])
def test_c_a_cut_between_the_glitch_edges(oracle, glitches):
    """a cut c with first glitch edge < c <= last glitch edge: the shard in front holds the first edge on which nothing
    fires, the shard behind the last.  (One pulse of one sample has its two edges on neighbouring samples: the cut is
    its falling edge; from two pulses on a cut lies strictly between the first edge and the last.)"""
    c = sci.case("C%d" % glitches)
    first, last = sci.glitch_edges(c.stream)
    assert last - first == 2 * glitches - 1
    inside = [p for p in sci.cuts(c) if first < p <= last]
    assert inside and (glitches == 1 or any(p < last for p in inside))
    held = sci.carried(oracle, c)
    names = c.tables["state_names"]
    for p in inside:
        # nothing has fired since the falling edge in front of the gap (sample first - 25, on which `on` fired and
        # the count began anew): the carried count is what matters
        assert names[held[p].state] == "off" and held[p].k == p - 1 - (first - 25) and held[p].k != 0
    ms, _, es = _whole(oracle, c)
    assert len(ms) == 3 and len(es) == 0                # the glitches do not break the message


def test_d_a_cut_in_the_middle_of_a_period(oracle):
    c = sci.case("D")
    held = [sci.carried(oracle, c)[p] for p in sci.cuts(c)]
    assert any(h.k % dd.RLE_PERIOD != 0 and h.num_bits >= 1 and h.state != 0 for h in held)
    # a span with many firings cut in two: appends of one low run on both sides of a cut
    stats = dd.leaf_stats(oracle, c.tables, c.stream, c.spb)[0]
    assert stats.max() == 16
    e = edges_of(c.stream)
    leaf = int(np.argmax(stats))
    inside = [p for p in sci.cuts(c) if e[leaf - 1] < p < e[leaf]]
    assert len(inside) >= 8
    nb = [sci.carried(oracle, c)[p].num_bits for p in inside]
    assert nb == sorted(nb) and nb[-1] - nb[0] >= 8


def test_e_messages_on_both_sides_of_a_cut(oracle):
    c = sci.case("E")
    ms, _, _ = _whole(oracle, c)
    ms = np.asarray(ms, np.int64)
    both = [p for p in sci.cuts(c) if ((ms >= p - 2 * c.spb) & (ms < p)).any() and ((ms >= p) & (ms < p + 2 * c.spb)).any()]
    assert both
    # ... of ONE span: a cut inside a high run with an output in front of it and one behind
    e = edges_of(c.stream)
    assert any(((ms >= e[i]) & (ms < p)).any() and ((ms >= p) & (ms < e[i + 1])).any()
               for i in range(0, len(e) - 1, 2) for p in sci.cuts(c) if e[i] < p < e[i + 1])
    # shards that are one constant high level: the last two buffers
    n = c.stream.size
    assert c.stream[n - 2 * c.spb - 1:].all() and not c.stream[n - 141]


@pytest.mark.parametrize("name,levels", [("F_drip129", (65,)), ("F_drip188", (65, 129)), ("F_burst254", (65, 129, 193))])
def test_f_every_payload_word_is_carried(oracle, name, levels):
    c = sci.case(name)
    held = [sci.carried(oracle, c)[p] for p in sci.cuts(c)]
    nb = [h.num_bits for h in held if h.state != 0]
    for lv in levels:
        assert max(nb) >= lv
    # all fill levels: no stretch of 64 bits without a cut in it
    assert all(any(lo <= x < lo + 64 for x in nb) for lo in range(0, max(nb) - 63, 32))
    words = np.zeros((len(held), 40), np.uint8)
    for i, h in enumerate(held):
        words[i, :len(h.payload)] = np.frombuffer(h.payload, np.uint8)
    assert list((words.view(np.uint64) != 0).any(axis=0))[:(max(nb) + 63) // 64] == [True] * ((max(nb) + 63) // 64)
    assert dd.scan_domain(c.tables) <= dd.SCAN_DOMAIN_MAX or c.scan == "outside"


def test_g_a_shipped_device_is_cut_inside_its_messages(oracle):
    c = sci.case("G")
    fsm = sci.oracle_device(oracle, c)
    held = [sci.carried(oracle, c)[p] for p in sci.cuts(c)]
    assert any(h.state != 0 for h in held)
    mid = [h for h in held if sci.carried_class(fsm, h)[0] == "mid"]
    assert len(mid) >= 20 and any(h.num_bits >= 30 for h in mid) and any(h.prev_bit for h in mid)
    # k counts thirds of a microsecond: elapsed_us is no whole number at most cuts
    assert any(sci.k_matters(fsm, h.state) and h.k and h.elapsed_us != round(h.elapsed_us) for h in mid)
    ms, _, es = _whole(oracle, c)
    assert len(ms) == 3 and len(es) == 0


# ------------------------------------------------------------------- narrow shards through the front ends ----

@pytest.mark.parametrize("spb,dec", [(200, 1), (1000, 1), (800, 4)])
def test_front_cuts_end_inside_words_and_tiles(spb, dec):
    cuts = sci.front_cuts(spb, dec)
    n_in = sci.FRONT_OUTPUTS * dec
    assert len(cuts) == 8 and cuts[0] == spb and cuts[-1] == n_in - spb and cuts == sorted(set(cuts))
    for c in cuts:
        assert c % spb == 0 and c % dec == 0
        assert (c // dec) % 64 != 0 and (c // dec) % 1024 != 0      # the shard in front ends inside a word, inside a tile
    # cuts at both levels, inside pulses and inside gaps
    bits = sci.front_bits()
    inside = [c for c in cuts if bits[c // dec - 1] and bits[c // dec]]
    assert len(inside) >= 2 and len(cuts) - len(inside) >= 3


@pytest.mark.parametrize("name,spb", [(None, 200), ("fs32_fs4", 1000), ("unity16", 1000), ("fs128_fs16_dec4", 800)])
def test_front_capture_decodes_behind_every_filter(oracle, name, spb):
    """the threshold of the filtered legs -- half the filtered level of a pulse -- keeps all twelve messages"""
    from tests.helpers import golden_path
    of = oracle.load_filter_json(golden_path("filters", name)) if name else None
    dec = of.total_decimation if of else 1
    gain = float(np.prod([of.stage_taps(s).astype(np.float64).sum() for s in range(of.num_stages)])) if of else 1.0
    iq = sci.front_capture(dec)
    assert (iq[0::2] == sci.front_capture(dec, eight_bit=True)[0::2].astype(np.int16) * 16).all()
    od = dd.fsm_desc(oracle, dd.burst(8))
    want = oracle.rx(iq, of, sci.front_threshold(gain), od, spb, want_bits=True)
    assert len(want.msg_samples) == 12 and len(want.err_samples) == 0
    assert want.decimated == sci.FRONT_OUTPUTS
    # the pads are loud enough, and slow enough, to show: as history in front of the capture they change its first bits
    pad = sci.loud_pad()
    assert pad.size == 2 * sci.PAD and pad[-2] == -2047 and sci.loud_pad(behind=True)[0] == -2047
    if of is not None:
        glued = oracle.rx(np.concatenate([pad, iq]), of, sci.front_threshold(gain), None, spb * (sci.PAD // spb + 1),
                          want_bits=True)
        assert (glued.bits[sci.PAD // dec:sci.PAD // dec + 8] != want.bits[:8]).any()


@pytest.mark.parametrize("name", [n for n in sci.CASES if sci.case(n).stuck])
def test_nothing_fires_on_the_edges_of_a_stuck_stretch(oracle, name):
    """the stretches the GPU test's fsm_path conditions go by: from the sample in front of the first edge to the last
    edge the machine stays in its state and its count runs on, one increment per sample"""
    c = sci.case(name)
    fsm = sci.oracle_device(oracle, c)
    stretches = sci.stuck_stretches(c)
    assert len(stretches) == {"C1": 1, "C2": 1, "C7": 1, "G": 6}[name]
    L = oracle.lib()
    cs = fsm.c_struct()
    sm = L.ook_sm_new(C.byref(cs))
    table = sci.elapsed_table(fsm.sample_rate, 2 * c.stream.size + 2)
    nproc, nb, st, el, pb = C.c_uint(0), C.c_uint32(0), C.c_uint32(0), C.c_double(0), C.c_int(0)
    pos = 0

    def run_to(end):
        nonlocal pos
        while pos < end:
            assert L.ook_sm_process(sm, c.stream[pos:].ctypes.data, end - pos, C.byref(nproc)) != -1
            pos += nproc.value
        L.ook_sm_peek(sm, C.byref(st), C.byref(nb), C.byref(el), C.byref(pb))
        return st.value, nb.value, sci.k_of(table, el.value)

    for first, last in stretches:
        s0, n0, k0 = run_to(first)
        s1, n1, k1 = run_to(last + 1)
        assert (s1, n1, k1) == (s0, n0, k0 + last + 1 - first) and sci.k_matters(fsm, s0), (name, first, last)
        assert sci.holds_whole(c, first, last + 1) and not sci.holds_any(c, last + 1, last + 2)
    L.ook_sm_free(sm)
