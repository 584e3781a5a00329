"""Streams, devices and the oracle-side reference of a shard hand-over (test_gpu_shard_cuts.py; checked on the CPU by
test_shard_cuts_host.py), numpy and the oracle only.

A capture split over several GPUs is decoded shard by shard (ookd_rx_shard_begin / ookd_rx_shard_refine): a
shard hands the next one an ookd_fsm_state, which must be what the sequential state machine holds in front of that
sample.  `carried_states` is that reference: the oracle's machine fed buffer by buffer as device.c does, looked at in
front of every multiple of samples_per_buffer -- every place a shard may end.  The cases below are short streams whose
cuts fall into every phase of a message, behind errors, into stretches in which nothing fires, into spans with many
firings, into long payloads.  Nothing here knows what the kernels compute."""
import ctypes as C
from collections import namedtuple

import numpy as np

from tests import dense_devices as dd
from tests.helpers import edges_of, golden_path, stream_from_runs

# What the machine holds in front of sample `pos` (a multiple of samples_per_buffer):
#   state, num_bits, elapsed_us, prev_bit, payload   ook_sm_peek / ook_sm_data, as they are (in the reset state num_bits
#                                                    and payload are still those of the message before: the machine
#                                                    zeroes them on its next sample)
#   k             sequential additions of the per-sample increment that give elapsed_us
#   last_bit      level of sample pos - 1
#   error_before  the buffer in front of pos held an error (the rest of it was dropped); err_sample: where, else -1
Carried = namedtuple("Carried", "pos state num_bits elapsed_us k prev_bit payload last_bit error_before err_sample")


def elapsed_table(rate, upto):
    """E(0) = 0, E(k) = E(k-1) + (1.0 / rate) * 1e6 in doubles, added one after the other as the machine does
    (state_machine.c:78-82, :514).  (np.cumsum of float64 adds in sequence; test_shard_cuts_host.py replays a stretch
    in a plain loop.)"""
    inc = (1.0 / float(rate)) * 1e6
    return np.concatenate([[0.0], np.cumsum(np.full(int(upto), inc, np.float64))])


def k_of(table, elapsed):
    i = int(np.searchsorted(table, elapsed))
    assert i < table.size and table[i] == elapsed, ("elapsed_us is no sum of increments", elapsed)
    return i


def fsm_of(oracle, dev):
    return dev if isinstance(dev, oracle.FsmDesc) else dd.fsm_desc(oracle, dev)


def carried_states(oracle, dev, stream, spb):
    """One Carried per multiple of spb, from spb up to and including the stream's length (a multiple of spb).  dev: a
    table set of dense_devices or an oracle.FsmDesc."""
    fsm = fsm_of(oracle, dev)
    bits = np.ascontiguousarray(stream, np.uint8)
    assert bits.size and bits.size % spb == 0
    L = oracle.lib()
    cs = fsm.c_struct()
    h = L.ook_sm_new(C.byref(cs))
    # (the reset state evaluates twice per sample: at most two increments each)
    table = elapsed_table(fsm.sample_rate, 2 * bits.size + 2)
    nproc, nb, st = C.c_uint(0), C.c_uint32(0), C.c_uint32(0)
    el, pb = C.c_double(0), C.c_int(0)
    nbytes = fsm.payload_bytes + 1          # (an append at index max_bits is still stored: state_machine.c:365-385)
    out = []
    for base in range(0, bits.size, spb):
        total, r, err = 0, 0, -1
        while total < spb and r != -1:
            r = L.ook_sm_process(h, bits[base + total:].ctypes.data, spb - total, C.byref(nproc))
            total += nproc.value
            if r == -1:
                err = base + total - 1          # device.c:646: the rest of this buffer is never fed in
        L.ook_sm_peek(h, C.byref(st), C.byref(nb), C.byref(el), C.byref(pb))
        d = L.ook_sm_data(h)
        out.append(Carried(base + spb, int(st.value), int(nb.value), float(el.value), k_of(table, el.value),
                           int(pb.value), bytes(d[i] for i in range(nbytes)), int(bits[base + spb - 1]), err >= 0, err))
    L.ook_sm_free(h)
    return out


# ------------------------------------------------------------------------------------- reading a device ----

def quiet_state(fsm):
    """where the reset state goes on its first sample (burst: idle; drip: run)"""
    t = int(fsm.trig_begin[0])
    assert fsm.trig_cond[t] == dd.ALWAYS
    return int(fsm.trig_next[t])


def k_matters(fsm, state):
    """the state, or a trigger of it, has a duration, or it has a time-out that a trigger waits for: elapsed_us is
    looked at in it.  Everywhere else the machine counts on and nothing ever reads the count."""
    t0, t1 = int(fsm.trig_begin[state]), int(fsm.trig_begin[state + 1])
    if fsm.state_duration_us[state] != 0 or any(fsm.trig_duration_us[t] != 0 for t in range(t0, t1)):
        return True
    return fsm.state_timeout_us[state] != 0 and any(fsm.trig_cond[t] == dd.TIMEOUT for t in range(t0, t1))


def carried_class(fsm, c):
    """("reset" | "quiet" | "mid", prev_bit, error_before)"""
    kind = "reset" if c.state == 0 else "quiet" if c.state == quiet_state(fsm) else "mid"
    return kind, c.prev_bit, c.error_before


# ---------------------------------------------------------------------------------------------- streams ----

def padded(stream, spb):
    """low samples behind the stream up to a whole buffer: what a run pads the last buffer with"""
    return np.concatenate([stream, np.zeros(-stream.size % spb, np.uint8)])


def gated_runs(nbits, nmsg, seed, lead=dd.LEAD, gap=(230, 400)):
    """dd.burst_runs behind gated's preamble: [20, 30] in front of every message"""
    rng = np.random.default_rng(seed)
    runs = [lead]
    for _ in range(nmsg):
        runs += [20, 30]
        for b in rng.integers(0, 2, size=nbits):
            runs += [20, 50 if b else 20]
        runs += [20, int(rng.integers(gap[0], gap[1]))]
    return runs


def error_runs(nbits, nmsg, seed):
    """gated_runs with one wrong length in three messages of four: a bit pulse of 7 us, one of 30 us (too short, too
    long for `on`: an error on the falling edge, a LOW sample) or a preamble gap of 42 us (an error on the rising edge
    that ends it, a HIGH sample).  The rest of the error's buffer is dropped and the machine comes back in the middle of
    the message, where the next gap has the wrong length for `gap`: errors in buffers one after the other."""
    rng = np.random.default_rng(seed + 1000)
    runs = gated_runs(nbits, nmsg, seed)
    per = 2 + 2 * nbits + 2
    for m in range(nmsg):
        first = 1 + m * per             # the preamble pulse
        kind = m % 4
        if kind == 1 or kind == 2:
            at = first + 2 + 2 * int(rng.integers(0, nbits))        # a bit pulse
            new = 7 if kind == 1 else 30
            runs[at + 1] += runs[at] - new
            runs[at] = new
        elif kind == 3:
            runs[first + 1] = 42
    return runs


def glitch_runs(glitches, spb, nmsg=3, seed=11):
    """burst(8) messages with `glitches` pulses of 1 us inside one 50 us gap of the second message -- low 25, the pulses
    1 us apart, low again up to 50: 2 * glitches edges on which nothing fires, `off` counts on and the rising edge behind
    them is judged by the whole gap.  The silence in front is stretched so that a multiple of spb falls between the
    first glitch edge and the last (for one pulse: on the last, its falling edge -- one sample behind the first)."""
    runs = dd.burst_runs(8, nmsg, seed=seed)
    per = 2 * 8 + 2
    at = next(i for i in range(1 + per, 1 + 2 * per) if runs[i] == 50 and runs[i - 1] == 20)
    runs[at:at + 1] = [25] + [1, 1] * (glitches - 1) + [1] + [50 - 25 - (2 * glitches - 1)]
    first = sum(runs[:at]) + 25
    target = first + glitches
    runs[0] += -target % spb
    return runs


def glitch_edges(stream):
    """(first, last) sample index among the edges that begin or end a run of one sample"""
    e = edges_of(stream)
    short = np.diff(e) == 1
    idx = np.nonzero(np.concatenate([short, [False]]) | np.concatenate([[False], short]))[0]
    return int(e[idx[0]]), int(e[idx[-1]])


def ticker_high_runs(spb, seed=31):
    """ticker: six high runs of 110 samples (two messages each), and at the stream's end one of 140 -- two buffers of
    64 that are one constant high level -- with the silence in front of it stretched to whole buffers"""
    runs = dd.ticker_runs(2, 6, seed=seed)
    runs[-1] += -(sum(runs) + 140) % spb
    return runs + [140]


def glitchy_p3l_runs(nmsg, seed, us=3):
    """p3l-nexa2012 at 3 Msps: messages (36 bits, pulses of 500 us, gaps of 2000 / 4000) with 1 to 3 short pulses inside
    bit gaps, before any bit window opens: the messages still decode, through the scan's stuck codes"""
    rng = np.random.default_rng(seed)
    runs = [5000]
    for m in range(nmsg):
        runs += [500 * us, 8700 * us]
        bits = rng.integers(0, 2, size=36)
        hit = {int(x) for x in rng.choice(36, size=1 + m % 3, replace=False)}
        for i, bit in enumerate(bits):
            gap = (4000 if bit else 2000) * us
            runs.append(500 * us)
            if i in hit:
                a = int(rng.integers(100, 900))
                g = int(rng.integers(20, 400))
                runs += [a, g, gap - a - g]
            else:
                runs.append(gap)
        runs += [500 * us, int(rng.integers(12000, 40000))]
    return runs


# ------------------------------------------------------------------------------------------------ cases ----
# name -> Case.  tables: a table set of dense_devices, or None for a shipped device (json: its name under
# tests/golden/devices).  scan: what the scan form makes of the WHOLE stream, as the documents say -- "keeps" (fsm_path
# 1), "outside" (the device is beyond the scan's domain: round form, 2), None (not stated: recorded by the GPU test).
# stuck: the stream holds stretches of edges on which nothing fires (glitch pulses inside a bit gap; `stuck_stretches`).
# "held": the table forms hold such a stretch as stuck codes; "deep": it is deeper than they hold, and they refuse a
# shard that holds all of it.  The form that simulates every span (OOKD_RX_SCAN_SIMS) has no stuck codes at all.

Case = namedtuple("Case", "name tables json rate spb stream scan stuck")

P3L, P3L_RATE = "p3l-nexa2012", 3000000


def _drip_head(nbits, samples):
    dev, runs = dd.long_case("drip", nbits)
    return dev, stream_from_runs(runs)[:samples]


def _designed(name, tables, spb, runs, scan, stuck=False):
    return Case(name, tables, None, dd.RATE, spb, padded(stream_from_runs(runs), spb), scan, stuck)


def _build(name):
    if name == "A16":
        return _designed(name, dd.burst(8), 16, dd.burst_runs(8, 3, seed=3), "keeps")
    if name == "A64":
        return _designed(name, dd.burst(8), 64, dd.burst_runs(8, 6, seed=3), "keeps")
    if name == "B":
        # (an error is no refusal: one per span is what a span's record holds)
        return _designed(name, dd.gated(8), 64, error_runs(8, 12, seed=3), "keeps")
    if name in ("C1", "C2", "C7"):
        g = int(name[1:])
        # (seven pulses are what test_gpu_dense_results._refused_burst_capture uses: deeper than the stuck codes hold)
        return _designed(name, dd.burst(8), 16, glitch_runs(g, 16), None, stuck="deep" if g == 7 else "held")
    if name == "D":
        return _designed(name, dd.rle(40), 16, dd.rle_runs(40, 16, 3, seed=41), "keeps")
    if name == "E":
        return _designed(name, dd.ticker(), 64, ticker_high_runs(64), "keeps")
    if name in ("F_drip129", "F_drip188"):
        dev, stream = _drip_head(int(name[6:]), 100 * 64)
        return Case(name, dev, None, dd.RATE, 64, stream, "keeps", False)
    if name == "F_burst254":
        dev, runs = dd.long_case("burst", 254, nmsg=2)
        return _designed(name, dev, 64, runs, "outside")
    if name == "G":
        return Case(name, None, P3L, P3L_RATE, 8192, padded(stream_from_runs(glitchy_p3l_runs(3, seed=5)), 8192), "keeps", "held")
    raise KeyError(name)


CASES = ("A16", "A64", "B", "C1", "C2", "C7", "D", "E", "F_drip129", "F_drip188", "F_burst254", "G")
MULTI_SHARD_CASES = ("A16", "A64", "B", "G")
_cache = {}


def case(name):
    if name not in _cache:
        c = _build(name)
        assert c.stream.size % c.spb == 0
        _cache[name] = c
    return _cache[name]


def oracle_device(oracle, c):
    if c.tables is not None:
        return dd.fsm_desc(oracle, c.tables)
    return oracle.load_device_json(golden_path("devices", c.json), c.rate)[0]


def ok_device(ok, c):
    if c.tables is not None:
        return dd.ok_device(ok, c.tables)
    return ok.Device.load(golden_path("devices", c.json), c.rate)


def stuck_stretches(c):
    """[(first, last)]: sample indices of the first and the last edge of every stretch of edges on which nothing fires --
    cases C: the 1 us pulses of the one bit gap; G: each short pulse inside a bit gap (every real pulse of p3l-nexa2012
    is 1500 samples long), its rising and its falling edge"""
    if not c.stuck:
        return []
    if c.tables is not None:
        return [glitch_edges(c.stream)]
    e = edges_of(c.stream)
    return [(int(a), int(b)) for a, b in zip(e[0::2], e[1::2]) if b - a < 1500]


def holds_any(c, lo, hi):
    """the shard [lo, hi) holds an edge of a stuck stretch"""
    return any(first < hi and last >= lo for first, last in stuck_stretches(c))


def holds_whole(c, lo, hi):
    """... all the edges of one"""
    return any(lo <= first and last < hi for first, last in stuck_stretches(c))


def cuts(c):
    """every place the stream can be cut in two shards"""
    return list(range(c.spb, c.stream.size, c.spb))


_carried = {}


def carried(oracle, c):
    """{pos: Carried} for every cut and the stream's end; computed once per case"""
    if c.name not in _carried:
        _carried[c.name] = {x.pos: x for x in carried_states(oracle, oracle_device(oracle, c), c.stream, c.spb)}
    return _carried[c.name]


def purity_cuts(oracle, c, count=5):
    """`count` cuts spread over the carried classes: the first cut of each class, most different first (mid-message
    and behind an error before the quiet ones), filled up with cuts spread evenly over the stream"""
    fsm = oracle_device(oracle, c)
    held = carried(oracle, c)
    first = {}
    for p in cuts(c):
        first.setdefault(carried_class(fsm, held[p]) + (held[p].state,), p)
    order = sorted(first, key=lambda k: (not k[2], k[0] != "mid", not k[1], k[3]))
    picked = [first[k] for k in order][:count]
    rest = [p for p in cuts(c) if p not in picked]
    while len(picked) < count and rest:
        picked.append(rest.pop(len(rest) * (len(picked) + 1) // (count + 1) % len(rest)))
    return sorted(picked)


def shard_layouts(oracle, c):
    """Bounds of three to five uneven shards, each layout with one shard of a single alignment unit and one empty
    middle shard; the units stand where the machine is in the middle of a message (or behind an error)."""
    fsm = oracle_device(oracle, c)
    held = carried(oracle, c)
    n, spb = c.stream.size, c.spb
    mid = [p for p in cuts(c) if carried_class(fsm, held[p])[0] == "mid" and p + spb < n]
    high = [p for p in mid if held[p].prev_bit == 1] or mid
    err = [p for p in cuts(c) if held[p].error_before and p + spb < n] or mid
    assert len(mid) >= 3
    a, b = mid[len(mid) // 4], mid[3 * len(mid) // 4]
    assert a + spb < b
    e = high[len(high) // 2]
    f = err[len(err) // 2]
    layouts = [[0, a, a + spb, a + spb, b, n],         # 5: long, one unit, empty, long, last
               [0, e, e, e + spb, n],                  # 4: long, empty, one unit, last
               [0, f, f + spb, f + spb, n]]            # 4: the unit behind an error (or mid-message)
    return layouts


# ------------------------------------------------------------------- narrow shards through the front ends ----
# Case A's recipe with twelve messages (buffers of 1000 outputs leave nine places to cut), every sample repeated D times:
# behind a filter of total decimation D the designed device still sees 1 Msps.

FRONT_LEVEL8 = 121              # a high sample as CS8; 16 times that as SC16Q11 (1936 LSB = 0.945)
FRONT_OUTPUTS = 10000           # outputs of the whole capture: whole buffers of 200 and of 1000 outputs
PAD = 8192                      # loud samples on either side of a shard in its own allocation: two tiles of any front end
FRONT_CUTS = 8


def front_bits():
    s = stream_from_runs(dd.burst_runs(8, 12, seed=3))
    assert s.size <= FRONT_OUTPUTS
    return np.concatenate([s, np.zeros(FRONT_OUTPUTS - s.size, np.uint8)])


def front_capture(dec, eight_bit=False):
    """I,Q samples (Q = 0) of front_bits, each repeated `dec` times: int8 values for a CS8 context, or the same capture
    as SC16Q11 (CS8 v is 16 v)"""
    i = np.repeat(front_bits(), dec).astype(np.int16) * FRONT_LEVEL8
    iq = np.zeros(2 * i.size, np.int16)
    iq[0::2] = i
    return iq.astype(np.int8) if eight_bit else iq * 16


def front_threshold(gain):
    """Half of what the filter makes of a high level (its DC gain times 0.945): the slicer cuts the smoothed edges of
    a pulse half way up, so the pulse keeps its width and burst(8) its messages.  (At 0.1 a 32-tap low-pass widens a
    20 us pulse beyond what `on` accepts.)"""
    return round(0.5 * abs(gain) * 16 * FRONT_LEVEL8 / 2048.0, 3)


def loud_pad(eight_bit=False, behind=False):
    """PAD samples at full scale, I in blocks of 37 and Q in blocks of 53 samples of alternating sign -- slow enough to
    pass any low-pass --, the block next to the shard NEGATIVE on I: as a filter's history it pulls a high level down
    and lifts a low one over the threshold, and as the level in front it makes an edge where there is none (or hides
    one)."""
    full = 127 if eight_bit else 2047
    t = np.arange(PAD)
    i = np.where((t // 37) % 2 == 0, -full, full)
    q = np.where((t // 53) % 2 == 0, full, -full)
    if not behind:
        i, q = i[::-1], q[::-1]             # the negative block last: next to the shard's first sample
    out = np.empty(2 * PAD, np.int8 if eight_bit else np.int16)
    out[0::2], out[1::2] = i, q
    return out


def front_cuts(spb, dec, count=FRONT_CUTS):
    """`count` cuts (input samples) spread over the capture: the first and the last possible one, three inside a pulse
    (the shard behind starts high, its filter's history is high) and the rest spread evenly; none leaves the shard in
    front a whole number of 64-bit words"""
    per = spb // dec
    nbuf = FRONT_OUTPUTS // per
    assert spb % dec == 0 and FRONT_OUTPUTS % per == 0
    bits = front_bits()
    cand = [b for b in range(1, nbuf) if (b * per) % 64 != 0]
    assert cand[0] == 1 and cand[-1] == nbuf - 1 and len(cand) >= count
    high = [b for b in cand[1:-1] if bits[b * per - 1] and bits[b * per]]
    picked = {cand[0], cand[-1]} | {high[i * (len(high) - 1) // 2] for i in range(3)}
    rest = [b for b in cand if b not in picked]
    while len(picked) < count:
        picked.add(rest.pop(len(rest) * (count - len(picked)) // (count - len(picked) + 1) % len(rest)))
    return [b * spb for b in sorted(picked)]
