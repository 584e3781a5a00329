"""Designed devices and streams for the result stage of the state machine (test_gpu_dense_results.py; checked on the
CPU by test_dense_results_host.py), numpy only.  The shipped devices append at most one bit per span, hold 32 or 36
bits and send a message every 70 ms; these five small machines put as many appends, outputs, firings, messages, payload
bits and errors into a span, a finish block, a capture as the scan's records and lists are built to hold -- and one more.

All run at 1 000 000 samples per second (one sample per microsecond) with no filter and threshold 0.1.  A device is the
table set ok.Device.from_tables and oracle.FsmDesc take; a stream is a list of run lengths for helpers.stream_from_runs
(low first).  Nothing here knows what the kernels compute: `leaf_stats` restates a leaf of the scan from its definition
(leaf i holds the samples behind edge i-1 up to and including edge i) and runs the oracle over it."""
import ctypes as C

import numpy as np

from tests.helpers import edges_of, stream_from_runs

RATE = 1000000
THR = 0.1
AMP = 1945
ALWAYS, PULSE_START, PULSE_END, TIMEOUT, MSG_COMPLETE = 1, 2, 3, 4, 5
NONE, APPEND_0, APPEND_1, OUTPUT = 1, 2, 3, 4

# the scan's limits these inputs are laid against (fsm_scan.hip, rx.cpp; DESIGN 4.6 "limits of a span's record")
COMPACT_APPS = 8            # appends the one-word leaf record holds
MAX_LEAF_APPS = 30          # kMaxLeafApps
MAX_LEAF_OUTPUTS = 2
MAX_FIRES = 48              # kMaxFires
FIN_BLOCK = 1024            # leaves per finish block
HOST_MSG_FIRST = 2048       # kHostMsgFirst
POOL_EXTRA = 512            # a capture's append pool: 2 * (edges + 1) + 512
FB_POOL = 8                 # kFbPool
SEGMENT = 1 << 19           # default segment of the round form
ERR_SLOTS_BEFORE = 32       # error positions a segment held before its list was sized by the buffers
SCAN_ERRS_BEFORE = 1 << 16  # ... and a run of the scan
SCAN_DOMAIN_MAX = 384       # states * (max_bits + 2) + 3 above this: the device runs in the round form


# --------------------------------------------------------------------------------------------------- devices ----

def _tables(name, max_bits, states):
    """states: [(name, duration_us, timeout_us, [(condition, action, next state name, trigger duration_us)])]; the
    first is the reset state"""
    names = [s[0] for s in states]
    tbeg, cond, act, nxt, tdur = [0], [], [], [], []
    for _, _, _, trigs in states:
        for c, a, to, d in trigs:
            cond.append(c)
            act.append(a)
            nxt.append(names.index(to))
            tdur.append(d)
        tbeg.append(len(cond))
    return dict(name=name, state_names=names, max_bits=int(max_bits), sample_rate=RATE,
                state_duration_us=np.array([s[1] for s in states], np.uint64),
                state_timeout_us=np.array([s[2] for s in states], np.uint64),
                trig_begin=np.array(tbeg, np.uint32), trig_cond=np.array(cond, np.uint8),
                trig_action=np.array(act, np.uint8), trig_next=np.array(nxt, np.uint32),
                trig_duration_us=np.array(tdur, np.uint64))


_RESET = ("reset", 0, 0, [(ALWAYS, NONE, "idle", 0)])
_IDLE = ("idle", 0, 0, [(PULSE_START, NONE, "on", 0)])
_ON = ("on", 20, 60, [(MSG_COMPLETE, OUTPUT, "reset", 0), (PULSE_END, NONE, "off", 0), (TIMEOUT, NONE, "reset", 0)])


def burst(nbits):
    """one bit per pulse pair: a 20 us pulse, then 50 us low for a 1 or 20 us low for a 0; a message is nbits + 1 pulses"""
    off = ("off", 0, 200, [(PULSE_START, APPEND_1, "on", 50), (PULSE_START, APPEND_0, "on", 20), (TIMEOUT, NONE, "reset", 0)])
    return _tables("burst%d" % nbits, nbits, [_RESET, _IDLE, _ON, off])


def rle(nbits, timeout_us=10):
    """zeros by time-out: while the level is low `off` appends a 0 every time its time-out runs out, the next pulse
    appends a 1 -- a low run appends many bits inside ONE span"""
    off = ("off", 0, timeout_us, [(PULSE_START, APPEND_1, "on", 0), (TIMEOUT, APPEND_0, "off", 0)])
    return _tables("rle%d" % nbits, nbits, [_RESET, _IDLE, _ON, off])


def ticker(timeout_us=50):
    """a one-bit message every time-out while the level is high: several outputs inside ONE span"""
    return _tables("ticker", 1, [
        _RESET,
        ("idle", 0, 0, [(PULSE_START, APPEND_1, "tick", 0)]),
        ("tick", 0, timeout_us, [(PULSE_END, NONE, "reset", 0), (TIMEOUT, OUTPUT, "reset2", 0)]),
        ("reset2", 0, 0, [(ALWAYS, APPEND_1, "tick", 0)])])


def pacer(timeout_us=10):
    """ticker without its messages: while the level is high `pace` fires its time-out and stays -- many firings inside
    ONE span that leave no append and no output behind (the firing limit cannot be met with rle, whose every firing
    appends, nor with ticker, whose every second firing is an output)"""
    return _tables("pacer", 1, [
        _RESET,
        ("idle", 0, 0, [(PULSE_START, NONE, "pace", 0)]),
        ("pace", 0, timeout_us, [(PULSE_END, NONE, "reset", 0), (TIMEOUT, NONE, "pace", 0)])])


def drip(nbits, timeout_us=10):
    """rle in TWO states, so that payloads beyond 93 bits stay within the scan's domain (SCAN_DOMAIN_MAX; burst and rle
    have four states): `run` appends a 1 on every rising edge and a 0 whenever 10 us pass without an edge, and puts a
    message out every nbits appends, back to back"""
    return _tables("drip%d" % nbits, nbits, [
        ("reset", 0, 0, [(ALWAYS, NONE, "run", 0)]),
        ("run", 0, timeout_us, [(MSG_COMPLETE, OUTPUT, "reset", 0), (PULSE_START, APPEND_1, "run", 0),
                                (PULSE_END, NONE, "run", 0), (TIMEOUT, APPEND_0, "run", 0)])])


def gated(nbits):
    """burst behind a preamble: a 20 us pulse and a gap of 30 us in front of every message.  `gap` has a DURATION, so a
    rising edge that ends a gap of another length is an error -- on a HIGH sample; burst's only error, a pulse of the
    wrong length in `on`, falls on a low one.  (tests/shard_cut_inputs.py: the level behind an error at a shard's end)"""
    sync = ("sync", 20, 60, [(PULSE_END, NONE, "gap", 0), (TIMEOUT, NONE, "reset", 0)])
    gap = ("gap", 30, 200, [(PULSE_START, NONE, "on", 0), (TIMEOUT, NONE, "reset", 0)])
    off = ("off", 0, 200, [(PULSE_START, APPEND_1, "on", 50), (PULSE_START, APPEND_0, "on", 20), (TIMEOUT, NONE, "reset", 0)])
    return _tables("gated%d" % nbits, nbits, [_RESET, ("idle", 0, 0, [(PULSE_START, NONE, "sync", 0)]), sync, gap, _ON, off])


_TABLE_KEYS = ("state_duration_us", "state_timeout_us", "trig_begin", "trig_cond", "trig_action", "trig_next",
               "trig_duration_us")


def fsm_desc(oracle, dev):
    return oracle.FsmDesc(state_names=dev["state_names"], max_bits=dev["max_bits"], sample_rate=dev["sample_rate"],
                          **{k: dev[k] for k in _TABLE_KEYS})


def ok_device(ok, dev):
    return ok.Device.from_tables(max_bits=dev["max_bits"], sample_rate=dev["sample_rate"],
                                 **{k: dev[k] for k in _TABLE_KEYS})


def scan_domain(dev):
    """abstract states of the scan form (rx.cpp setup_scan): above SCAN_DOMAIN_MAX the context runs the round form"""
    return len(dev["state_names"]) * (dev["max_bits"] + 2) + 3


def iq_of(runs_or_stream):
    """I,Q samples (Q = 0) of a run list or a 0/1 stream"""
    s = runs_or_stream if isinstance(runs_or_stream, np.ndarray) else stream_from_runs(runs_or_stream)
    iq = np.zeros(2 * s.size, np.int16)
    iq[0::2] = s.astype(np.int16) * AMP
    return iq


# --------------------------------------------------------------------------------------------------- streams ----

LEAD = 300          # low samples in front of the first message


def burst_runs(nbits, nmsg, seed, lead=LEAD, gap=(230, 400), payloads=None):
    """nmsg messages of random bits: [20, 50 or 20] per bit, then [20, gap]"""
    rng = np.random.default_rng(seed)
    runs = [lead]
    for m in range(nmsg):
        bits = rng.integers(0, 2, size=nbits) if payloads is None else payloads[m]
        for b in bits:
            runs += [20, 50 if b else 20]
        runs += [20, int(rng.integers(gap[0], gap[1]))]
    return runs


RLE_PERIOD = 11     # samples between two time-outs of rle's `off` (10 us: the counter passes 0 .. 10)


def rle_low(z):
    """Length of the low run whose span appends z bits: z - 1 zeros by time-out and the one of the pulse that ends it
    (that edge is the span's last sample).  The falling edge, z - 1 periods of the time-out and 4 samples more.  (A
    time-out of 10 us runs out every ELEVEN samples: a run of 10 z + 5 appends fewer than z zeros from z = 6 on.)"""
    assert z >= 1
    return RLE_PERIOD * (z - 1) + 5


def rle_message_runs(groups):
    """one message whose bits are, per entry z of `groups`, z - 1 zeros and a one (z appends in one span): the opening
    pulse, then per group the low run and a 20 us pulse (the last pulse completes the message on its second sample)"""
    runs = []
    for z in groups:
        runs += [20, rle_low(z)]
    return runs + [20]


def rle_groups(nbits, z, rng, fill=(1, 2, 3, 4)):
    """groups that add up to nbits bits with one group of z at a random place, the rest short (never above z)"""
    assert z <= nbits
    rest, out = nbits - z, []
    while rest:
        g = min(int(rng.choice(fill)), rest, z)
        out.append(g)
        rest -= g
    out.insert(int(rng.integers(0, len(out) + 1)), z)
    return out


def rle_runs(nbits, z, nmsg, seed, lead=LEAD, gap=(100, 300), fill=(1, 2, 3, 4)):
    """nmsg messages of nbits bits, each with ONE span of z appends; every other span holds at most min(z, max(fill))"""
    rng = np.random.default_rng(seed)
    runs = [lead]
    for _ in range(nmsg):
        runs += rle_message_runs(rle_groups(nbits, z, rng, fill)) + [int(rng.integers(gap[0], gap[1]))]
    return runs


def rle_dense_runs(nbits, z, nmsg, seed, lead=LEAD, gap=(100, 300)):
    """messages made of groups of up to z appends (zeros and a one): bits set all over a long payload"""
    rng = np.random.default_rng(seed)
    runs = [lead]
    for _ in range(nmsg):
        groups, rest = [], nbits
        while rest:
            g = min(int(rng.integers(1, z + 1)), rest)
            groups.append(g)
            rest -= g
        runs += rle_message_runs(groups) + [int(rng.integers(gap[0], gap[1]))]
    return runs


def ticker_runs(outputs, npulses, seed, lead=LEAD, gap=(30, 200)):
    """npulses high runs of 50 * outputs + 10 samples: `outputs` messages inside one span each"""
    rng = np.random.default_rng(seed)
    runs = [lead]
    for _ in range(npulses):
        runs += [50 * outputs + 10, int(rng.integers(gap[0], gap[1]))]
    return runs


def pacer_runs(fires, npulses, seed, lead=LEAD, gap=(30, 200)):
    """npulses high runs in which `pace` times out `fires` times: the rising edge, `fires` periods and 4 samples more;
    the falling edge that ends the span is one more firing, on the span's last sample"""
    rng = np.random.default_rng(seed)
    runs = [lead]
    for _ in range(npulses):
        runs += [RLE_PERIOD * fires + 5, int(rng.integers(gap[0], gap[1]))]
    return runs


def drip_runs(nedges, seed, lead=LEAD, run=(3, 25)):
    """random short runs: about one append per span, far below the pool's two.  Cut to whole buffers of 4096 (a run
    pads the capture with zeros, through which drip would go on appending -- past kMaxLeafApps in one span)."""
    rng = np.random.default_rng(seed)
    runs = [lead] + [int(x) for x in rng.integers(run[0], run[1], size=nedges)]
    end = np.cumsum(runs)
    whole = int(end[-1]) // 4096 * 4096
    keep = int(np.searchsorted(end, whole, side="left"))        # runs[keep] holds sample whole - 1
    runs = runs[:keep + 1]
    runs[keep] -= int(end[keep]) - whole
    return runs


def error_runs(spb, nbuf, high=8):
    """[high, spb - high] per buffer for burst: the pulse is too short for `on`, its falling edge is an error and the
    rest of the buffer is dropped"""
    return [0] + [high, spb - high] * nbuf


def pool_runs(total_extra, seed=0, lead=LEAD):
    """One rle(40) capture whose appends number 2 * (edges + 1) + 512 + total_extra: messages of four groups of ten
    appends (per two edges), then an unfinished one whose last low run, with no edge behind it, tunes the total to
    the unit."""
    rng = np.random.default_rng(seed)
    runs = [lead]
    edges, apps = 0, 0
    nmsg = 25
    for _ in range(nmsg):
        runs += rle_message_runs([10, 10, 10, 10]) + [int(rng.integers(100, 300))]
        edges += 2 + 2 * 4
        apps += 40
    # the unfinished message: pulse (2 edges), then z zeros by time-out up to the capture's end
    edges += 2
    z = 2 * (edges + 1) + POOL_EXTRA + total_extra - apps
    assert 0 < z < MAX_LEAF_APPS, z
    runs += [20, RLE_PERIOD * z + 5]
    # (a run pads the capture to whole buffers with zeros, through which `off` would go on appending: the silence in
    #  front makes it whole buffers of any size up to 8192)
    runs[0] += -sum(runs) % 8192
    return runs


# ----------------------------------------------------------------------------------- what a stream holds ----

def leaf_stats(oracle, dev, stream, spb):
    """Per leaf of the scan -- leaf i: the samples behind edge i-1 up to and including edge i; leaf 0 from the
    capture's start, the last one to its end -- what the oracle's state machine does inside it: (appends, outputs,
    errors) as three arrays.  The stream is fed buffer by buffer as device.c does (an error drops the rest of its
    buffer)."""
    bits = np.ascontiguousarray(stream, np.uint8)
    fsm = fsm_desc(oracle, dev)
    L = oracle.lib()
    cs = fsm.c_struct()
    h = L.ook_sm_new(C.byref(cs))
    e = edges_of(bits)
    cuts = np.concatenate([e + 1, [bits.size]]).astype(np.int64)        # leaf i ends in front of cuts[i]
    cuts = cuts[cuts <= bits.size]
    napp = np.zeros(cuts.size, np.int64)
    nout = np.zeros(cuts.size, np.int64)
    nerr = np.zeros(cuts.size, np.int64)
    nproc, nb, st = C.c_uint(0), C.c_uint32(0), C.c_uint32(0)
    el, pb = C.c_double(0), C.c_int(0)

    def nbits():
        # (in the reset state the count is zeroed on the next sample, before anything can append)
        L.ook_sm_peek(h, C.byref(st), C.byref(nb), C.byref(el), C.byref(pb))
        return 0 if st.value == 0 else nb.value

    pos, leaf = 0, 0
    while pos < bits.size:
        while cuts[leaf] <= pos:
            leaf += 1
        buf_end = min((pos // spb + 1) * spb, bits.size)
        end = min(int(cuts[leaf]), buf_end)
        before = nbits()
        r = L.ook_sm_process(h, bits[pos:].ctypes.data, end - pos, C.byref(nproc))
        pos += nproc.value
        after = nbits()
        # (a reset zeroes the count on the sample behind the output or the error: never together with an append here)
        if after > before:
            napp[leaf] += after - before
        if r == 1:
            nout[leaf] += 1
        elif r == -1:
            nerr[leaf] += 1
            pos = buf_end
    L.ook_sm_free(h)
    return napp, nout, nerr


def collected_at(oracle, dev, stream, spb, positions):
    """(state, bits collected) of the oracle's state machine in front of each of the (increasing) sample positions;
    the stream must not hold an error (a dropped rest-of-buffer is not modelled here)"""
    bits = np.ascontiguousarray(stream, np.uint8)
    fsm = fsm_desc(oracle, dev)
    L = oracle.lib()
    cs = fsm.c_struct()
    h = L.ook_sm_new(C.byref(cs))
    nproc, nb, st = C.c_uint(0), C.c_uint32(0), C.c_uint32(0)
    el, pb = C.c_double(0), C.c_int(0)
    out, pos = [], 0
    for p in positions:
        while pos < p:
            r = L.ook_sm_process(h, bits[pos:].ctypes.data, int(p) - pos, C.byref(nproc))
            assert r != -1
            pos += nproc.value
        L.ook_sm_peek(h, C.byref(st), C.byref(nb), C.byref(el), C.byref(pb))
        out.append((st.value, 0 if st.value == 0 else nb.value))
    L.ook_sm_free(h)
    return out


def carried_at(oracle, dev, stream, pos):
    """(state, bits collected, payload bytes so far) of the oracle's state machine in front of sample `pos`: what a
    shard that ends there hands to the next (no error in front of it)"""
    bits = np.ascontiguousarray(stream, np.uint8)
    fsm = fsm_desc(oracle, dev)
    L = oracle.lib()
    cs = fsm.c_struct()
    h = L.ook_sm_new(C.byref(cs))
    nproc, nb, st = C.c_uint(0), C.c_uint32(0), C.c_uint32(0)
    el, pb = C.c_double(0), C.c_int(0)
    at = 0
    while at < pos:
        r = L.ook_sm_process(h, bits[at:].ctypes.data, int(pos) - at, C.byref(nproc))
        assert r != -1
        at += nproc.value
    L.ook_sm_peek(h, C.byref(st), C.byref(nb), C.byref(el), C.byref(pb))
    d = L.ook_sm_data(h)
    data = bytes(d[i] for i in range(fsm.payload_bytes))
    L.ook_sm_free(h)
    return st.value, nb.value, data


def moved_to_boundary(oracle, dev, stream, target_bits, grid):
    """The stream with so much put in front of it -- and cut to whole multiples of `grid` behind -- that a multiple of
    `grid` falls where the state machine holds at least target_bits collected bits of an unfinished message: where a
    chunk of a pipelined run, or a shard, hands every word of its payload on.  In front go low samples; for drip, which
    appends a zero every 11 us of silence (more than a span's record holds, in so long a one), pulses of 8 us: a one
    every 16."""
    always_on = len(dev["state_names"]) == 2

    def moved(shift):
        front = ((np.arange(shift) // 8) & 1).astype(np.uint8) if always_on else np.zeros(shift, np.uint8)
        m = np.concatenate([front, stream])
        return m[:m.size // grid * grid]

    def holds(m):
        cuts = np.arange(grid, m.size, grid)
        return any(st != 0 and target_bits <= nb < dev["max_bits"] for st, nb in collected_at(oracle, dev, m, grid, cuts))

    if not always_on:
        pos = np.arange(2, stream.size, 2)
        for p, (st, nb) in zip(pos, collected_at(oracle, dev, stream, grid, pos)):
            if st != 0 and target_bits <= nb < dev["max_bits"]:
                m = moved(int(-p % grid))
                assert holds(m)
                return m
    for shift in range(grid):       # (what goes in front moves drip's message boundaries: try)
        m = moved(shift)
        if holds(m):
            return m
    raise AssertionError("no message of the stream collects %d bits" % target_bits)


# ------------------------------------------------------------------------------------------------- the cases ----
# name -> (device, runs); built on demand, the same on the CPU and on the GPU

BURST_BITS = (1, 8, 9)
BURST_MESSAGES = 3000
RLE_BITS = 40
COMPACT_Z = (1, 7, 8, 9, 16)            # appends in one span around the one-word record's eight
LIMIT_Z = (30, 31)                      # ... around kMaxLeafApps
TICKER_OUTPUTS = (1, 2, 3, 4)           # outputs in one span around the record's two
PACER_FIRES = (47, 48, 49)              # time-outs in one span around kMaxFires (the edge that ends it fires once more)
LONG_BITS = (63, 64, 65, 127, 128, 129, 254)
DRIP_BITS = (129, 188)                  # two states: payload words 1 and 2 inside the scan's domain
ERROR_STREAMS = {"spb64": (64, 66000), "spb97": (97, 3000), "spb64x2": (64, 132000)}


def burst_case(nbits, chunk=4 * 4096):
    """BURST_MESSAGES messages; the silence in front is stretched so that a multiple of `chunk` (the pipelined legs'
    chunk at 4096 samples per buffer) lies in the gap between message 2047 and message 2048: the last message of the
    pinned head and the first of the device tail come from different chunks"""
    runs = burst_runs(nbits, BURST_MESSAGES, seed=100 + nbits)
    gap = HOST_MSG_FIRST * (2 * nbits + 2)          # index of the gap behind message 2047
    mid = sum(runs[:gap]) + runs[gap] // 2
    runs[0] += -mid % chunk
    return burst(nbits), runs


def rle_case(z, nmsg=20):
    return rle(RLE_BITS), rle_runs(RLE_BITS, z, nmsg, seed=200 + z)


def ticker_case(outputs, npulses=100):
    return ticker(), ticker_runs(outputs, npulses, seed=300 + outputs)


def pacer_case(fires, npulses=60):
    return pacer(), pacer_runs(fires, npulses, seed=400 + fires)


def pool_case(extra):
    return rle(RLE_BITS), pool_runs(extra)


def long_case(kind, nbits, nmsg=12):
    if kind == "rle":
        return rle(nbits), rle_dense_runs(nbits, 4, nmsg, seed=500 + nbits)
    if kind == "drip":
        return drip(nbits), drip_runs(60 * nbits, seed=600 + nbits)
    return burst(nbits), burst_runs(nbits, nmsg, seed=700 + nbits)


def error_case(name):
    spb, nbuf = ERROR_STREAMS[name]
    return burst(8), error_runs(spb, nbuf), spb


def recorded_cases():
    """(name, device, runs): short versions of every stream above -- at most 200 messages each -- whose decoding by
    the reference's own state machine is committed (tests/golden/dense_ref_recorded.json)"""
    for n in BURST_BITS:
        yield "burst%d" % n, burst(n), burst_runs(n, 100, seed=100 + n)
    for z in COMPACT_Z + LIMIT_Z:
        yield "rle40_z%d" % z, rle(RLE_BITS), rle_runs(RLE_BITS, z, 20, seed=200 + z)
    for k in TICKER_OUTPUTS:
        yield "ticker_%d" % k, ticker(), ticker_runs(k, 40, seed=300 + k)
    for f in PACER_FIRES:
        yield "pacer_%d" % f, pacer(), pacer_runs(f, 10, seed=400 + f)
    for extra in (0, 1):
        yield "pool_%d" % extra, rle(RLE_BITS), pool_runs(extra)
    for n in LONG_BITS:
        for kind in ("rle", "burst"):
            dev, runs = long_case(kind, n, nmsg=4)
            yield "long_%s%d" % (kind, n), dev, runs
    for n in DRIP_BITS:
        yield "long_drip%d" % n, drip(n), drip_runs(20 * n, seed=600 + n)
    for spb in (64, 97):
        yield "errors_spb%d" % spb, burst(8), error_runs(spb, 200)
