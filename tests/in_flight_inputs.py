"""Captures and schedules of the in-flight tests (test_gpu_in_flight.py; checked on the CPU by test_in_flight_host.py),
numpy, the golden vectors and the library's host-side synthesiser only.

Several contexts with a run in flight each, behind one front-end gate, is how bench.py measures and how INTEGRATION.md
tells hosts to work (ookd_rx_submit_device / ookd_rx_wait).  A test of that path sees crosstalk only if the contexts hold
DIFFERENT captures at the same time: `capture(name)` gives the named captures below, each built deterministically, and
the schedules are plain lists of steps ("submit", context, capture name) / ("wait", context) in which no two contexts
ever hold the same capture at once.  Nothing here knows what the kernels compute."""
import collections
import json
import os

import numpy as np

from tests.helpers import GOLDEN, edges_of, golden_path, iq_from_rle, stream_from_runs

RATE, SPB, THR = 3000000, 8192, 0.1
NOISE = 40                      # +-LSB on both components
AMP = 1945                      # the golden captures' "on" level
SHIFT = 77000                   # g1_shifted: pulses where g1 has silence

# The smallest power-of-two length at which the forced walk from synchronising spans gives up on the first run of a
# fresh context (stats: fsm_path 1 with scan_entry_form 2, where a walk that held reports 1).
NOSYNC_LOG2 = 25
NOSYNC_NOTE = ("measured on an MI355X, fs32_fs4 and no filter, first and second run of a fresh context under "
               "OOKD_SYNC_MIN_EDGES=0: at 2^16 .. 2^24 samples (8 .. 3001 edges) the walk holds (scan_entry_form 1), at "
               "2^25 (6026 edges) it gives up.  Nothing shorter gives up: 2^25, the length of "
               "test_scan_walk_gives_up_and_the_scan_composes, stays for this one capture")

# dense_edges: runs of DENSE_RUN samples, alternately off and on, DENSE_RUNS of them behind a low lead -- one edge per
# run boundary, the first at DENSE_LEAD; the last run is low, so the capture's end adds none
DENSE_LEAD, DENSE_RUN, DENSE_RUNS = 300, 37, 4000
DENSE_EDGES = DENSE_RUNS        # what the overflow leg sizes edge_capacity from (test_in_flight_host.py holds it)

NOTES = {
    "g1": "golden capture G1 (three p3l-nexa2012 messages) with noise",
    "g2": "golden capture G2 (two unknown-remote1 messages) with noise: another length, other pulse shapes",
    "g1_shifted": "g1 moved by 77 000 samples: pulses where g1 has silence, messages at other samples",
    "silence": "noise of +-40 LSB: nothing may survive, whatever the neighbours hold",
    "short": "5 000 samples of g1 around its first pulse: far fewer tiles than the run before",
    "one": "1 sample, on: the filter's answer to it and nothing else",
    "empty": "0 samples: a run that launches next to nothing",
    "deep": "six p3l messages, six glitches inside ONE bit gap of the third (twelve inert edges): the scan refuses it "
            "(2.5 M samples without a filter: the builder of test_batch_with_one_refused_capture_redoes_only_that_one, "
            "unchanged)",
    "nosync": "Synth(p3l-nexa2012, gap_us=(4000, 5500), glitch_every=0): gaps under the longest time-out, the forced "
              "walk from synchronising spans gives up",
    "dense_edges": "a square wave of known edge count (DENSE_EDGES) for the overflow leg",
}

_made = {}


def _vectors():
    if "vectors" not in _made:
        with open(os.path.join(GOLDEN, "vectors.json")) as f:
            _made["vectors"] = json.load(f)
    return _made["vectors"]


def _golden(name, noise_seed):
    """as _g1 of test_gpu_parity.py: the golden capture plus uniform noise on both rails"""
    g = _vectors()[name]
    iq = iq_from_rle(g["i_rle"], g["num_samples"])
    rng = np.random.default_rng(noise_seed)
    return (iq + rng.integers(-NOISE, NOISE + 1, size=iq.size)).astype(np.int16)


def iq_from_stream(stream, amp=AMP):
    iq = np.zeros(2 * stream.size, dtype=np.int16)
    iq[0::2] = stream.astype(np.int16) * amp
    return iq


def p3l_message_captures(deep_flags, seed=9):
    """Captures of six p3l-nexa2012 messages each, built one after the other from ONE generator.  A True flag puts a
    stretch of inert edges deeper than the scan's stuck codes hold into the third message: six short pulses inside one
    bit gap, twelve edges on which nothing fires."""
    us = RATE // 1000000
    sh = dict(bits=36, start=500, first=8700, pulse=500, gap0=2000, gap1=4000)

    def message(bits, deep_at=None):
        runs = [sh["start"] * us, sh["first"] * us]
        for i, bit in enumerate(bits):
            gap = (sh["gap1"] if bit else sh["gap0"]) * us
            runs.append(sh["pulse"] * us)
            if i == deep_at:
                pre = []
                for _ in range(6):
                    pre += [150, 90]                    # low 150, glitch 90: ends long before any bit window opens
                runs += pre + [gap - sum(pre)]
            else:
                runs.append(gap)
        return runs + [sh["pulse"] * us, 20000]

    rng = np.random.default_rng(seed)

    def capture(deep):
        runs = [5000]
        for m in range(6):
            bits = rng.integers(0, 2, size=sh["bits"])
            ones = [i for i, b in enumerate(bits) if b]
            runs += message(bits, deep_at=(ones[len(ones) // 2] if (deep and m == 2 and ones) else None))
        return iq_from_stream(stream_from_runs(runs))

    return [capture(bool(d)) for d in deep_flags]


def refused_batch():
    """Three captures for one batched run: p3l_message_captures((False, True, False)), each with one pulse of its last
    message stretched to 2400 samples -- the machine reports errors in every capture, the scan still refuses the middle
    one for its third message -- and all padded with zeros to one length.  -> (samples per capture, [iq])"""
    caps = p3l_message_captures((False, True, False))
    n = max(c.size // 2 for c in caps)
    out = []
    for c in caps:
        x = np.zeros(2 * n, np.int16)
        x[:c.size] = c
        e = edges_of(x[0::2] > AMP // 2)
        rise = int(e[int(e.size * 0.9) & ~1])           # (even entries of an edge list are rising edges)
        x[2 * rise:2 * (rise + 2400):2] = AMP
        out.append(x)
    return n, out


def dense_runs():
    return [DENSE_LEAD] + [DENSE_RUN] * DENSE_RUNS


def _build(name):
    if name == "g1":
        return _golden("G1", 41)
    if name == "g2":
        return _golden("G2", 43)
    if name == "g1_shifted":
        a = capture("g1")
        rng = np.random.default_rng(42)
        return np.concatenate([rng.integers(-NOISE, NOISE + 1, size=2 * SHIFT).astype(np.int16), a[:-2 * SHIFT]])
    if name == "silence":
        return np.random.default_rng(44).integers(-NOISE, NOISE + 1, size=2 * 700000).astype(np.int16)
    if name == "short":
        return capture("g1")[2 * 11000:2 * 16000].copy()       # starts inside the idle gap before the first pulse
    if name == "one":
        return np.array([AMP, 0], dtype=np.int16)
    if name == "empty":
        return np.zeros(0, dtype=np.int16)
    if name == "deep":
        return p3l_message_captures((False, True))[1]
    if name == "nosync":
        import ookiedokie_amd as ok                 # (the synthesiser's host side: no GPU)
        d = ok.Device.load(golden_path("devices", "p3l-nexa2012"), RATE)
        return ok.Synth(d, 1 << NOSYNC_LOG2, seed=12, sample_rate=RATE, gap_us=(4000, 5500), glitch_every=0).fill_host()
    if name == "dense_edges":
        return iq_from_stream(stream_from_runs(dense_runs()))
    raise KeyError(name)


def capture(name):
    """the named capture as interleaved int16 I,Q, read-only, built once"""
    if name not in _made:
        assert name in NOTES, name
        iq = np.ascontiguousarray(_build(name), dtype=np.int16)
        iq.setflags(write=False)
        _made[name] = iq
    return _made[name]


def length(name):
    return capture(name).size // 2


# --------------------------------------------------------------------------------------- oracle results ----

Want = collections.namedtuple("Want", "decimated msgs errs bits edges")
_want = {}


def oracle_filter(oracle, filt):
    """None, the name of a golden filter, or the name of a generic shape of tests/front_shapes_inputs.py"""
    from tests import front_shapes_inputs as S
    if filt is None:
        return None
    if filt in S.GENERIC_SHAPES:
        return oracle.make_fir(S.stages(S.GENERIC_SHAPES[filt]))
    return oracle.load_filter_json(golden_path("filters", filt))


def oracle_result(oracle, name, filt="fs32_fs4", devname="p3l-nexa2012", thr=THR, iq=None):
    """The oracle's result for a capture, computed once per (capture, filter, device, threshold) and left unchanged.
    iq: samples of a capture that is not one of the named ones (a widened 8-bit copy, a slice of a batch) -- `name` is
    then the key alone."""
    key = (name, filt, devname, float(thr))
    if key not in _want:
        of = oracle_filter(oracle, filt)
        dec = of.total_decimation if of else 1
        od = oracle.load_device_json(golden_path("devices", devname), RATE // dec)[0] if devname else None
        w = oracle.rx(capture(name) if iq is None else iq, of, thr, od, SPB, want_bits=True)
        bits = w.bits
        bits.setflags(write=False)
        msgs = tuple((int(s), bytes(p)) for s, p in zip(w.msg_samples, w.payloads))
        _want[key] = Want(w.decimated, msgs, tuple(int(e) for e in w.err_samples), bits,
                          tuple(int(e) for e in edges_of(bits)))
    return _want[key]


# ------------------------------------------------------------------------------------------ schedules ----
# A schedule is a list of steps ("submit", ctx, capture name) | ("wait", ctx).  Step k of a schedule takes capture
# ring[k % len(ring)]: K runs in flight are K neighbours of the ring.  Three captures decode to nothing on the
# two-stage filter (`silence`, `empty`, and `one`, whose single sample the decimation swallows): the rings keep them at
# least K apart, so that whatever flies together differs in what it decodes to.

RING2 = ("g1", "silence", "short", "one", "g2", "empty", "g1_shifted")          # K = 2
RING3 = ("g1", "short", "silence", "g2", "g1_shifted", "empty", "g2")           # K = 3
RING5 = ("g1", "short", "g2", "g1_shifted", "one")                              # K = 4, and one_hot's five in flight


def ring_for(K):
    return {2: RING2, 3: RING3}.get(K, RING5)


def round_robin(K, captures=None, steps=None):
    """bench.py's timed_steps: step k goes to context k % K, which is first waited for (step k - K ran on it) while
    the other K - 1 runs are still in flight; the last K runs are waited for in the order they were queued."""
    captures = captures or ring_for(K)
    steps = steps if steps is not None else 4 * K
    out = []
    for k in range(steps):
        if k >= K:
            out.append(("wait", k % K))
        out.append(("submit", k % K, captures[k % len(captures)]))
    for k in range(max(0, steps - K), steps):
        out.append(("wait", k % K))
    return out


def lifo(K, captures=None, rounds=4):
    """submit to all contexts, wait in reverse order"""
    captures = captures or ring_for(K)
    out = []
    for r in range(rounds):
        for c in range(K):
            out.append(("submit", c, captures[(r * K + c) % len(captures)]))
        for c in reversed(range(K)):
            out.append(("wait", c))
    return out


def fifo_lagged(captures=None, ncaptures=9):
    """the loop of INTEGRATION.md "Captures in flight": two contexts alternate, capture k is queued before capture
    k - 1 is waited for"""
    captures = captures or RING2
    out = [("submit", 0, captures[0])]
    for k in range(1, ncaptures):
        out.append(("submit", k & 1, captures[k % len(captures)]))
        out.append(("wait", (k - 1) & 1))
    out.append(("wait", (ncaptures - 1) & 1))
    return out


def one_hot(K, captures=None, phases=3, hot_steps=3):
    """Per phase one context (phase % K) runs hot_steps runs, one after the other, while every other context holds one
    run in flight the whole time -- queued before the hot context's first run, waited for after its last.  (K - 1 +
    hot_steps neighbours of the ring fly together.)"""
    captures = captures or RING5
    out, k = [], 0
    for p in range(phases):
        hot = p % K
        cold = [c for c in range(K) if c != hot]
        for c in cold:
            out.append(("submit", c, captures[k % len(captures)]))
            k += 1
        for _ in range(hot_steps):
            out.append(("submit", hot, captures[k % len(captures)]))
            out.append(("wait", hot))
            k += 1
        for c in cold:
            out.append(("wait", c))
    return out


def schedules():
    """name -> (number of contexts, schedule): every schedule the GPU legs play"""
    out = collections.OrderedDict()
    for K in (2, 3, 4):
        out["round_robin%d" % K] = (K, round_robin(K))
    out["lifo3"] = (3, lifo(3))
    out["fifo_lagged"] = (2, fifo_lagged())
    out["one_hot3"] = (3, one_hot(3))
    return out


def walk(schedule):
    """Plays a schedule on paper: yields (step, {ctx: capture in flight} after the step).  Raises on a submit to a
    context with a run in flight and on a wait for a context without one."""
    held = {}
    for step in schedule:
        if step[0] == "submit":
            _, c, name = step
            if c in held:
                raise ValueError("two submits without a wait on context %d" % c)
            held[c] = name
        elif step[0] == "wait":
            if step[1] not in held:
                raise ValueError("wait without a submit on context %d" % step[1])
            del held[step[1]]
        else:
            raise ValueError(step)
        yield step, dict(held)


def seen_by(schedule):
    """ctx -> the captures it is given, in order"""
    out = collections.defaultdict(list)
    for step in schedule:
        if step[0] == "submit":
            out[step[1]].append(step[2])
    return dict(out)


def together(schedule):
    """the set of pairs of captures that are in flight at the same time somewhere in the schedule"""
    pairs = set()
    for _, held in walk(schedule):
        names = sorted(held.values())
        if len(set(names)) != len(names):
            raise ValueError("two contexts hold %s at the same time" % names)
        pairs.update((a, b) for i, a in enumerate(names) for b in names[i + 1:])
    return pairs
