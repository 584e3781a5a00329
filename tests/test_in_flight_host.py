"""What test_gpu_in_flight.py relies on, checked without a GPU: the schedules of tests/in_flight_inputs.py are well
formed and hold distinct captures in flight, the oracle's results for captures that fly together differ (crosstalk
would show), and the designed captures hold what their legs are about."""
import numpy as np
import pytest

from tests import in_flight_inputs as I
from tests.helpers import edges_of

SCHEDULES = I.schedules()
# the forms the schedule legs run on: (filter, device)
FORMS = (("fs32_fs4", "p3l-nexa2012"), ("fs128_fs16_dec4", "p3l-nexa2012"))


def test_captures_are_named_sized_and_repeatable():
    for name in I.NOTES:
        if name == "nosync":
            continue                    # (built by the library's synthesiser: below)
        a = I.capture(name)
        assert a.dtype == np.int16 and a.size % 2 == 0 and not a.flags.writeable, name
        assert (np.array(I._build(name)) == a).all(), name
    g1 = I.capture("g1")
    assert I.length("g1") == 1221300 and I.length("g1_shifted") == I.length("g1")
    assert (I.capture("g1_shifted")[2 * I.SHIFT:] == g1[:-2 * I.SHIFT]).all()
    assert np.abs(I.capture("silence")).max() <= I.NOISE
    assert I.length("short") == 5000 and I.length("one") == 1 and I.length("empty") == 0
    # every capture of the schedules within G1's size
    for ring in (I.RING2, I.RING3, I.RING5):
        assert all(I.length(nm) <= I.length("g1") for nm in ring)


def test_nosync_is_the_synthesiser_capture_of_the_stated_length():
    a = I.capture("nosync")
    assert a.size == 2 << I.NOSYNC_LOG2 and a.dtype == np.int16
    assert I.NOSYNC_NOTE


@pytest.mark.parametrize("name", list(SCHEDULES))
def test_schedule_is_well_formed(name):
    K, sched = SCHEDULES[name]
    held = {}
    for step, held in I.walk(sched):            # raises on a second submit, on a wait for nothing
        assert step[0] in ("submit", "wait") and 0 <= step[1] < K
        if step[0] == "submit":
            assert step[2] in I.NOTES
    assert held == {}, "a submit is never waited for"
    assert sorted(I.seen_by(sched)) == list(range(K))
    with pytest.raises(ValueError):
        list(I.walk([("submit", 0, "g1"), ("submit", 0, "g2")]))
    with pytest.raises(ValueError):
        list(I.walk([("wait", 0)]))


@pytest.mark.parametrize("name", list(SCHEDULES))
def test_schedule_properties(name):
    """every context sees at least three different captures of three different lengths, a longer one followed by a
    shorter one; no two contexts in flight at the same time hold the same capture; more than one run is in flight"""
    K, sched = SCHEDULES[name]
    for c, names in I.seen_by(sched).items():
        assert len(set(names)) >= 3, (c, names)
        assert len({I.length(nm) for nm in names}) >= 3, (c, names)
        assert any(I.length(a) > I.length(b) for a, b in zip(names, names[1:])), (c, names)
    pairs = I.together(sched)                   # raises if two contexts hold one capture at a time
    assert pairs
    with pytest.raises(ValueError):
        I.together([("submit", 0, "g1"), ("submit", 1, "g1"), ("wait", 0), ("wait", 1)])
    assert max(len(held) for _, held in I.walk(sched)) == K


def test_round_robin_is_the_bench_order():
    """bench.py timed_steps, restated: for k in range(steps): h = k % K; if k >= K: finish(h); submit(h); then finish
    the last K in order"""
    for K in (2, 3, 4):
        steps = 4 * K
        sched = I.round_robin(K)
        want = []
        for k in range(steps):
            if k >= K:
                want.append(("wait", k % K))
            want.append(("submit", k % K))
        want += [("wait", k % K) for k in range(steps - K, steps)]
        assert [s[:2] for s in sched] == want
    # INTEGRATION.md's loop
    assert [s[:2] for s in I.fifo_lagged(ncaptures=3)] == [("submit", 0), ("submit", 1), ("wait", 0), ("submit", 0),
                                                          ("wait", 1), ("wait", 0)]


def _differ(a, b):
    return a.msgs != b.msgs or a.edges != b.edges


@pytest.mark.parametrize("filt,devname", FORMS)
def test_results_of_captures_in_flight_together_differ(oracle, filt, devname):
    pairs = set()
    for K, sched in SCHEDULES.values():
        pairs |= I.together(sched)
    assert len(pairs) >= 10
    for a, b in sorted(pairs):
        assert _differ(I.oracle_result(oracle, a, filt, devname), I.oracle_result(oracle, b, filt, devname)), (a, b)
    # what the rings keep apart decodes to the same (nothing) ...
    s, e = (I.oracle_result(oracle, nm, filt, devname) for nm in ("silence", "empty"))
    assert not s.msgs and not s.edges and not s.bits.any() and not _differ(s, e) and ("empty", "silence") not in pairs
    # (`one`: the 32-tap filter's answer to one sample crosses the threshold, the two-stage filter swallows it)
    assert I.oracle_result(oracle, "one", "fs32_fs4", devname).edges
    assert not I.oracle_result(oracle, "one", "fs128_fs16_dec4", devname).edges
    # ... and the golden captures decode to their messages
    assert len(I.oracle_result(oracle, "g1", filt, devname).msgs) == 3
    assert len(I.oracle_result(oracle, "g1_shifted", filt, devname).msgs) >= 2


def test_deep_has_twelve_inert_edges_inside_one_gap(oracle):
    """six glitches of 90 samples, 150 apart, inside one 4000 us gap of the third message: twelve edges between two
    pulses of 1500 samples; the oracle decodes the message all the same"""
    plain, deep = I.p3l_message_captures((False, True))
    assert (deep == I.capture("deep")).all()
    w = I.oracle_result(oracle, "deep", None)
    e = np.array(w.edges, dtype=np.int64)
    runs = np.diff(e)
    short = np.nonzero(runs[::2] == 90)[0]          # "on" runs of 90 samples: the glitches
    assert short.size == 6 and (np.diff(short) == 1).all()
    first = 2 * int(short[0])
    inert = e[first:first + 12]
    assert list(np.diff(inert)) == [90, 150] * 5 + [90]
    assert runs[first - 2] == 1500 and runs[first - 1] == 150             # the bit's pulse, then the first low stretch
    gap = e[first + 12] - e[first - 1]
    assert gap == 12000 and runs[first + 12] == 1500                        # one gap of 4000 us, the next pulse
    assert len(w.msgs) == 6 and w.decimated >= 2400000
    # (without the glitches: a capture of the same kind, no such stretch)
    assert not (np.diff(np.array(edges_of(plain[0::2] > 1000)))[::2] == 90).any()


def test_refused_batch_reports_errors_in_every_capture(oracle):
    """the error order of a batch with a refused capture is asserted on lists that are not empty, the refused capture
    keeps its stretch of inert edges, and every capture still decodes five messages"""
    n, members = I.refused_batch()
    assert len(members) == 3 and all(m.size == 2 * n for m in members)
    for c, x in enumerate(members):
        w = I.oracle_result(oracle, "refused_batch|%d" % c, None, "p3l-nexa2012", I.THR, iq=x)
        assert len(w.errs) >= 2 and len(w.msgs) == 5, (c, w.errs, len(w.msgs))
        on = np.diff(np.array(w.edges))[::2]
        assert int(np.count_nonzero(on == 90)) == (6 if c == 1 else 0) and int(np.count_nonzero(on == 2400)) == 1
        if c == 1:              # the errors lie behind the glitches: the message that holds them is clean
            assert min(w.errs) > max(e for e, r in zip(w.edges[::2], on) if r == 90)


def test_dense_edges_has_the_edge_count_the_overflow_leg_sizes_from(oracle):
    w = I.oracle_result(oracle, "dense_edges", None)
    assert len(w.edges) == I.DENSE_EDGES == len(I.dense_runs()) - 1
    assert w.edges[0] == I.DENSE_LEAD and set(np.diff(w.edges)) == {I.DENSE_RUN}
    # `short`, which the failed context decodes next, fits a list one entry too small for dense_edges
    assert 0 < len(I.oracle_result(oracle, "short", None).edges) < I.DENSE_EDGES - 1
