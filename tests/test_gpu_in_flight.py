"""Captures in flight (ookd_rx_submit_device / ookd_rx_wait): several contexts, each with a run queued,
behind one front-end gate -- the path bench.py measures on.  Every context holds a DIFFERENT capture while the others
run (tests/in_flight_inputs.py; what the captures and schedules hold is checked without a GPU in
test_in_flight_host.py), and after every wait that context's run is compared with the CPU oracle's result for the
capture IT was given: messages (sample, payload, capture index), every error position, edges, num_edges, bits.
Everything is exact.  Had a context read a neighbour's bit words, tile infos, header, pinned messages or edge list, or
taken a stale stamp or ticket for a live one, its result would be the neighbour's or a mixture, and differ.

Legs: 1 schedules x forms (alike, without a gate, contexts that differ, tuned + carriers), 2 every redo that
ookd_rx_wait may run on the stream, with neighbours in flight, 3 an edge list overflow in flight, 4 the gate's life,
5 two host threads, 6 a caller's stream, 7 split front-end launches where nothing met them, 8 a post-run pass beside a
neighbour's run.  Schedules are deterministic; nothing here measures time (tools/overlap_cost.py does)."""
import collections
import threading

import numpy as np
import pytest

from tests import front_shapes_inputs as S
from tests import in_flight_inputs as I
from tests import pulse_contract as P
from tests.helpers import edges_of, golden_path
from tests.test_gpu_parity import _form_for, _sync_walk_forced
from tests.tuned_contract import contract_rx, lib_stages, moved, to_8bit

pytestmark = pytest.mark.gpu

SCHEDULES = I.schedules()
P3L, REMOTE = "p3l-nexa2012", "unknown-remote1"


@pytest.fixture(scope="module")
def ok():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from ookiedokie_amd import build as okbuild
    okbuild.build()
    import ookiedokie_amd as okm
    okm.lib()
    return okm


# A kind of context: filter (a golden filter's name, a generic shape's name or None), device, threshold, sample format,
# batch (every run is three captures with a stride) and further Receiver arguments
Kind = collections.namedtuple("Kind", "filt devname thr fmt batch kw")


def kind(filt, devname=P3L, thr=I.THR, fmt="sc16q11", batch=False, **kw):
    return Kind(filt, devname, thr, fmt, batch, tuple(sorted(kw.items())))


# What a context is given in one run: device memory, geometry, the oracle's result per capture, the error list's order
Job = collections.namedtuple("Job", "name tensor n caps stride wants errs")

_tensors = {}       # uploaded captures, by (capture, format): each uploaded once, never written again
_jobs = {}


def _tensor(key, make):
    import torch
    if key not in _tensors:
        host = np.ascontiguousarray(make())
        t = torch.zeros(max(host.size, 16), dtype=torch.int8 if host.dtype == np.int8 else torch.int16, device="cuda")
        if host.size:
            t[:host.size] = torch.from_numpy(host.copy()).cuda()
        assert t.data_ptr() % 16 == 0
        torch.cuda.synchronize()            # (a context's own stream does not wait for the copy's)
        _tensors[key] = t
    return _tensors[key]


def _batch_members(name):
    """the three captures of a batched run given `name`: the capture itself and two others cut (or padded with zeros) to
    its length"""
    n = I.length(name)
    others = [x for x in ("g1_shifted", "g2", "g1") if x != name][:2]
    out = [np.array(I.capture(name))]
    for o in others:
        x = np.zeros(2 * n, np.int16)
        src = I.capture(o)[:2 * n]
        x[:src.size] = src
        out.append(x)
    return n, out


def _job(oracle, k, name):
    """the job `name` is for a context of kind k (built and uploaded once)"""
    key = (k.filt, k.devname, k.thr, k.fmt, k.batch, name)
    if key in _jobs:
        return _jobs[key]
    if k.batch:
        assert k.fmt == "sc16q11"
        n, members = _batch_members(name)
        stride = n + 8

        def host():
            h = np.zeros((len(members), 2 * stride), np.int16)
            for c, x in enumerate(members):
                h[c, :2 * n] = x
            return h.reshape(-1)
        wants = [I.oracle_result(oracle, "%s|%d" % (name, c), k.filt, k.devname, k.thr, iq=x) for c, x in enumerate(members)]
        job = Job(name, _tensor(("batch", name), host), n, len(members), stride, wants, None)
    elif k.fmt == "cs8":
        raw, wide = to_8bit(I.capture(name), "cs8")
        want = I.oracle_result(oracle, name + "@cs8", k.filt, k.devname, k.thr, iq=wide)
        job = Job(name, _tensor((name, "cs8"), lambda: raw), I.length(name), 1, I.length(name), [want], None)
    else:
        want = I.oracle_result(oracle, name, k.filt, k.devname, k.thr)
        job = Job(name, _tensor((name, "sc16q11"), lambda: I.capture(name)), I.length(name), 1, I.length(name), [want], None)
    _jobs[key] = job
    return job


def _filters(ok, oracle, filt):
    of = I.oracle_filter(oracle, filt)
    if filt is None:
        return None, None
    if filt in S.GENERIC_SHAPES:
        return ok.Filter.from_stages(S.stages(S.GENERIC_SHAPES[filt])), of
    return ok.Filter.load(golden_path("filters", filt)), of


EIGHT = {"FRONT_NO_FILTER": "FRONT_NO_FILTER_8", "FRONT_FIR1_MFMA": "FRONT_FIR1_MFMA_8", "FRONT_FIR2_MFMA": "FRONT_FIR2_MFMA_8"}


def _expected_form(ok, of, k):
    """the header's OOKD_FRONT_* value for the kind's filter and flags"""
    form = _form_for(ok, of, valu=bool(dict(k.kw).get("fir_valu")))
    if k.fmt == "cs8":
        name = next(nm for nm in EIGHT if getattr(ok, nm) == form)
        form = getattr(ok, EIGHT[name])
    return form


class _Ctx:
    """a context of some kind and what it holds in flight"""

    def __init__(self, ok, oracle, k, gate=None, max_samples=None, **extra):
        self.kind, self.oracle = k, oracle
        f, of = _filters(ok, oracle, k.filt)
        dec = of.total_decimation if of else 1
        self.device = ok.Device.load(golden_path("devices", k.devname), I.RATE // dec)
        self.filter = f
        kw = dict(k.kw)
        kw.update(extra)
        if k.batch:
            kw["max_captures"] = 3
        self.rx = ok.Receiver(f, self.device, max_samples=max_samples or I.length("g1"), threshold=k.thr,
                              sample_format=k.fmt, front_gate=gate, **kw)
        self.form = _expected_form(ok, of, k)
        assert self.rx.front_info()["form"] == self.form, k
        self.held = None

    def job(self, name):
        return name if isinstance(name, Job) else _job(self.oracle, self.kind, name)

    def submit(self, name):
        assert self.held is None
        j = self.job(name)
        self.rx.submit_device(j.tensor.data_ptr(), j.n, num_captures=j.caps, stride=j.stride)
        self.held = j

    def wait(self):
        self.rx.wait()

    def check(self, tag=""):
        """the run just waited for against the oracle's result for the capture this context was given"""
        j, self.held = self.held, None
        return _same(self.rx, j, self.form, (tag, j.name))

    def run(self, name, tag=""):
        self.submit(name)
        self.wait()
        return self.check(tag)

    def close(self):
        self.rx.close()


def _same(rx, j, form, tag):
    res = rx.result()
    st = res.stats
    assert st["front_form"] == form, tag
    assert st["decimated_samples"] == j.wants[0].decimated, tag
    got = [(int(c), int(s), bytes(p)) for c, s, p in zip(res.captures, res.msg_samples, res.payloads)]
    want = [(c, s, p) for c, w in enumerate(j.wants) for s, p in w.msgs]
    assert got == want, (tag, "messages")
    assert st["num_messages"] == len(want), tag
    want_errs = j.errs if j.errs is not None else [e for w in j.wants for e in w.errs]
    errs, nerr = rx.errors(len(want_errs) + 8)
    assert nerr == len(want_errs) == st["num_errors"], (tag, "errors", nerr, len(want_errs))
    assert [int(e) for e in errs] == list(want_errs), (tag, "error positions")
    assert st["num_edges"] == sum(len(w.edges) for w in j.wants), (tag, "num_edges")
    for c, w in enumerate(j.wants):
        e = rx.edges(c)                                     # (before the bits are read back, which cleans up)
        assert e.size == len(w.edges) and (e == np.array(w.edges, dtype=np.uint64)).all(), (tag, c, "edges")
        bits = rx.bits(c)
        assert bits.size == w.bits.size, (tag, c)
        diff = np.nonzero(bits != w.bits)[0]
        assert diff.size == 0, (tag, c, "first differing bits at %s" % diff[:5])
    return st


def _play(ctxs, sched, tag=""):
    """Plays a schedule: every capture uploaded (once) and the device synchronised before the first submit -- a
    context's own stream does not wait for the copy's --, every wait followed by the comparison."""
    import torch
    for step in sched:
        if step[0] == "submit":
            ctxs[step[1]].job(step[2])
    torch.cuda.synchronize()
    for i, step in enumerate(sched):
        c = ctxs[step[1]]
        if step[0] == "submit":
            c.submit(step[2])
        else:
            c.wait()
            c.check((tag, i))
    assert all(c.held is None for c in ctxs)


def _close(ctxs):
    for c in ctxs:
        c.close()


# ------------------------------------------------------------------------------- 1. schedules x forms ----

@pytest.fixture(scope="module")
def alike(ok, oracle):
    """four contexts alike per filter behind one gate, made once and reused by every schedule"""
    made = {}

    def get(filt):
        if filt not in made:
            gate = ok.FrontGate()
            made[filt] = (gate, [_Ctx(ok, oracle, kind(filt), gate) for _ in range(4)])
        return made[filt][1]
    yield get
    for gate, ctxs in made.values():
        _close(ctxs)
        gate.close()


@pytest.mark.parametrize("filt", ["fs32_fs4", "fs128_fs16_dec4"])
@pytest.mark.parametrize("sname", list(SCHEDULES))
def test_schedule_with_contexts_alike(ok, alike, sname, filt):
    K, sched = SCHEDULES[sname]
    ctxs = alike(filt)[:K]
    assert ctxs[0].form == (ok.FRONT_FIR1_MFMA if filt == "fs32_fs4" else ok.FRONT_FIR2_MFMA)
    _play(ctxs, sched, sname)


@pytest.mark.parametrize("filt", ["fs32_fs4", "fs128_fs16_dec4"])
def test_round_robin_without_a_gate(ok, oracle, filt):
    ctxs = [_Ctx(ok, oracle, kind(filt)) for _ in range(3)]
    _play(ctxs, I.round_robin(3), "no gate")
    _close(ctxs)


DIFFER = {
    "real": (kind("fs32_fs4", thr=0.1), kind("fs128_fs16_dec4", REMOTE, thr=0.05), kind(None)),
    # a generic-kernel shape (no wave tiles: the gate's event is recorded, it does not ride on a kernel), 8-bit samples
    # (the same bytes widened are what the oracle decodes), a batch of three with a stride
    "generic_cs8_batch": (kind("d3t40"), kind("fs32_fs4", fmt="cs8"), kind("fs128_fs16_dec4", batch=True)),
    "cs8_batch_real": (kind("fs128_fs16_dec4", fmt="cs8"), kind("fs32_fs4", batch=True), kind("fs32_fs4", thr=0.1)),
}


@pytest.mark.parametrize("trio", list(DIFFER))
def test_round_robin_with_contexts_that_differ(ok, oracle, trio):
    """one gate, three different front forms: each context against its own oracle result"""
    gate = ok.FrontGate()
    ctxs = [_Ctx(ok, oracle, k, gate) for k in DIFFER[trio]]
    want = {"real": [ok.FRONT_FIR1_MFMA, ok.FRONT_FIR2_MFMA, ok.FRONT_NO_FILTER],
            "generic_cs8_batch": [ok.FRONT_GENERIC, ok.FRONT_FIR1_MFMA_8, ok.FRONT_FIR2_MFMA],
            "cs8_batch_real": [ok.FRONT_FIR2_MFMA_8, ok.FRONT_FIR1_MFMA, ok.FRONT_FIR1_MFMA]}[trio]
    assert [c.form for c in ctxs] == want           # (every run's stats.front_form is held to it in _same)
    assert len(set(want)) >= 2
    _play(ctxs, I.round_robin(3), trio)
    _close(ctxs)
    gate.close()


def test_tuned_and_carrier_contexts_share_a_gate(ok):
    """a tuned context and a carrier context behind one gate, each against tests/tuned_contract.py: bits and edges
    per carrier"""
    import torch
    nu = 0.2
    f = ok.Filter.load(golden_path("filters", "fs32_fs4"))
    carriers = [(nu, I.THR), (0.0, 0.1)]
    caps = collections.OrderedDict()
    for nm, src, seed in (("a", I.capture("g1")[:2 * 600000], 61), ("b", I.capture("g2"), 62), ("c", I.capture("short"), 63)):
        iq = moved(src, nu, noise=I.NOISE, seed=seed)
        t = torch.from_numpy(iq.copy()).cuda()
        caps[nm] = (iq, t, [contract_rx(iq, lib_stages(f, cnu), cthr, I.SPB)[0] for cnu, cthr in carriers])
    assert all(caps[nm][2][0].any() for nm in "ab")
    torch.cuda.synchronize()
    gate = ok.FrontGate()
    n_max = max(v[0].size // 2 for v in caps.values())
    tuned = ok.Receiver(f, None, max_samples=n_max, tune=nu, front_gate=gate, edge_capacity=n_max + 64)
    multi = ok.Receiver(f, None, max_samples=n_max, carriers=carriers, front_gate=gate, edge_capacity=2 * n_max + 64)

    def check(rx, nm, form, ncar):
        assert rx.stats()["front_form"] == form, nm
        for k in range(ncar):
            bits = caps[nm][2][k]
            assert list(rx.edges(k)) == list(edges_of(bits)), (nm, k)
            got = rx.bits(k)
            assert got.size == bits.size and not np.nonzero(got != bits)[0].size, (nm, k)

    # round-robin over the two: the tuned context one capture ahead in the ring
    for step in range(4):
        a, b = "abc"[step % 3], "abc"[(step + 1) % 3]
        tuned.submit_device(caps[a][1].data_ptr(), caps[a][0].size // 2)
        multi.submit_device(caps[b][1].data_ptr(), caps[b][0].size // 2)
        first, second = ((multi, b, ok.FRONT_TUNED_MULTI, 2), (tuned, a, ok.FRONT_TUNED_FIR1, 1))[::(1 if step & 1 else -1)]
        for rx, nm, form, ncar in (first, second):
            rx.wait()
            check(rx, nm, form, ncar)
    tuned.close()
    multi.close()
    gate.close()


# -------------------------------------------------------- 2. every wait-side redo, neighbours in flight ----

def _redo_leg(make, special, taken, ordinary=("g1", "g2", "short"), fresh=False, then=None):
    """Three contexts behind one gate.  The middle one is given `special` while both others have ordinary runs in
    flight, one queued before it and one after; it is waited for first -- its redo runs on the stream beside them.  All
    three give their own capture's result, the one that took the path gives it again on two ordinary runs; then the
    roles move on by one context.  make() -> (gate, three contexts); fresh: new contexts for every rotation (the walk
    gives up on a context's FIRST run).  taken(stats): asserts that the path the leg is about was taken; then(name,
    stats): what an ordinary run behind it shows."""
    import torch
    gate, ctxs = None, None
    for r in range(3):
        if ctxs is None or fresh:
            if ctxs is not None:
                _close(ctxs)
                gate.close()
            gate, ctxs = make()
        a, m, b = (ctxs[(r + i) % 3] for i in range(3))
        sp = m.job(special(m))
        for c in ctxs:
            for nm in ordinary:
                c.job(nm)
        torch.cuda.synchronize()
        a.submit(ordinary[0])
        m.submit(sp)
        b.submit(ordinary[1])
        m.wait()
        taken(m.check(("special", r)))
        a.wait()
        a.check(("before", r))
        b.wait()
        b.check(("after", r))
        for nm in (ordinary[2], ordinary[0]):
            st = m.run(nm, ("then", r))
            if then:
                then(nm, st)
    _close(ctxs)
    gate.close()


def test_redo_walk_gives_up_with_neighbours_in_flight(ok, oracle):
    """`nosync` on a fresh context whose scan tries the walk from synchronising spans alone (sync_try 2): the walk gives
    up, ookd_rx_wait re-arms the device header and queues the scan again, composing.  A walk that held reports
    scan_entry_form 1; on a context's first run form 2 is reached through that redo only."""
    n = I.length("nosync")
    k = kind("fs32_fs4")

    def make():
        gate = ok.FrontGate()
        with _sync_walk_forced():
            return gate, [_Ctx(ok, oracle, k, gate, max_samples=n) for _ in range(3)]

    def taken(st):
        assert st["fsm_path"] == 1 and st["scan_entry_form"] == 2, st

    _redo_leg(make, lambda m: "nosync", taken, fresh=True)


def _nofilter_trio(ok, oracle, max_samples=None, **kw):
    def make():
        gate = ok.FrontGate()
        return gate, [_Ctx(ok, oracle, kind(None, **kw), gate, max_samples=max_samples or I.length("deep")) for _ in range(3)]
    return make


def test_redo_scan_refuses_with_neighbours_in_flight(ok, oracle):
    def taken(st):
        assert st["fsm_path"] == 3 and st["fsm_fallback_reason"] != 0, st

    _redo_leg(_nofilter_trio(ok, oracle), lambda m: "deep", taken)


def test_redo_batch_with_one_refused_capture_with_neighbours_in_flight(ok, oracle):
    """a batch of three whose middle capture the scan refuses: that one is redone in the round form inside wait; results
    per capture, and the error list in the header's order -- the refused capture's errors behind all the others'"""
    n, members = I.refused_batch()
    stride = n + 8

    def host():
        h = np.zeros((3, 2 * stride), np.int16)
        for c, x in enumerate(members):
            h[c, :2 * n] = x
        return h.reshape(-1)
    wants = [I.oracle_result(oracle, "refused_batch|%d" % c, None, P3L, I.THR, iq=x) for c, x in enumerate(members)]
    errs = list(wants[0].errs) + list(wants[2].errs) + list(wants[1].errs)
    job = Job("refused_batch", _tensor(("batch", "refused_batch"), host), n, 3, stride, wants, errs)
    assert sum(len(w.msgs) for w in wants) >= 15 and all(w.errs for w in wants)

    def taken(st):
        assert st["fsm_path"] == 3, st

    _redo_leg(_nofilter_trio(ok, oracle, max_samples=n, max_captures=3), lambda m: job, taken)


@pytest.mark.parametrize("refused", [True, False], ids=["refused", "kept"])
def test_redo_pipelined_run_with_neighbours_in_flight(ok, oracle, refused):
    """pipeline_chunk_samples = 4 buffers.  Over `deep` a chunk is refused and the capture is redone whole inside wait:
    the front end again, through the gate a second time, with the neighbours' runs queued behind it.  Over `g1_shifted`
    nothing is refused and the chunks' results stand."""
    def taken(st):
        if refused:
            assert st["fsm_fallback_reason"] != 0 and st["pipeline_chunks"] == 0 and st["fsm_path"] == 3, st
        else:
            assert st["fsm_fallback_reason"] == 0 and st["pipeline_chunks"] >= 2 and st["fsm_path"] == 1, st

    def then(nm, st):
        # (the context does pipeline: what `deep` reported is a pipelined run refused, not a run that never was one)
        assert nm != "g1" or (st["pipeline_chunks"] >= 2 and st["fsm_fallback_reason"] == 0), st

    _redo_leg(_nofilter_trio(ok, oracle, pipeline_chunk_samples=4 * I.SPB),
              lambda m: "deep" if refused else "g1_shifted", taken, then=then)


# ------------------------------------------------------------------------------ 3. overflow in flight ----

def test_edge_list_overflow_in_flight(ok, oracle):
    """The middle context's edge list is one entry too small for `dense_edges`: its wait fails with the capacity error,
    the neighbours' runs are exact, and the context is usable again (include/ookiedokie_amd.h at ookd_rx_wait: nothing
    in flight, the next submit is accepted): `short` decodes exactly, `dense_edges` fails again."""
    import torch
    gate = ok.FrontGate()
    k = kind(None)
    a, b = _Ctx(ok, oracle, k, gate), _Ctx(ok, oracle, k, gate)
    m = _Ctx(ok, oracle, k, gate, edge_capacity=I.DENSE_EDGES - 1)
    for nm in ("g1", "g2", "short", "dense_edges"):
        a.job(nm)
    torch.cuda.synchronize()
    for rnd in range(2):
        a.submit("g1")
        m.submit("dense_edges")
        b.submit("g2")
        with pytest.raises(ok.OokdError) as e:
            m.wait()
        assert "edge list overflow" in str(e.value), str(e.value)
        m.held = None
        with pytest.raises(ok.OokdError) as e:
            m.wait()                                # the failed wait cleared the run: nothing is in flight
        assert "nothing was submitted" in str(e.value)
        if rnd == 0:
            m.run("short", "after the failed wait, neighbours still in flight")
        a.wait()
        a.check("before")
        b.wait()
        b.check("after")
        m.run("short", "after the failed wait")
    # the same capture fits a list that holds it
    fits = _Ctx(ok, oracle, k, gate, edge_capacity=I.DENSE_EDGES)
    fits.run("dense_edges", "fits")
    _close([a, b, m, fits])
    gate.close()


# ----------------------------------------------------------------------------------- 4. gate lifetime ----

@pytest.mark.parametrize("filt", ["fs32_fs4", "d3t40"])
def test_gate_outlives_its_contexts_events(ok, oracle, filt):
    """The gate remembers the stop event of the last front end queued; a context that is destroyed takes its event with
    it and must make the gate forget it.  A closes while its event is the gate's last, B (made before) and C (made
    after) then run through the gate; all close, the gate goes, a new gate and new contexts run.  (fs32_fs4: the event
    rides on the kernel; d3t40: it is recorded.)"""
    import torch
    k = kind(filt)
    gate = ok.FrontGate()
    a, b = _Ctx(ok, oracle, k, gate), _Ctx(ok, oracle, k, gate)
    for nm in ("g1", "g2", "g1_shifted", "short"):
        a.job(nm)
    torch.cuda.synchronize()
    b.run("short", "b first")
    a.run("g1", "a")
    a.close()                                       # A's event is the gate's last
    b.run("g2", "b after a is gone")
    c = _Ctx(ok, oracle, k, gate)
    c.run("g1_shifted", "c")
    b.submit("g1")
    c.submit("g2")
    c.wait()
    c.check("c in flight")
    b.wait()
    b.check("b in flight")
    c.close()                                       # C's event was overtaken by B's: not the gate's last
    b.run("short", "b alone")
    b.close()
    gate.close()
    gate = ok.FrontGate()
    ctxs = [_Ctx(ok, oracle, k, gate) for _ in range(2)]
    _play(ctxs, I.fifo_lagged(ncaptures=4), "new gate")
    _close(ctxs)
    gate.close()
    assert ok.last_error() == ""


# -------------------------------------------------------------------------------- 5. two host threads ----

def test_two_host_threads_share_a_gate(ok, oracle):
    """one context per host thread (the header allows it; the gate has a mutex): six submit/wait steps each, over
    captures the other thread never holds, started together"""
    import torch
    gate = ok.FrontGate()
    ctxs = [_Ctx(ok, oracle, kind("fs32_fs4"), gate), _Ctx(ok, oracle, kind("fs128_fs16_dec4"), gate)]
    plans = [("g1", "short", "one", "g1", "short", "one"), ("g1_shifted", "g2", "silence", "g2", "g1_shifted", "empty")]
    assert not set(plans[0]) & set(plans[1])
    jobs = [[c.job(nm) for nm in plan] for c, plan in zip(ctxs, plans)]
    torch.cuda.synchronize()
    barrier = threading.Barrier(2)
    out = [[], []]
    failed = [None, None]

    def drive(i):
        try:
            rx = ctxs[i].rx
            barrier.wait(timeout=30)
            for j in jobs[i]:
                rx.submit_device(j.tensor.data_ptr(), j.n, num_captures=j.caps, stride=j.stride)
                rx.wait()
                res = rx.result()
                errs, nerr = rx.errors()
                out[i].append((res, [int(e) for e in errs], nerr, rx.edges(), rx.bits(), ok.last_error()))
        except BaseException as e:                  # reported by the main thread
            failed[i] = e

    threads = [threading.Thread(target=drive, args=(i,)) for i in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=120)
    assert not any(t.is_alive() for t in threads), "a thread did not finish"
    assert failed == [None, None], failed
    for i in range(2):
        assert len(out[i]) == 6
        for j, (res, errs, nerr, edges, bits, last) in zip(jobs[i], out[i]):
            w = j.wants[0]
            tag = (i, j.name)
            assert last == "", tag
            assert res.stats["front_form"] == ctxs[i].form, tag
            assert [(int(s), bytes(p)) for s, p in zip(res.msg_samples, res.payloads)] == list(w.msgs), tag
            assert not res.captures.any(), tag
            assert nerr == len(w.errs) and errs == list(w.errs), tag
            assert res.stats["num_edges"] == len(w.edges) and [int(e) for e in edges] == list(w.edges), tag
            assert bits.size == w.bits.size and (bits == w.bits).all(), tag
    _close(ctxs)
    gate.close()


# ---------------------------------------------------------------------------------- 6. caller's stream ----

@pytest.mark.parametrize("own", [False, True], ids=["callers_stream", "own_stream_synchronised"])
def test_run_reads_the_capture_in_the_streams_order(ok, oracle, own):
    """ookd_rx_config.stream: a run reads the capture in the stream's order.  Two contexts on one torch stream; the
    producer -- a copy from pinned memory on that stream -- is followed by the submit with no synchronisation in
    between, four different captures into ONE device buffer, waiting only before the buffer is overwritten.  Control:
    contexts on their own (non-blocking) streams and a synchronize() behind the copy."""
    import torch
    k = kind("fs32_fs4")
    s = torch.cuda.Stream()
    names = ("g1", "g1_shifted", "g2", "short")
    n_max = max(I.length(nm) for nm in names)
    buf = torch.zeros(2 * n_max, dtype=torch.int16, device="cuda")
    pinned = {nm: torch.from_numpy(np.array(I.capture(nm))).pin_memory() for nm in names}
    jobs = {nm: _job(oracle, k, nm) for nm in names}
    torch.cuda.synchronize()
    kw = {} if own else dict(stream=s.cuda_stream)
    ctxs = [_Ctx(ok, oracle, k, None, **kw) for _ in range(2)]
    prev = None
    for i, nm in enumerate(names + names[:2]):
        c = ctxs[i & 1]
        if prev is not None:
            prev.wait()                             # the run that reads the buffer, before it is overwritten
            prev.check(("stream", i - 1))
        with torch.cuda.stream(s):
            buf[:2 * I.length(nm)].copy_(pinned[nm], non_blocking=True)
        if own:
            torch.cuda.synchronize()
        c.submit(jobs[nm]._replace(tensor=buf))
        prev = c
    prev.wait()
    prev.check("last")
    _close(ctxs)


# ------------------------------------------------------------------------------------ 7. split launches ----

SPLIT = {
    "dec4_mfma": kind("fs128_fs16_dec4"),
    "dec4_valu": kind("fs128_fs16_dec4", fir_valu=True),
    "fs32_batch": kind("fs32_fs4", batch=True),
    "dec4_batch": kind("fs128_fs16_dec4", batch=True),
    "fs32_cs8": kind("fs32_fs4", fmt="cs8"),
    "dec4_cs8": kind("fs128_fs16_dec4", fmt="cs8"),
}


def _split_env(monkeypatch, on):
    if on:
        monkeypatch.setenv("OOKD_DEVELOPER", "1")
        monkeypatch.setenv("OOKD_FRONT_LAUNCH_LOG2", "16")
    else:
        monkeypatch.delenv("OOKD_FRONT_LAUNCH_LOG2", raising=False)


@pytest.mark.parametrize("which", list(SPLIT))
def test_split_launches(ok, oracle, monkeypatch, which):
    """OOKD_FRONT_LAUNCH_LOG2=16: launches of 65 536 outputs (divided among the captures of a batch: with G1's length a
    launch ends inside every capture, never on a capture's end).  Bits, edges, messages and the quiet / total wave
    counts are those of the one-launch context and the oracle's."""
    import torch
    k = SPLIT[which]
    runs = []
    for split in (False, True):
        _split_env(monkeypatch, split)
        c = _Ctx(ok, oracle, k, None, count_quiet=True)
        _split_env(monkeypatch, False)
        c.job("g1")
        torch.cuda.synchronize()
        for nm in ("g1", "g2", "g1"):
            st = c.run(nm, (which, split))
            if not split:
                assert st["front_launches"] == 1, (which, nm)
        assert st["front_launches"] > 1 or not split, (which, st["front_launches"])          # (the last run: g1)
        runs.append((st["quiet_waves"], st["total_waves"], [list(c.rx.edges(i)) for i in range(3 if k.batch else 1)]))
        print("split launches", which, split, "launches", st["front_launches"], "quiet", st["quiet_waves"], "of", st["total_waves"])
        c.close()
    assert runs[0] == runs[1]
    assert 0 < runs[1][0] < runs[1][1]


def test_round_robin_with_split_launches(ok, oracle, monkeypatch):
    """every front end of the schedule in several launches: a neighbour's chain gets onto the chip between them"""
    gate = ok.FrontGate()
    _split_env(monkeypatch, True)
    ctxs = [_Ctx(ok, oracle, kind("fs128_fs16_dec4"), gate) for _ in range(3)]
    _split_env(monkeypatch, False)
    _play(ctxs, I.round_robin(3), "split")
    assert ctxs[0].run("g1")["front_launches"] > 1
    _close(ctxs)
    gate.close()


# ------------------------------------------------------------- 8. a post-run pass beside a neighbour ----

@pytest.mark.parametrize("filt", ["fs32_fs4", "fs128_fs16_dec4"])
def test_pulse_hist_while_a_neighbour_is_in_flight(ok, oracle, filt):
    import torch
    gate = ok.FrontGate()
    a, b = (_Ctx(ok, oracle, kind(filt), gate) for _ in range(2))
    for nm in ("g1", "g1_shifted", "g2"):
        a.job(nm)
    torch.cuda.synchronize()
    for na, nb in (("g1", "g1_shifted"), ("g2", "g1")):
        a.submit(na)
        b.submit(nb)
        a.wait()
        w = a.held.wants[0]
        P.assert_same_hist(a.rx.pulse_hist(0), P.hist_of(w.edges, w.decimated), (filt, na))    # B's run is in flight
        a.check("a")
        b.wait()
        b.check("b")
    _close([a, b])
    gate.close()
