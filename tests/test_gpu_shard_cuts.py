"""The shard hand-over (ookd_rx_shard_begin / ookd_rx_shard_refine) at EVERY cut of the designed streams of
tests/shard_cut_inputs.py: what a shard hands on is what the sequential machine holds at that sample -- state, bits
collected, payload, the count k, prev_bit, byte for byte --, what a shard does with an incoming state is what the
sequential machine does from there -- messages, payloads, every error position, bits, edges --, refinement is a pure
function of (shard, incoming state), and a shard's front end sees its own samples and its halo and nothing else.
Everything is exact against the CPU oracle; what the inputs hold is checked without a GPU in test_shard_cuts_host.py.

fsm_path per shard (1 = the scan kept it, 3 = it refused and the round form decoded it, 2 = round form from the start)
is printed and recorded; what is asserted of it is the table of DESIGN 6.1."""
import bisect
import collections

import numpy as np
import pytest

from tests import dense_devices as dd
from tests import shard_cut_inputs as sci
from tests.helpers import edges_of
from tests.test_gpu_parity import _sync_walk_forced

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ok():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from ookiedokie_amd import build as okbuild
    okbuild.build()
    import ookiedokie_amd as okm
    okm.lib()
    return okm


# (name, Receiver arguments, walk from synchronising spans forced) -- named as test_gpu_dense_results.LEGS; the rounds
# leg in segments of two buffers: a shard holds several, a refinement travels across them
LEGS = (("tables", dict(), False),
        ("sims", dict(scan_sims=True), False),
        ("composed", dict(scan_tables=True), False),
        ("walk", dict(), True),
        ("rounds", dict(fsm_rounds=True, quiet_skip=False, segment_buffers=2), False))
LEG_NAMES = tuple(x[0] for x in LEGS)


class _Ctx:
    """a case on the GPU: the stream uploaded once, the oracle's whole-capture result and its carried states"""
    _made = {}

    def __init__(self, ok, oracle, name):
        import torch
        self.case = c = sci.case(name)
        self.fsm = sci.oracle_device(oracle, c)
        self.n = c.stream.size
        iq = dd.iq_of(c.stream)
        self.want = oracle.rx(iq, None, dd.THR, self.fsm, c.spb, want_bits=True, msg_cap=1 << 12)
        assert self.want.decimated == self.n and (self.want.bits == c.stream).all()
        self.msgs = [(int(s), bytes(p)) for s, p in zip(self.want.msg_samples, self.want.payloads)]
        self.msg_at = [m[0] for m in self.msgs]
        self.errs = [int(e) for e in self.want.err_samples]
        self.held = sci.carried(oracle, c)
        self.edges = edges_of(c.stream)
        self.err_cap = self.n // c.spb + 8      # (at most one error per buffer: the rest of it is dropped)
        self.dev_t = torch.from_numpy(iq.copy()).cuda()
        torch.cuda.synchronize()            # (a context's stream does not wait for the copy's)
        self.ptr = self.dev_t.data_ptr()

    @classmethod
    def of(cls, ok, oracle, name):
        if name not in cls._made:
            cls._made[name] = cls(ok, oracle, name)
        return cls._made[name]

    def receivers(self, ok, leg, count):
        kw, walk = next((kw, walk) for nm, kw, walk in LEGS if nm == leg)
        d = sci.ok_device(ok, self.case)
        M = len(self.msgs)
        with _sync_walk_forced(walk):
            rxs = [ok.Receiver(None, d, max_samples=self.n, threshold=dd.THR, samples_per_buffer=self.case.spb,
                               message_slots=M + 2, message_capacity=M + 64, **kw) for _ in range(count)]
        assert all(rx.halo_samples == 0 for rx in rxs)
        return d, rxs

    # ---- the oracle's slice [lo, hi) of the whole capture, in the shard's own coordinates
    def msgs_in(self, lo, hi):
        a, b = bisect.bisect_left(self.msg_at, lo), bisect.bisect_left(self.msg_at, hi)
        return [(s - lo, p) for s, p in self.msgs[a:b]]

    def errs_in(self, lo, hi):
        a, b = bisect.bisect_left(self.errs, lo), bisect.bisect_left(self.errs, hi)
        return [e - lo for e in self.errs[a:b]]

    def edges_in(self, lo, hi):
        """edges of the slice under the documented convention: the sample in front of a shard counts as 0"""
        a, b = bisect.bisect_left(self.edges, lo), bisect.bisect_left(self.edges, hi)
        inner = b - a - (1 if a < b and self.edges[a] == lo else 0)
        return inner + int(self.case.stream[lo]) if hi > lo else 0


def expected_state(ok, fsm, h):
    """The ookd_fsm_state of a carried state of the oracle's, by the rules of include/ookiedokie_amd.h: state, num_bits,
    prev_bit and payload as the sequential machine holds them (in the reset state still those of the message before);
    k the count of increments where the state looks at it and 0 where it cannot matter; every other byte 0."""
    s = ok.FsmState()
    s.state, s.num_bits, s.prev_bit = h.state, h.num_bits, h.prev_bit
    s.k = h.k if sci.k_matters(fsm, h.state) else 0
    for i, b in enumerate(h.payload):
        s.payload[i] = b
    return s


def _show(s):
    return "state %d bits %d k %d prev %d reserved %d payload %s" % (s.state, s.num_bits, s.k, s.prev_bit, s.reserved,
                                                                    bytes(s.payload).rstrip(b"\0").hex())


class _Bad(list):
    """mismatches of a sweep, each with (case, leg, cut): collected so that a failing id shows all of them by kind --
    the id fails if there is a single one"""

    def __init__(self, name, leg):
        super().__init__()
        self.tag = (name, leg)

    def check(self, cond, cut, what, got=None, want=None):
        if not cond:
            self.append((self.tag + (cut,), what, got, want))

    def report(self):
        kinds = collections.Counter(b[1] for b in self)
        lines = ["%d mismatches: %s" % (len(self), dict(kinds))]
        seen = collections.Counter()
        for tag, what, got, want in self:
            seen[what] += 1
            if seen[what] <= 4:
                lines.append("%s %s\n    got  %s\n    want %s" % (tag, what, got, want))
        return "\n".join(lines)


def _state_checks(bad, cut, what, fsm, got, h, ok):
    """the outgoing state `got` against the oracle's carried state h, field by field, then byte by byte"""
    exp = expected_state(ok, fsm, h)
    bad.check((got.state, got.prev_bit) == (exp.state, exp.prev_bit), cut, what + ": state / prev_bit", _show(got), _show(exp))
    nbytes = (max(h.num_bits, 0) + 7) // 8
    if h.state != 0:
        below = np.unpackbits(np.frombuffer(bytes(got.payload), np.uint8), bitorder="little")[:h.num_bits]
        want = np.unpackbits(np.frombuffer(h.payload.ljust(nbytes + 1, b"\0"), np.uint8), bitorder="little")[:h.num_bits]
        bad.check(got.num_bits == h.num_bits and (below == want).all(), cut, what + ": num_bits / payload",
                  _show(got), _show(exp))
    if sci.k_matters(fsm, h.state):
        bad.check(got.k == h.k, cut, what + ": k where it matters", _show(got), _show(exp))
    else:
        bad.check(got.k == 0, cut, what + ": k where it cannot matter is 0", _show(got), _show(exp))
    bad.check(got.reserved == 0, cut, what + ": reserved", _show(got), _show(exp))
    bad.check(got.key() == exp.key(), cut, what + ": bytes", _show(got), _show(exp))


def _result_checks(bad, cut, what, ctx, rx, res, lo, hi):
    """messages, payloads, every error position, bits and num_edges of one shard against the oracle's slice [lo, hi)"""
    got = [(int(s), bytes(p)) for s, p in zip(res.msg_samples, res.payloads)]
    bad.check(got == ctx.msgs_in(lo, hi), cut, what + ": messages", got[:4], ctx.msgs_in(lo, hi)[:4])
    want_e = ctx.errs_in(lo, hi)
    errs, nerr = rx.errors(len(want_e) + 8)
    bad.check(nerr == len(want_e) == res.stats["num_errors"] and [int(e) for e in errs] == want_e, cut, what + ": errors",
              (nerr, res.stats["num_errors"], [int(e) for e in errs][:6]), (len(want_e), want_e[:6]))
    bad.check(res.stats["decimated_samples"] == hi - lo, cut, what + ": decimated_samples")
    if hi > lo:
        b = rx.bits()
        bad.check(b.size == hi - lo and (b == ctx.case.stream[lo:hi]).all(), cut, what + ": bits")
    bad.check(res.stats["num_edges"] == ctx.edges_in(lo, hi), cut, what + ": num_edges", res.stats["num_edges"], ctx.edges_in(lo, hi))
    return got, [int(e) for e in errs]


def _expected_path(c, leg, lo, hi, first_shard, kind):
    """fsm_path of the shard [lo, hi) on a scan leg -- the first shard of a capture, or one begun at LOW level from the
    carried state of class `kind` -- as the table of DESIGN 6.1 states it; None where the table leaves it open"""
    if not c.stuck:
        return 1 if c.scan == "keeps" else None
    if not sci.holds_any(c, lo, hi):
        return 1                    # no edge on which nothing fires: every form of the scan keeps it
    whole = sci.holds_whole(c, lo, hi)
    if leg == "sims":
        return 3 if whole else None     # the simulating form has no stuck codes
    if c.stuck == "deep":
        return 3 if whole else None     # seven pulses: deeper than the stuck codes hold
    if c.scan == "keeps" or first_shard:
        return 1                    # one or two pulses, the shipped device's glitches: held as stuck codes
    # begun in front of the stretch from the reset or the idle state: held; begun inside that very bit gap (`off`, a
    # carried count): the first span, simulated from the count, ends on an edge on which nothing fires -- left open
    return 1 if kind in ("reset", "quiet") else None


def _path_check(bad, cut, what, want, res):
    got, reason = res.stats["fsm_path"], res.stats["fsm_fallback_reason"]
    if want is not None:
        bad.check(got == want and (want != 3 or reason != 0), cut, "fsm_path: " + what, (got, reason), want)


SWEEP_IDS = [(name, leg) for name in sci.CASES for leg in LEG_NAMES]


@pytest.mark.parametrize("name,leg", SWEEP_IDS, ids=["%s-%s" % x for x in SWEEP_IDS])
def test_two_shards_at_every_cut(ok, oracle, name, leg, record_property):
    """Shard 0 = [0, c), shard 1 = [c, n) for every multiple c of samples_per_buffer.  Both begin from the reset state,
    shard 1 is refined with shard 0's outgoing state; shard 1 is also begun from the oracle's state at c directly (the
    chain): same results, same outgoing bytes.  At five cuts the refinement is repeated with the true and the reset
    state in turn: a pure function of the incoming state."""
    ctx = _Ctx.of(ok, oracle, name)
    c, fsm, n, held = ctx.case, ctx.fsm, ctx.n, ctx.held
    d, (rx0, rx1, rx2) = ctx.receivers(ok, leg, 3)
    bad = _Bad(name, leg)
    scan_leg = leg != "rounds" and c.scan != "outside"
    paths = {"shard0": collections.Counter(), "refined": collections.Counter(), "chain": collections.Counter()}
    chain_by_class = collections.defaultdict(collections.Counter)
    reasons = collections.Counter()
    pure_at = set(sci.purity_cuts(oracle, c))
    swept, low_refused, asserted = [], [], 0
    for cut in sci.cuts(c):
        h = held[cut]
        cls = sci.carried_class(fsm, h)
        # ---- shard 0 and what it hands on
        r0, s0 = rx0.shard_begin(ctx.ptr, cut, None, False, None)
        _result_checks(bad, cut, "shard 0", ctx, rx0, r0, 0, cut)
        _state_checks(bad, cut, "handed on", fsm, s0, h, ok)
        # ---- shard 1: speculative pass, then the refinement with what shard 0 handed on
        rx1.shard_begin(ctx.ptr + 4 * cut, n - cut, None, True, None)
        r1, s1 = rx1.shard_refine(s0)
        m1, e1 = _result_checks(bad, cut, "shard 1 refined", ctx, rx1, r1, cut, n)
        _state_checks(bad, cut, "shard 1 refined, at the end", fsm, s1, held[n], ok)
        # ---- the chain: shard 1 begun from the oracle's state
        r2, s2 = rx2.shard_begin(ctx.ptr + 4 * cut, n - cut, None, True, expected_state(ok, fsm, h))
        m2, e2 = _result_checks(bad, cut, "shard 1 chained", ctx, rx2, r2, cut, n)
        bad.check((m2, e2) == (m1, e1), cut, "chained != refined: results")
        bad.check(s2.key() == s1.key(), cut, "chained != refined: outgoing bytes", _show(s2), _show(s1))
        # ---- which path ran
        p0, p1, p2 = r0.stats["fsm_path"], r1.stats["fsm_path"], r2.stats["fsm_path"]
        paths["shard0"][p0] += 1
        paths["refined"][p1] += 1
        paths["chain"][p2] += 1
        chain_by_class[cls[:2]][p2] += 1
        if scan_leg and h.prev_bit == 0 and p2 != 1:
            low_refused.append(cut)
        for r in (r0, r1, r2):
            if r.stats["fsm_fallback_reason"]:
                reasons[r.stats["fsm_fallback_reason"]] += 1
        if not scan_leg:
            bad.check((p0, p1, p2) == (2, 2, 2), cut, "fsm_path: round form everywhere", (p0, p1, p2), (2, 2, 2))
        else:
            _path_check(bad, cut, "shard 0", _expected_path(c, leg, 0, cut, True, "reset"), r0)
            if h.prev_bit == 0:
                _path_check(bad, cut, "chained shard 1 from %s, prev_bit 0" % cls[0],
                            _expected_path(c, leg, cut, n, False, cls[0]), r2)
                asserted += _expected_path(c, leg, cut, n, False, cls[0]) is not None
            asserted += _expected_path(c, leg, 0, cut, True, "reset") is not None
        # ---- refinement is a pure function of the incoming state
        if cut in pure_at:
            a, b = s0, ok.FsmState()
            runs = []
            for state in (a, b, a, a):
                r, s = rx1.shard_refine(state)
                errs, nerr = rx1.errors(ctx.err_cap)
                runs.append((s.key(), [(int(x), bytes(p)) for x, p in zip(r.msg_samples, r.payloads)], [int(e) for e in errs], nerr))
            bad.check(runs[0] == runs[2] == runs[3], cut, "refine(a), refine(b), refine(a), refine(a): a's differ")
            bad.check(runs[0] == (s1.key(), m1, e1, len(e1)), cut, "refine(a) again != the first refinement")
            want_b = oracle.rx(dd.iq_of(c.stream[cut:]), None, dd.THR, fsm, c.spb)
            bad.check(runs[1][1] == [(int(x), bytes(p)) for x, p in zip(want_b.msg_samples, want_b.payloads)] and
                      runs[1][2] == [int(e) for e in want_b.err_samples], cut, "refine(reset state) != the shard as a capture")
        swept.append(cut)
    for rx in (rx0, rx1, rx2):
        rx.close()
    d.close()
    line = ("shard-cuts %s leg %s: cuts %d, fsm_path shard0 %s refined %s chain %s, chain by (class, prev_bit) %s, "
            "chained from prev_bit 0 outside the scan at %s, fsm_path asserted of %d shards, fallback reasons %s"
            % (name, leg, len(swept), dict(paths["shard0"]), dict(paths["refined"]), dict(paths["chain"]),
               {k: dict(v) for k, v in sorted(chain_by_class.items())}, low_refused[:12], asserted, dict(reasons)))
    print(line)
    record_property("shard_cuts", line)
    assert swept == sci.cuts(c)             # no cut is left out
    assert asserted >= len(swept) or not scan_leg       # fsm_path is pinned for at least as many shards as there are cuts
    assert not bad, bad.report()


MULTI_IDS = [(name, leg) for name in sci.MULTI_SHARD_CASES for leg in LEG_NAMES]


@pytest.mark.parametrize("name,leg", MULTI_IDS, ids=["%s-%s" % x for x in MULTI_IDS])
def test_several_uneven_shards(ok, oracle, name, leg, record_property):
    """Three to five shards with uneven bounds, one of a single alignment unit and an empty one in the middle (it passes
    the state through), iterated as the ranks do (ookiedokie_amd/distributed.py: every shard begins from the reset
    state; round by round each one whose predecessor's outgoing bytes changed refines): closed after at most as many
    rounds as there are shards, and then every shard's results and outgoing state are the oracle's."""
    ctx = _Ctx.of(ok, oracle, name)
    c, fsm, held = ctx.case, ctx.fsm, ctx.held
    layouts = sci.shard_layouts(oracle, c)
    d, rxs = ctx.receivers(ok, leg, max(len(b) - 1 for b in layouts))
    bad = _Bad(name, leg)
    lines = []
    for bounds in layouts:
        nsh = len(bounds) - 1
        tag = tuple(bounds)
        res, outs, ins = [None] * nsh, [None] * nsh, [None] * nsh
        for r in range(nsh):
            lo, hi = bounds[r], bounds[r + 1]
            res[r], outs[r] = rxs[r].shard_begin(ctx.ptr + 4 * lo, hi - lo, None, r == nsh - 1, None)
        rounds, prev_all = 0, None
        for _ in range(nsh + 2):
            all_states = [o.key() for o in outs]
            if prev_all is not None:
                if all_states == prev_all:
                    break
                rounds += 1
            prev_all = all_states
            for r in range(1, nsh):
                if ins[r] != all_states[r - 1]:
                    ins[r] = all_states[r - 1]
                    res[r], outs[r] = rxs[r].shard_refine(ok.Receiver.state_from_bytes(ins[r]))
        else:
            bad.check(False, tag, "the carried states did not settle")
        bad.check(rounds <= nsh, tag, "rounds", rounds, nsh)
        msgs, errs = [], []
        for r in range(nsh):
            lo, hi = bounds[r], bounds[r + 1]
            m, e = _result_checks(bad, tag, "shard %d" % r, ctx, rxs[r], res[r], lo, hi)
            msgs += [(s + lo, p) for s, p in m]
            errs += [x + lo for x in e]
            if hi > 0:
                _state_checks(bad, tag, "shard %d hands on" % r, fsm, outs[r], held[hi], ok)
        bad.check(msgs == ctx.msgs and errs == ctx.errs, tag, "all shards together")
        # which path ran: the round form everywhere on the rounds leg; the first shard as DESIGN 6.1 states (the others
        # began from the reset state in the middle of a message: recorded).  An empty shard ran nothing: 0
        for r in range(nsh):
            if bounds[r + 1] == bounds[r]:
                bad.check(res[r].stats["fsm_path"] == 0, tag, "fsm_path: empty shard %d" % r, res[r].stats["fsm_path"], 0)
            elif leg == "rounds" or c.scan == "outside":
                bad.check(res[r].stats["fsm_path"] == 2, tag, "fsm_path: shard %d" % r, res[r].stats["fsm_path"], 2)
        if leg != "rounds" and c.scan != "outside":
            _path_check(bad, tag, "shard 0", _expected_path(c, leg, 0, bounds[1], True, "reset"), res[0])
        lines.append("bounds %s rounds %d fsm_path %s" % (bounds, rounds, [x.stats["fsm_path"] for x in res]))
    for rx in rxs:
        rx.close()
    d.close()
    line = "shard-cuts several shards %s leg %s: %s" % (name, leg, "; ".join(lines))
    print(line)
    record_property("shard_cuts", line)
    assert not bad, bad.report()


# ------------------------------------------------------------------- narrow shards through the front ends ----
# The sweeps above run unfiltered and hand every shard a pointer into the middle of the whole capture: a front end that
# read in front of a shard's first sample instead of its halo, or past its last, would read the right samples.  Here
# every shard lies in an allocation of its own between two pads of loud samples (tests/shard_cut_inputs.loud_pad), and
# its length is no multiple of a 64-bit word or of a tile.

# (name, filter, Receiver arguments, samples per buffer as a multiple of the total decimation D, expected form)
FRONT_LEGS = (
    ("none", None, dict(), 200, "FRONT_NO_FILTER"),
    ("fs32_fs4", "fs32_fs4", dict(), 1000, "FRONT_FIR1_MFMA"),
    ("fs32_fs4-valu", "fs32_fs4", dict(fir_valu=True), 1000, "FRONT_FIR1_VALU"),
    ("fs32_fs4-exact", "fs32_fs4", dict(exact_fir=True), 1000, "FRONT_FIR1_VALU_EXACT"),
    ("dec4", "fs128_fs16_dec4", dict(), 200, "FRONT_FIR2_MFMA"),
    ("dec4-valu", "fs128_fs16_dec4", dict(fir_valu=True), 200, "FRONT_FIR2_VALU"),
    ("unity16", "unity16", dict(), 1000, "FRONT_FIR1_MFMA"),
    ("d2d1d2", "shape:d2d1d2", dict(), 200, "FRONT_GENERIC"),        # three stages: the generic kernel
    ("fs32_fs4-cs8", "fs32_fs4", dict(sample_format="cs8"), 1000, "FRONT_FIR1_MFMA_8"),
    ("dec4-cs8", "fs128_fs16_dec4", dict(sample_format="cs8"), 200, "FRONT_FIR2_MFMA_8"),
    # the floats of a shard's first and last outputs against the whole capture's, one 1-stage and one 2-stage leg
    ("fs32_fs4-floats", "fs32_fs4", dict(keep_fir=True), 1000, "FRONT_FIR1_MFMA"),
    ("dec4-valu-floats", "fs128_fs16_dec4", dict(fir_valu=True, keep_fir=True), 200, "FRONT_FIR2_VALU"),
)
NEAR = 96           # outputs at either end of a shard whose floats are compared (beyond the longest filter's reach)


def _front_filter(ok, oracle, spec):
    from tests import front_shapes_inputs as fsi
    from tests.helpers import golden_path
    if spec is None:
        return None, None
    if spec.startswith("shape:"):
        st = fsi.stages(fsi.GENERIC_SHAPES[spec[6:]])
        return ok.Filter.from_stages([(d, [float(t) for t in h]) for d, h in st]), oracle.make_fir(st)
    return ok.Filter.load(golden_path("filters", spec)), oracle.load_filter_json(golden_path("filters", spec))


def _own_tensor(samples, eight_bit):
    """the shard's samples between two loud pads in one device allocation; (tensor, byte offset of the first sample)"""
    import torch
    host = np.concatenate([sci.loud_pad(eight_bit), samples, sci.loud_pad(eight_bit, behind=True)])
    t = torch.from_numpy(host).cuda()
    return t, sci.loud_pad(eight_bit).nbytes


@pytest.mark.parametrize("leg", FRONT_LEGS, ids=[x[0] for x in FRONT_LEGS])
def test_narrow_shards_through_the_front_end(ok, oracle, leg, record_property):
    import torch
    name, spec, kw, per, form = leg
    eight = kw.get("sample_format") == "cs8"
    f, of = _front_filter(ok, oracle, spec)
    dec = of.total_decimation if of else 1
    gain = float(np.prod([of.stage_taps(s).astype(np.float64).sum() for s in range(of.num_stages)])) if of else 1.0
    thr = sci.front_threshold(gain)
    spb = per * dec
    dev = dd.burst(8)
    d, od = dd.ok_device(ok, dev), dd.fsm_desc(oracle, dev)
    x = sci.front_capture(dec, eight)               # what the context reads
    wide = sci.front_capture(dec)                   # ... and the same capture as SC16Q11, for the oracle
    n = wide.size // 2
    want = oracle.rx(wide, of, thr, od, spb, want_bits=True)
    msgs = [(int(s), bytes(p)) for s, p in zip(want.msg_samples, want.payloads)]
    errs = [int(e) for e in want.err_samples]
    assert want.decimated == sci.FRONT_OUTPUTS and len(msgs) == 12
    rx0, rx1 = (ok.Receiver(f, d, max_samples=n, threshold=thr, samples_per_buffer=spb, **kw) for _ in range(2))
    H = int(rx0.halo_samples)
    assert rx0.front_info()["form"] == getattr(ok, form), (name, rx0.front_info()["form"])
    whole_fir = None
    if kw.get("keep_fir"):
        # the whole capture through the same form, its floats kept
        whole = ok.Receiver(f, d, max_samples=n, threshold=thr, samples_per_buffer=spb, **kw)
        res = whole.rx(x)
        assert res.stats["front_form"] == getattr(ok, form) and (whole.bits() == want.bits).all()
        whole_fir = whole.fir_output().astype(np.float64)
        info = whole.front_info()
        # (each run is within half of the bound of the exact value -- test_error_bound_margin --: two runs of one
        #  form differ by no more than the bound itself)
        err = info["err_valu"] if kw.get("fir_valu") else info["err_nominal"]
        assert err > 0
        whole.close()
    bad = _Bad(name, "front")
    worst = 0.0
    for cut in sci.front_cuts(spb, dec):
        assert cut % spb == 0 and (cut // dec) % 64 != 0
        states, got_m, got_e = [], [], []
        for r, (rx, lo, hi) in enumerate(((rx0, 0, cut), (rx1, cut, n))):
            t, off = _own_tensor(x[2 * lo:2 * hi], eight)
            torch.cuda.synchronize()        # (the context's stream does not wait for the copy's)
            halo = x[2 * (lo - H):2 * lo] if r and H else None
            res, s = rx.shard_begin(t.data_ptr() + off, hi - lo, halo, r == 1, None)
            if r:
                res, s = rx.shard_refine(states[0])
            states.append(s)
            what = "shard %d" % r
            olo, ohi = lo // dec, hi // dec
            b = rx.bits()
            bad.check(b.size == ohi - olo and (b == want.bits[olo:ohi]).all(), cut, what + ": bits",
                      np.nonzero(b != want.bits[olo:ohi])[0][:8] if b.size == ohi - olo else b.size)
            e = edges_of(want.bits[olo:ohi])
            bad.check(res.stats["num_edges"] == len(e) and list(rx.edges()) == list(e), cut, what + ": edges",
                      (res.stats["num_edges"], list(rx.edges())[:4]), (len(e), list(e)[:4]))
            bad.check(res.stats["front_form"] == rx.front_info()["form"] == getattr(ok, form), cut, what + ": front_form",
                      res.stats["front_form"], getattr(ok, form))
            got_m += [(int(p) + olo, bytes(q)) for p, q in zip(res.msg_samples, res.payloads)]
            el, ne = rx.errors(sci.FRONT_OUTPUTS // per + 8)
            bad.check(ne == len(el) == res.stats["num_errors"], cut, what + ": num_errors")
            got_e += [int(p) + olo for p in el]
            if whole_fir is not None:
                y = rx.fir_output().astype(np.float64)
                near = np.r_[0:NEAR, ohi - olo - NEAR:ohi - olo]
                dist = float(np.abs(y[near] - whole_fir[olo + near]).max() / err)
                worst = max(worst, dist)
                bad.check(dist <= 1.0, cut, what + ": floats near its ends against the whole capture's, in bounds", dist, 1.0)
            del t
        bad.check(got_m == msgs, cut, "messages", got_m[:3], msgs[:3])
        bad.check(got_e == errs, cut, "errors", got_e[:6], errs[:6])
    rx0.close()
    rx1.close()
    d.close()
    line = "shard-cuts front leg %s: form %d, D %d, spb %d, halo %d, cuts %s, worst float distance / bound %.3g" % (
        name, getattr(ok, form), dec, spb, H, [c // dec for c in sci.front_cuts(spb, dec)], worst)
    print(line)
    record_property("shard_cuts", line)
    assert not bad, bad.report()
