"""The scan's walk from synchronising spans (scan_sync_kernel, scan_syncwalk_kernel, scan_syncpick_kernel)
at its region limits, on the streams of tests/sync_walk_inputs.py: the first sync leaf of a block at either end of it,
the next region start 1, 7, 8 and 9 blocks on, 8 and 9 blocks without one at the capture's tail, regions around the
walk's 64-leaf fetch, stuck stretches `depth` and `depth` + 1 leaves in front of a sync leaf (inside a block and across
a block boundary), errors whose dropped rest-of-buffer ends inside a region, on a sync leaf and behind it, 1023 to 2049
blocks for the pick kernel's one workgroup (the regions across its thread and wave seams started in a candidate other
than the first), batches, and two captures pipelined in chunks whose middle chunk starts high.  Everything is bit-exact against the CPU oracle, and on the walk
leg scan_entry_form is what the host restatement of the module says (test_sync_walk_host.py checks the inputs without
a GPU): 1 where the walk holds, 2 with fsm_fallback_reason 16 where it gives up and the scan composes."""
import pytest

from tests import dense_devices as dd
from tests import sync_walk_inputs as sw
from tests.helpers import edges_of
from tests.test_gpu_dense_results import LEGS, _batch, _same
from tests.test_gpu_parity import _sync_walk_forced

pytestmark = pytest.mark.gpu

ERR_HIP = -4                # OOKD_ERR_HIP


@pytest.fixture(scope="module")
def ok():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from ookiedokie_amd import build as okbuild
    okbuild.build()
    import ookiedokie_amd as okm
    okm.lib()
    return okm


_wanted = {}


def _reference(oracle, name):
    """per case, computed once: [(I,Q samples, the oracle's result, edges)] per capture"""
    if name not in _wanted:
        c = sw.case(name)
        od = dd.fsm_desc(oracle, sw.DEVICE)
        out = []
        for stream in sw.streams(c):
            iq = dd.iq_of(stream)
            want = oracle.rx(iq, None, dd.THR, od, c.spb, want_bits=True, msg_cap=1 << 17)
            out.append((iq, want, len(edges_of(want.bits))))
        _wanted[name] = out
    return _wanted[name]


class _Context:
    """a Receiver for the case on one leg of test_gpu_dense_results.LEGS, and runs of it against the oracle"""

    def __init__(self, ok, oracle, name, leg):
        self.ok = ok
        self.c = sw.case(name)
        self.ref = _reference(oracle, name)
        self.leg = leg
        kw, walk, chunked = next((kw, walk, chunked) for lname, kw, walk, chunked in LEGS if lname == leg)
        self.n = max(iq.size // 2 for iq, _, _ in self.ref)
        if name in sw.GIVE_UP_THEN:                 # (room for the capture that is run behind the give-up)
            self.n = max(self.n, _reference(oracle, sw.GIVE_UP_THEN[name])[0][0].size // 2)
        M = sum(len(w.msg_samples) for _, w, _ in self.ref)
        kw = dict(kw, message_slots=max(len(w.msg_samples) for _, w, _ in self.ref) + 2)
        if chunked:
            kw["pipeline_chunk_samples"] = sw.CHUNK_BUFFERS * self.c.spb
        if leg == "rounds":
            kw["segment_buffers"] = max(1, self.n // self.c.spb // 8)
        self.d = dd.ok_device(ok, sw.DEVICE)
        with _sync_walk_forced(walk):
            self.rx = ok.Receiver(None, self.d, max_samples=self.n, max_captures=len(self.ref), threshold=dd.THR,
                                  samples_per_buffer=self.c.spb, message_capacity=M + 64, **kw)

    def run(self, ref=None):
        """one run, compared with the oracle: message samples, payloads, the error count, every error position, num_edges.
        ref: another case's reference (one capture) to run on this context.  Returns the stats."""
        try:
            return self._run(self.ref if ref is None else ref)
        except self.ok.OokdError as e:
            if e.code == ERR_HIP:
                # a kernel of this chain faulted, or the runtime failed: nothing more is started on this GPU
                pytest.exit("HIP failure in %s, leg %s: %s" % (self.c.name, self.leg, e), returncode=3)
            raise

    def _run(self, ref):
        tag = (self.c.name, self.leg)
        if len(ref) == 1:
            iq, want, nedges = ref[0]
            got = self.rx.rx(iq)
            _same(self.rx, got, want, tag)
        else:
            import torch
            host, n, stride = _batch([iq for iq, _, _ in ref])
            assert n == self.n
            dev_iq = torch.from_numpy(host).cuda()
            torch.cuda.synchronize()            # (the context's stream does not wait for the copy's)
            got = self.rx.rx_device(dev_iq.data_ptr(), n, num_captures=len(ref), stride=stride)
            for k, (_, want, _) in enumerate(ref):
                gc = got.for_capture(k)
                assert list(gc.msg_samples) == list(want.msg_samples), tag + (k,)
                assert gc.payloads.shape == want.payloads.shape and (gc.payloads == want.payloads).all(), tag + (k,)
            errs_want = [int(e) for _, w, _ in ref for e in w.err_samples]         # capture-major
            errs, nerr = self.rx.errors(len(errs_want) + 8)
            assert nerr == len(errs_want) == got.stats["num_errors"] and list(errs) == errs_want, tag
            nedges = sum(x for _, _, x in ref)
        st = got.stats
        print("sync-walk %-28s leg %-14s fsm_path %d entry form %d reason %d chunks %d edges %d messages %d errors %d"
              % (self.c.name, self.leg, st["fsm_path"], st["scan_entry_form"], st["fsm_fallback_reason"],
                 st["pipeline_chunks"], st["num_edges"], len(got.msg_samples), st["num_errors"]))
        assert st["num_edges"] == nedges, tag
        return st

    def close(self):
        self.rx.close()
        self.d.close()


@pytest.mark.parametrize("name", sw.NAMES)
def test_walk_leg(ok, oracle, name):
    """The walk forced, twice on one context.  Where the walk holds both runs report form 1 with no fallback reason --
    the second with the first's records, digests and planes behind it.  Where it gives up the first run reports form 2
    with reason 16 and the second comes out composed: the back-off.  Behind run_9 and tail_9 the same context then
    decodes run_8's capture, in whatever form the back-off gives it."""
    c = sw.case(name)
    ctx = _Context(ok, oracle, name, "walk")
    try:
        for run in range(2):
            st = ctx.run()
            assert st["fsm_path"] == 1, (name, run, st)
            assert st["scan_entry_form"] == c.form, (name, run, st)
            if c.form == 1:
                assert st["fsm_fallback_reason"] == 0, (name, run, st)
            else:
                # (the second run does not try the walk again: no reason)
                assert st["fsm_fallback_reason"] == (sw.REASON_SYNC if run == 0 else 0), (name, run, st)
        if name in sw.GIVE_UP_THEN:
            other = _reference(oracle, sw.GIVE_UP_THEN[name])
            assert other[0][0].size // 2 <= ctx.n
            st = ctx.run(other)
            # the back-off still holds: composed outright, though this capture's walk would hold
            assert st["fsm_path"] == 1 and st["scan_entry_form"] == 2 and st["fsm_fallback_reason"] == 0, (name, st)
    finally:
        ctx.close()


@pytest.mark.parametrize("leg", ["composed", "tables", "sims", "rounds"])
@pytest.mark.parametrize("name", sw.NAMES + sw.CHUNK_NAMES)
def test_other_legs(ok, oracle, name, leg):
    """the same capture composed (scan_tables), with the tables' default, simulating every span, and in the round form:
    what the walk leg is held against besides the oracle, and the forms a give-up falls back to"""
    c = sw.case(name)
    ctx = _Context(ok, oracle, name, leg)
    try:
        st = ctx.run()
        if leg == "sims" and (c.kind == "chunks" or c.kind == "single" and c.meta.get("stuck")):
            # the form that simulates every span has no stuck codes: it refuses a capture with a stuck stretch, and
            # the round form decodes it
            assert st["fsm_path"] == 3 and st["fsm_fallback_reason"] != 0, (name, leg, st)
            return
        assert st["fsm_path"] == (2 if leg == "rounds" else 1), (name, leg, st)
        if leg != "rounds":
            assert st["fsm_fallback_reason"] == 0, (name, leg, st)
        if leg == "composed":
            assert st["scan_entry_form"] == 2, (name, leg, st)
    finally:
        ctx.close()


@pytest.mark.parametrize("name", sw.CHUNK_NAMES)
def test_pipelined_walk_leg(ok, oracle, name):
    """Pipelined in chunks of four buffers with the walk forced, twice on one context; every chunk is a scan of its own,
    with its own blocks, and chunk 1 starts high.  d = depth + 1: every chunk's walk holds, form 1, three chunks.
    d = depth: chunk 1's walk gives up, which redoes the capture whole and composed (form 2, reason 16); the second run
    is pipelined again and composed outright.  Then the same capture pipelined without the walk."""
    c = sw.case(name)
    nchunks = len(sw.chunk_bounds(_reference(oracle, name)[0][0].size // 2, c.spb))
    ctx = _Context(ok, oracle, name, "pipelined+walk")
    try:
        for run in range(2):
            st = ctx.run()
            assert st["fsm_path"] == 1 and st["scan_entry_form"] == c.form, (name, run, st)
            assert st["fsm_fallback_reason"] == (sw.REASON_SYNC if c.form == 2 and run == 0 else 0), (name, run, st)
            if c.form == 1 or run == 1:
                assert st["pipeline_chunks"] == nchunks, (name, run, st)
    finally:
        ctx.close()
    ctx = _Context(ok, oracle, name, "pipelined")
    try:
        st = ctx.run()
        assert st["fsm_path"] == 1 and st["fsm_fallback_reason"] == 0 and st["pipeline_chunks"] == nchunks, (name, st)
    finally:
        ctx.close()
