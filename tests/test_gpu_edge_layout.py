"""The tile-info contract between the front ends and the edge stage, on the GPU: every kernel that writes
tile info words, and the generic path behind edge_count_kernel / edge_write_kernel, decodes captures whose level
changes are laid on chosen bit positions of chosen wave tiles (tests/edge_layout_inputs.py, checked on the CPU by
tests/test_edge_layout_host.py).  Impulse filters make the expected bits and edge lists known by construction; every
comparison is exact.  The tile size of a form is the front plan's; every run asserts the form that ran."""
import numpy as np
import pytest

from tests import edge_layout_inputs as E
from tests.helpers import golden_path

pytestmark = pytest.mark.gpu

NU = 0.2
# id -> (impulse shape, Receiver keywords, the form it must run).  "quiet_skip" in the keywords pins it (the tuned
# 1-stage kernels run tiles of 512 bits with the quiet test and of 1024 without); the other forms run
# test_positions with and without.
FORMS = {
    "nofilter": ("none", {}, "FRONT_NO_FILTER"),
    "fir1_mfma_i32k0": ("i32k0", {}, "FRONT_FIR1_MFMA"),
    "fir1_mfma_i32k31": ("i32k31", {}, "FRONT_FIR1_MFMA"),
    "fir1_mfma_i255": ("i255", {}, "FRONT_FIR1_MFMA"),
    "fir1_valu": ("i32k31", dict(fir_valu=True), "FRONT_FIR1_VALU"),
    "fir1_valu_exact": ("i32k31", dict(exact_fir=True), "FRONT_FIR1_VALU_EXACT"),
    "fir2_mfma": ("i16x32", {}, "FRONT_FIR2_MFMA"),
    "fir2_mfma_k0": ("i16x32k0", {}, "FRONT_FIR2_MFMA"),
    "fir2_valu": ("i16x32", dict(fir_valu=True), "FRONT_FIR2_VALU"),
    "fir2_valu_exact": ("i16x32k0", dict(exact_fir=True), "FRONT_FIR2_VALU_EXACT"),
    "tuned_fir1_R8": ("i32k0", dict(tune=NU, quiet_skip=True), "FRONT_TUNED_FIR1"),
    "tuned_fir1_R16": ("i32k31", dict(tune=NU, quiet_skip=False), "FRONT_TUNED_FIR1"),
    "tuned_multi_R8": ("i32k0", dict(carriers=[(NU, 0.1), (NU, 0.3)], quiet_skip=True), "FRONT_TUNED_MULTI"),
    "tuned_multi_R16": ("i32k31", dict(carriers=[(NU, 0.1), (NU, 0.3)], quiet_skip=False), "FRONT_TUNED_MULTI"),
    "tuned_fir2": ("i16x32", dict(tune=NU, tuned_fir2=True), "FRONT_TUNED_FIR2"),
    "generic": ("g3x40", {}, "FRONT_GENERIC"),
    "fir1_mfma_cs8": ("i32k31", dict(sample_format="cs8"), "FRONT_FIR1_MFMA_8"),
}
TILE_BITS = {"tuned_fir1_R8": 512, "tuned_fir1_R16": 1024, "tuned_multi_R8": 512, "tuned_multi_R16": 1024}
# (filters without a delay where the form has one: a capture of the batch starts high at its first bit)
GROUP_FORMS = ["nofilter", "fir1_mfma_i32k0", "fir2_mfma_k0", "tuned_fir1_R8", "generic"]
CHUNK_FORMS = ["fir1_mfma_i32k31", "fir2_mfma", "nofilter"]


@pytest.fixture(scope="module")
def ok():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from ookiedokie_amd import build as okbuild
    okbuild.build()
    import ookiedokie_amd as okm
    okm.lib()
    return okm


class _Form:
    def __init__(self, ok, name, quiet_skip=None):
        self.ok, self.name = ok, name
        self.shape, kw, form = FORMS[name]
        self.kw = dict(kw)
        if quiet_skip is not None:
            assert "quiet_skip" not in kw
            self.kw["quiet_skip"] = quiet_skip
        self.form = getattr(ok, form)
        stages, self.dec, _ = E.SHAPES[self.shape]
        self.stages = stages
        self.filter = ok.Filter.from_stages(stages) if stages else None
        self.results = len(self.kw.get("carriers", ())) or 1
        self.cs8 = self.kw.get("sample_format") == "cs8"
        self.tile_bits = self._plan_tile()

    def _plan_tile(self):
        """the tile the front plan gives this context: tile_bits of the kernels that write tile infos, the generic
        kernels' own tile otherwise"""
        from tests.front_plan_cases import plan_digest
        ok, kw = self.ok, self.kw
        flags = ((ok.RX_FIR_VALU if kw.get("fir_valu") else 0) | (ok.RX_EXACT_FIR if kw.get("exact_fir") else 0)
                 | (0 if kw.get("quiet_skip", True) else ok.RX_NO_QUIET_SKIP)
                 | (ok.RX_SAMPLES_CS8 if self.cs8 else 0) | (ok.RX_TUNED_FIR2 if kw.get("tuned_fir2") else 0))
        d = plan_digest(dict(flags=flags, threshold=E.THR, nu=kw.get("tune"), carriers=kw.get("carriers")), self.filter)
        assert d.form == self.form, (self.name, d.form)
        tile = d.tile_bits or d.gen_tile
        assert tile in (256, 512, 1024), tile
        if self.name in TILE_BITS:          # (the two register blocks of the tuned 1-stage kernels are both here)
            assert tile == TILE_BITS[self.name]
        assert (d.tile_bits != 0) == (self.form != ok.FRONT_GENERIC)
        return tile

    def capture(self, bits):
        if self.cs8:
            return E.capture(bits, self.shape, E.ON8, E.OFF8, np.int8)
        return E.capture(bits, self.shape)

    def receiver(self, n, spb, edge_capacity, max_captures=1, device=None, **more):
        kw = dict(self.kw, **more)
        return self.ok.Receiver(self.filter, device, max_samples=n, threshold=E.THR, samples_per_buffer=spb,
                                max_captures=max_captures, edge_capacity=self.results * edge_capacity, **kw)

    def check(self, rx, got, want, what):
        """want: [(bits, edges)] per capture (a carrier context: the one capture's, for every carrier)"""
        assert got.stats["front_form"] == self.form, what
        if self.results > 1:
            want = list(want) * self.results
        for k, (bits, edges) in enumerate(want):
            b = rx.bits(k)
            assert b.size == bits.size, (what, k)
            diff = np.nonzero(b != bits)[0]
            assert diff.size == 0, "%s, result %d: first differing bits at %s" % (what, k, diff[:5])
            assert list(rx.edges(k)) == list(edges), (what, k)
        assert got.stats["num_edges"] == sum(len(e) for _, e in want), what

    def run_batch(self, rx, caps, n):
        """captures of n samples each, side by side in device memory"""
        import torch
        host = np.stack(caps)
        dev_t = torch.from_numpy(host).cuda()
        got = rx.rx_device(dev_t.data_ptr(), n, num_captures=len(caps), stride=n)
        torch.cuda.synchronize()
        return got


_LAYOUTS = {}


def _layout(tile_bits):
    """layout and its complement, built once per tile size and never changed"""
    if tile_bits not in _LAYOUTS:
        bits, edges, _ = E.layout(tile_bits)
        comp = E.complement(bits, tile_bits)
        comp_edges = np.nonzero(np.diff(np.concatenate([[0], comp.astype(np.int8)])))[0].astype(np.uint64)
        for a in (bits, edges, comp, comp_edges):
            a.setflags(write=False)
        _LAYOUTS[tile_bits] = (bits, edges, comp, comp_edges)
    return _LAYOUTS[tile_bits]


# ---------------------------------------------------------------------------------------------- 1. positions ----

@pytest.mark.parametrize("form", list(FORMS))
def test_positions(ok, form):
    """One isolated instance of every tile class at every word index (layout): bits, edge list and count are the
    construction's.  Then the complementary layout on the same context -- what the first run wrote into its all-high
    tiles lies under quiet tiles now -- and the first capture again."""
    pinned = "quiet_skip" in FORMS[form][1]
    for quiet in ((None,) if pinned else (True, False)):
        f = _Form(ok, form, quiet)
        T = f.tile_bits
        bits, edges, comp, comp_edges = _layout(T)
        n = bits.size * f.dec
        rx = f.receiver(n, T * f.dec, max(len(edges), len(comp_edges)))
        first, second = f.capture(bits), f.capture(comp)
        for run, (iq, want) in enumerate(((first, (bits, edges)), (second, (comp, comp_edges)), (first, (bits, edges)))):
            got = rx.rx(iq)
            assert got.stats["decimated_samples"] == bits.size
            f.check(rx, got, [want], "%s tile %d quiet_skip %s run %d" % (form, T, quiet, run))
        rx.close()


# ----------------------------------------------------------------------- 2. a capture that ends high in a tile ----

@pytest.mark.parametrize("r", E.ENDING_R)
@pytest.mark.parametrize("form", list(FORMS))
def test_capture_ends_high_inside_a_tile(ok, form, r):
    """Whole buffers, n_out = r (mod the tile), the level still on at the end: no edge at n_out -- changes at or
    beyond n_out do not exist -- whether the last tile holds nothing else (a change counted there would be its one
    change) or two real changes.  Alone, and as the middle capture of a batch of three (a carrier context takes one
    capture per run: alone only), where one change too many also shifts the capture behind.
    Before the matrix-core epilogues masked their change bits by n_out, every residue but 0 failed for FRONT_FIR1_MFMA
    (32 and 255 taps), FRONT_FIR1_MFMA_8 and FRONT_FIR2_MFMA, and for no other form: tile 1024, n_out 5121, the last
    tile holding only the high level, gave the edges [3149, 5121] for [3149]."""
    f = _Form(ok, form)
    T = f.tile_bits
    for two in (False, True):
        case = E.ending_high(T, E.ending_r(r, T), two)
        if case is None:
            continue            # (a tile of one or two bits holds no two changes behind its first bit)
        bits, edges, per_buf = case
        n_out = bits.size
        spb, n = per_buf * f.dec, n_out * f.dec
        what = "%s tile %d n_out %d two_changes %s" % (form, T, n_out, two)
        rx = f.receiver(n, spb, n_out)
        got = rx.rx(f.capture(bits))
        assert got.stats["decimated_samples"] == n_out
        f.check(rx, got, [(bits, edges)], what)
        rx.close()
        if f.results > 1:
            continue
        others = [E.few_a_cases(T, n_out, seed) for seed in (1, 4)]
        want = [others[0], (bits, edges), others[1]]
        rx = f.receiver(n, spb, 3 * n_out, max_captures=3)
        got = f.run_batch(rx, [f.capture(b) for b, _ in want], n)
        f.check(rx, got, want, what + " in a batch")
        rx.close()


# ------------------------------------------------------------------------------------ 3. scan-group boundary ----

@pytest.mark.parametrize("form", GROUP_FORMS)
def test_scan_group_boundary(ok, form):
    """Edges on the boundary between two first-level scan groups (1024 blocks): the last bit of block 1023, the first
    bit of block 1024, a run across both; then a batch of three captures of 700 blocks, where the boundary falls
    inside capture 1 and every capture boundary has a level on one side.  The edge list has exactly the room the
    expected edges take."""
    f = _Form(ok, form)
    T = f.tile_bits
    spb = E.GROUP_PER_BUF * f.dec           # whole buffers: a capture that ends high ends there, inside a tile
    alone = {kind: E.group_layout(T, kind) for kind in E.F_KINDS}
    n = max(bits.size for bits, _ in alone.values()) * f.dec
    rx = f.receiver(n, spb, max(len(edges) for _, edges in alone.values()))
    for kind, (bits, edges) in alone.items():
        got = rx.rx(f.capture(bits))
        assert got.stats["decimated_samples"] == bits.size
        f.check(rx, got, [(bits, edges)], "%s %s" % (form, kind))
    rx.close()
    caps, cap_edges = E.group_layout_batch(T, E.SHAPES[f.shape][2])
    n = caps[0].size * f.dec
    rx = f.receiver(n, spb, sum(len(e) for e in cap_edges), max_captures=3)
    got = f.run_batch(rx, [f.capture(b) for b in caps], n)
    f.check(rx, got, list(zip(caps, cap_edges)), "%s batch" % form)
    rx.close()


# ----------------------------------------------------------------------------------------- 4. chunk boundary ----

@pytest.mark.parametrize("form", CHUNK_FORMS)
def test_chunk_boundary(ok, oracle, form):
    """A pipelined run (chunks of 4 buffers, the front end of one beside the state machine of the one before): a level
    high across a chunk boundary, an edge exactly at a chunk's first bit and a one-sample pulse at a chunk's last bit.
    Bits and edges are the construction's, messages and errors the oracle's."""
    f = _Form(ok, form)
    T, dec = f.tile_bits, f.dec
    spb = 4096
    # chunks end where a block and a buffer end: multiples of 4096 outputs here; the chunk aimed at is 4 buffers
    chunk_out = max(4096, 4 * spb // dec // 4096 * 4096)
    n_out = 4 * chunk_out
    n = n_out * dec
    assert n >= 16 * spb
    bits, edges = E.chunk_layout(n_out, chunk_out, T)
    iq = f.capture(bits)
    rate = 3000000 // dec
    d = ok.Device.load(golden_path("devices", "p3l-nexa2012"), rate)
    od = oracle.load_device_json(golden_path("devices", "p3l-nexa2012"), rate)[0]
    of = oracle.make_fir([(s, np.asarray(h, np.float32)) for s, h in f.stages]) if f.stages else None
    want = oracle.rx(iq, of, E.THR, od, spb, want_bits=True)
    assert (want.bits == bits).all()
    # (each chunk gets a share of the edge list by its blocks)
    rx = f.receiver(n, spb, n_out, device=d, pipeline_chunk_samples=4 * spb)
    got = rx.rx(iq)
    assert got.stats["pipeline_chunks"] >= 2 and got.stats["fsm_path"] == 1, got.stats
    assert got.stats["pipeline_chunks"] == 4, "the cases do not sit on chunk boundaries"
    f.check(rx, got, [(bits, edges)], form)
    assert list(got.msg_samples) == list(want.msg_samples)
    assert (got.payloads == want.payloads).all()
    errs, nerr = rx.errors()
    assert nerr == len(want.err_samples) and list(errs) == list(want.err_samples)
    rx.close()
