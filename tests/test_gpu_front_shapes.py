"""The front ends across stage shapes, on the GPU, against the CPU oracle (and tests/tuned_contract.py for tuned
contexts): the two-stage family (fir2_mfma_kernel, fir2_bits_kernel) at every corner of its (n1 <= 16, n2 <= 32) tap
range, and the generic kernels (fir_generic_kernel, fir_tuned_generic_kernel) across decimations, stage counts and
tile sizes -- down to the filters whose level buffers only hold a tile smaller than 1024 outputs.  Every case first
checks, on the oracle's result alone, that the capture decides something (tests/front_shapes_inputs.py), and pins the
kernel that ran by stats["front_form"]."""
import numpy as np
import pytest

from tests import front_shapes_inputs as S
from tests.helpers import edges_of
from tests.test_survey_host import np_hist, oracle_power
from tests.tuned_contract import contract_rx, lib_stages

pytestmark = pytest.mark.gpu

FIR_RTOL = 1e-5                 # the suite's float rule for the fused forms (test_gpu_parity.py)
NU = 0.2
CARRIERS = [(0.2, S.THR), (-0.31, 0.05)]


@pytest.fixture(scope="module")
def ok():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from ookiedokie_amd import build as okbuild
    okbuild.build()
    import ookiedokie_amd as okm
    okm.lib()
    return okm


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)


_CASES = {}


def _case(oracle, shape):
    """(stages, capture, oracle filter, oracle result) of a shape: computed once, shared, left unchanged"""
    key = S.shape_id(shape)
    if key not in _CASES:
        st = S.stages(shape)
        n = S.sweep_len(shape)
        iq = S.capture(n, seed=S.capture_seed(shape))
        of = oracle.make_fir(st)
        want = oracle.rx(iq, of, S.THR, None, S.SPB, want_bits=True, want_fir=True)
        frac, edges = S.check_oracle_result(want.bits, n, S.total_decimation(shape))
        print("oracle", key, "n", n, "ones %.3f" % frac, "edges", edges)
        _frozen(iq, want.bits, want.fir)
        _CASES[key] = (st, iq, of, want)
    return _CASES[key]


_TUNED = {}


def _tuned_case(oracle, ok, shape):
    """the shape's two-carrier capture, and the contract's (bits, floats) for every carrier of CARRIERS (the first
    one is the tuned context's): each decides something before a GPU result is looked at"""
    key = S.shape_id(shape)
    if key not in _TUNED:
        st = S.stages(shape)
        iq = S.two_carrier_capture(shape, [nu for nu, _ in CARRIERS])
        f = ok.Filter.from_stages(st)
        want = [contract_rx(iq, lib_stages(f, nu), thr, S.SPB) for nu, thr in CARRIERS]
        for k in range(len(CARRIERS)):
            frac, edges = S.check_oracle_result(want[k][0], iq.size // 2, S.total_decimation(shape))
            print("contract", key, "carrier", k, "ones %.3f" % frac, "edges", edges)
        _frozen(iq, *[a for w in want for a in w])
        _TUNED[key] = (iq, want)
    return _TUNED[key]


def _same_bits(rx, want_bits, what, capture=0):
    bits = rx.bits(capture)
    assert bits.size == want_bits.size, what
    diff = np.nonzero(bits != want_bits)[0]
    assert diff.size == 0, "%s: first differing outputs %s" % (what, diff[:5])
    assert list(rx.edges(capture)) == list(edges_of(want_bits)), what
    # the bit words behind the last output, up to the end of the capture's words, are zeros
    import ookiedokie_amd as okm
    nw = int(okm.lib().ookd_rx_bit_words(rx._h))
    words = np.zeros(max(nw, 1), dtype=np.uint64)
    assert okm.lib().ookd_rx_get_bits(rx._h, capture, words.ctypes.data, nw) == 0
    tail = np.unpackbits(words[:nw].view(np.uint8), bitorder="little")[want_bits.size:]
    assert nw * 64 >= want_bits.size and not tail.any(), "%s: bits set behind the last output" % what


def _same_floats(y, want, what):
    bad = np.nonzero((y.view(np.uint32) != want.view(np.uint32)).any(axis=1))[0]
    assert y.shape == want.shape and bad.size == 0, "%s: floats differ first at outputs %s" % (what, bad[:5])


# ------------------------------------------------------------------ 1. two-stage family: tap-count sweep ----

def _fir2_forms(ok):
    return (("mfma", {}, ok.FRONT_FIR2_MFMA), ("valu", dict(fir_valu=True), ok.FRONT_FIR2_VALU),
            ("exact", dict(exact_fir=True), ok.FRONT_FIR2_VALU_EXACT))


@pytest.mark.parametrize("n1,n2", S.FIR2_SHAPES, ids=["%dx%d" % s for s in S.FIR2_SHAPES])
def test_two_stage_tap_counts(ok, oracle, n1, n2):
    """every form of the two-stage family at (n1, n2) taps: bits, edges and output count are the oracle's; the exact
    form's floats too, the fused forms' within the suite's rule; the 205 LSB stretch goes through the exact
    recompute, the silence takes the quiet shortcut and the shortcut changes no bit"""
    st, iq, of, want = _case(oracle, S.fir2_shape(n1, n2))
    n = iq.size // 2
    f = ok.Filter.from_stages(st)
    gain = float(np.prod([max(1.0, float(np.abs(h.astype(np.float64)).sum())) for _, h in st]))
    tol = FIR_RTOL * np.maximum(np.abs(want.fir), gain * float(np.abs(iq).max()) / 2048.0)
    for name, kw, form in _fir2_forms(ok):
        rx = ok.Receiver(f, None, max_samples=n, threshold=S.THR, samples_per_buffer=S.SPB, edge_capacity=n + 64,
                         keep_fir=True, **kw)
        assert rx.front_info()["form"] == form, name
        got = rx.rx(iq)
        assert got.stats["front_form"] == form, name
        assert got.stats["decimated_samples"] == want.decimated
        _same_bits(rx, want.bits, name)
        y = rx.fir_output()
        if name == "exact":
            _same_floats(y, want.fir, name)
        else:
            worst = np.abs(y - want.fir) / tol
            assert worst.max() <= 1.0, "%s: output %d off by %.3g of the tolerance" % (name, int(worst.argmax() // 2), worst.max())
        rx.close()
        # the legs ran what they claim: band, quiet shortcut, and the shortcut off
        res = {}
        for quiet in (True, False):
            rx = ok.Receiver(f, None, max_samples=n, threshold=S.THR, samples_per_buffer=S.SPB, edge_capacity=n + 64,
                             count_quiet=True, quiet_skip=quiet, **kw)
            got = rx.rx(iq)
            assert got.stats["front_form"] == form, name
            _same_bits(rx, want.bits, "%s quiet_skip=%s" % (name, quiet))
            res[quiet] = got.stats
            rx.close()
        print("two-stage", n1, n2, name, "recomputes", res[True]["guard_recomputes"], "quiet", res[True]["quiet_waves"],
              "of", res[True]["total_waves"])
        if name != "exact":
            assert res[True]["guard_recomputes"] > 0 and res[False]["guard_recomputes"] > 0, name
        assert 0 < res[True]["quiet_waves"] < res[True]["total_waves"], name
        assert res[False]["quiet_waves"] == 0, name


def test_two_stage_unaligned_and_batched(ok, oracle):
    """(3, 5) taps from a device pointer 4 bytes past a 16-byte boundary, and as three captures whose stride is no
    multiple of 4 samples: the tiles take the path that fetches sample by sample"""
    import torch
    st, iq, of, want = _case(oracle, S.fir2_shape(3, 5))
    n = iq.size // 2
    f = ok.Filter.from_stages(st)
    # one capture, one sample into an aligned allocation
    buf = torch.zeros(2 * (n + 4), dtype=torch.int16, device="cuda")
    assert buf.data_ptr() % 16 == 0
    buf[2:2 + 2 * n] = torch.from_numpy(np.array(iq)).cuda()
    caps = 3
    stride = n + 5 + ((n + 5) % 4 == 0)
    assert stride % 4 != 0
    host = np.zeros((caps, 2 * stride), np.int16)
    wants = []
    for c in range(caps):
        host[c, :2 * n] = iq if c == 0 else S.capture(n, seed=100 + c)
        wants.append(want if c == 0 else oracle.rx(host[c, :2 * n], of, S.THR, None, S.SPB, want_bits=True))
        S.check_oracle_result(wants[c].bits, n, 4)
    dev_t = torch.from_numpy(host).cuda()
    for name, kw, form in _fir2_forms(ok):
        rx = ok.Receiver(f, None, max_samples=n, threshold=S.THR, samples_per_buffer=S.SPB, edge_capacity=n + 64, **kw)
        got = rx.rx_device(buf.data_ptr() + 4, n)
        assert got.stats["front_form"] == form, name
        assert got.stats["decimated_samples"] == want.decimated
        _same_bits(rx, want.bits, name + " unaligned")
        rx.close()
        rx = ok.Receiver(f, None, max_samples=n, max_captures=caps, threshold=S.THR, samples_per_buffer=S.SPB,
                         edge_capacity=caps * n + 64, **kw)
        got = rx.rx_device(dev_t.data_ptr(), n, num_captures=caps, stride=stride)
        assert got.stats["front_form"] == form, name
        for c in range(caps):
            _same_bits(rx, wants[c].bits, "%s capture %d" % (name, c), c)
        rx.close()


# ------------------------------------------------------------------ 4. / 5. generic kernels ----

def _receiver_parity(ok, st, iq, want, what, **kw):
    """an untuned context on the generic kernel: bits, edges, output count and floats are the oracle's"""
    n = iq.size // 2
    f = ok.Filter.from_stages(st)
    rx = ok.Receiver(f, None, max_samples=max(n, 1), threshold=S.THR, edge_capacity=n + 64, keep_fir=True,
                     **dict(dict(samples_per_buffer=S.SPB), **kw))
    assert rx.front_info()["form"] == ok.FRONT_GENERIC, what
    got = rx.rx(iq)
    assert got.stats["front_form"] == ok.FRONT_GENERIC, what
    assert got.stats["decimated_samples"] == want.decimated, what
    _same_bits(rx, want.bits, what)
    _same_floats(rx.fir_output(), want.fir, what)
    rx.close()


def _batched_parity(ok, oracle, st, iq, of, want, dec):
    """three captures in one run, a stride that is no multiple of anything: each capture's result is the oracle's"""
    import torch
    n = iq.size // 2
    f = ok.Filter.from_stages(st)
    caps, stride = 3, n + 5
    host = np.zeros((caps, 2 * stride), np.int16)
    wants = []
    for c in range(caps):
        host[c, :2 * n] = iq if c == 0 else S.capture(n, seed=200 + c)
        wants.append(want if c == 0 else oracle.rx(host[c, :2 * n], of, S.THR, None, S.SPB, want_bits=True, want_fir=True))
        S.check_oracle_result(wants[c].bits, n, dec)
    dev_t = torch.from_numpy(host).cuda()
    rx = ok.Receiver(f, None, max_samples=n, max_captures=caps, threshold=S.THR, samples_per_buffer=S.SPB,
                     edge_capacity=caps * n + 64, keep_fir=True)
    got = rx.rx_device(dev_t.data_ptr(), n, num_captures=caps, stride=stride)
    assert got.stats["front_form"] == ok.FRONT_GENERIC
    for c in range(caps):
        _same_bits(rx, wants[c].bits, "capture %d" % c, c)
        _same_floats(rx.fir_output(c), wants[c].fir, "capture %d" % c)
    rx.close()


def _tuned_parity(ok, oracle, shape):
    """a tuned and a carrier context on the tuned generic kernel against the contract: bits equal, floats bit-identical"""
    st = S.stages(shape)
    iq, want = _tuned_case(oracle, ok, shape)
    n = iq.size // 2
    f = ok.Filter.from_stages(st)
    rx = ok.Receiver(f, None, max_samples=n, threshold=S.THR, samples_per_buffer=S.SPB, edge_capacity=n + 64,
                     keep_fir=True, tune=NU)
    assert rx.front_info()["form"] == ok.FRONT_TUNED_GENERIC
    got = rx.rx(iq)
    assert got.stats["front_form"] == ok.FRONT_TUNED_GENERIC
    _same_bits(rx, want[0][0], "tuned")
    _same_floats(rx.fir_output(), want[0][1], "tuned")
    rx.close()
    return f, iq, want


ALL_GENERIC = dict(S.GENERIC_SHAPES, **S.LARGE_SHAPES)


@pytest.mark.parametrize("name", sorted(ALL_GENERIC))
def test_generic_kernel_parity(ok, oracle, name):
    """shapes whose level buffers hold a 1024-output tile and shapes that need a smaller one"""
    st, iq, of, want = _case(oracle, ALL_GENERIC[name])
    _receiver_parity(ok, st, iq, want, name)


@pytest.mark.parametrize("name", ["d3t40", "d5t3"])
def test_generic_kernel_edges_buffers_batches_cs8(ok, oracle, name):
    """lengths at the decimation edge and the tile edge; a buffer size that is no multiple of anything; three
    captures in one run; a CS8 capture against the oracle on the widened one"""
    import torch
    shape = S.GENERIC_SHAPES[name]
    st, iq, of, want = _case(oracle, shape)
    dec = S.total_decimation(shape)
    f = ok.Filter.from_stages(st)
    for n in S.edge_lengths(dec):
        x = np.array(iq[:2 * n])
        _receiver_parity(ok, st, x, oracle.rx(x, of, S.THR, None, S.SPB, want_bits=True, want_fir=True), "n=%d" % n)
    _receiver_parity(ok, st, iq, oracle.rx(iq, of, S.THR, None, 1000, want_bits=True, want_fir=True), "spb 1000",
                     samples_per_buffer=1000)
    # batched
    n = iq.size // 2
    _batched_parity(ok, oracle, st, iq, of, want, dec)
    # CS8
    n = iq.size // 2
    raw, wide = S.to_cs8(iq)
    w8 = oracle.rx(wide, of, S.THR, None, S.SPB, want_bits=True, want_fir=True)
    S.check_oracle_result(w8.bits, n, dec)
    rx = ok.Receiver(f, None, max_samples=n, threshold=S.THR, samples_per_buffer=S.SPB, edge_capacity=n + 64, keep_fir=True,
                     sample_format="cs8")
    got = rx.rx(raw)
    assert got.stats["front_form"] == ok.FRONT_GENERIC and got.stats["decimated_samples"] == w8.decimated
    _same_bits(rx, w8.bits, "cs8")
    _same_floats(rx.fir_output(), w8.fir, "cs8")
    rx.close()


@pytest.mark.parametrize("name", ["d3t40", "d2d1d2", "d5t3"] + sorted(S.LARGE_SHAPES))
def test_tuned_generic_kernel_parity(ok, oracle, name):
    """tune=0.2 and carriers=[0.2, (-0.31, 0.05)] on the tuned generic kernel, against tests/tuned_contract.py, at
    tiles of 1024 outputs and at every smaller one"""
    f, iq, want = _tuned_parity(ok, oracle, ALL_GENERIC[name])
    n = iq.size // 2
    rx = ok.Receiver(f, None, max_samples=n, threshold=S.THR, samples_per_buffer=S.SPB, edge_capacity=2 * n + 64,
                     keep_fir=True, carriers=[CARRIERS[0][0], CARRIERS[1]])
    assert rx.front_info()["form"] == ok.FRONT_TUNED_GENERIC
    got = rx.rx(iq)
    assert got.stats["front_form"] == ok.FRONT_TUNED_GENERIC
    for k in range(len(CARRIERS)):
        _same_bits(rx, want[k][0], "carrier %d" % k, k)
        _same_floats(rx.fir_output(k), want[k][1], "carrier %d" % k)
    rx.close()


# ------------------------------------------------------------------ 5. large total decimation ----

SMALL_TILES = sorted(name for name in S.LARGE_SHAPES if S.TILES[name] < 256)


@pytest.mark.parametrize("name", SMALL_TILES)
def test_small_tiles_edges_and_batches(ok, oracle, name):
    """tiles of 128 and 64 outputs, where some of a workgroup's four waves own no bit word: lengths around the tile's
    edge (one tile and an output more or less), and three captures in one run"""
    shape = S.LARGE_SHAPES[name]
    st, iq, of, want = _case(oracle, shape)
    dec, tile = S.total_decimation(shape), S.TILES[name]
    for n in (tile * dec - 1, tile * dec, tile * dec + 1, 2 * tile * dec + dec):
        x = np.array(iq[:2 * n])
        _receiver_parity(ok, st, x, oracle.rx(x, of, S.THR, None, S.SPB, want_bits=True, want_fir=True), "n=%d" % n)
    _batched_parity(ok, oracle, st, iq, of, want, dec)


def test_filters_that_fit_no_tile_are_refused_at_creation(ok):
    """the refusal comes from the constructor -- of the context, the tuned context, the carrier context and the
    streaming FIR --, names its entry point, the total decimation, the tap counts and the limit, and no run is needed
    to meet it"""
    f = ok.Filter.from_stages([(4096, [0.125] * 8)])
    for who, make in (("ookd_rx_create:", lambda: ok.Receiver(f, None, max_samples=1 << 16)),
                      ("ookd_rx_create_tuned:", lambda: ok.Receiver(f, None, max_samples=1 << 16, tune=NU)),
                      ("ookd_rx_create_carriers:", lambda: ok.Receiver(f, None, max_samples=1 << 16, carriers=CARRIERS)),
                      ("ookd_fir_create:", lambda: ok.StreamFir(f, 8192))):
        with pytest.raises(ok.OokdError) as e:
            make()
        text = str(e.value)
        assert who in text and "total decimation 4096 " in text and "tap counts [8]" in text, text
        assert "%d bytes" % ((63 * 4096 + 8 + 2) * 8) in text and "163840 bytes" in text, text


@pytest.mark.parametrize("chunk", [7, 8192, 30000])
@pytest.mark.parametrize("name", sorted(S.LARGE_SHAPES))
def test_large_decimation_stream_fir(ok, oracle, name, chunk):
    """as test_stream_fir_matches_oracle_for_any_chunking: the floats do not depend on the chunking (30000: one call,
    several tiles of the smaller sizes)"""
    st, iq, of, _ = _case(oracle, S.LARGE_SHAPES[name])
    x = oracle.unpack(iq[:2 * 30000])
    sf = ok.StreamFir(ok.Filter.from_stages(st), max(chunk, 8192))
    y = np.concatenate([sf.filter_and_decimate(x[o:o + chunk]) for o in range(0, x.shape[0], chunk)])
    want = oracle.fir_run(of, x, chunk)
    assert want.shape[0] == 30000 // S.total_decimation(S.LARGE_SHAPES[name]) and np.abs(want).max() > 0.1
    _same_floats(y, want, "chunk %d" % chunk)
    sf.close()


@pytest.mark.parametrize("name", sorted(S.LARGE_SHAPES))
def test_large_decimation_survey_then_decode(ok, oracle, name):
    """what examples/ookd_scan.c chains: a Survey and a Receiver on the same filter and capture both succeed"""
    st, iq, of, want = _case(oracle, S.LARGE_SHAPES[name])
    n = iq.size // 2
    f = ok.Filter.from_stages(st)
    sv = ok.Survey(f)
    hist = sv.survey(iq)
    assert (hist == np_hist(oracle_power(oracle, of, iq))).all()
    sv.close()
    rx = ok.Receiver(f, None, max_samples=n, threshold=S.THR, samples_per_buffer=S.SPB, edge_capacity=n + 64)
    got = rx.rx(iq)
    assert got.stats["front_form"] == ok.FRONT_GENERIC
    _same_bits(rx, want.bits, name)
    rx.close()
