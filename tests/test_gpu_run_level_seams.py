"""The pulse levels at the seams of their kernel (run_levels.hip): the 64 lanes of the segmented wave
maximum, the 256-output pass of the workgroup over a tile, the tile, the block of the edge list, the 64-tile ballot,
the second and later iterations of the grid-stride loop, tiles narrower than a wave, the packing of the captures' peaks
into one array, and the cleaned list's single block.  The captures are those of tests/run_level_seams_inputs.py -- what
each is laid for is proved on the reference by tests/test_run_level_seams_host.py -- and every answer goes through
check() of tests/test_gpu_run_levels.py: peaks as uint32 patterns with no tolerance, the histogram, num_runs,
tiles_total and tiles_filtered against the numpy restatement (tests/run_levels_contract.py).  Without a filter the edge
list itself must be the laid one, element for element.

The speed rule: the whole suite runs for every later change, so every test here takes a few seconds at the most.  The
captures are as short as their seam allows (the longest, 133 000 unfiltered samples, is what two chunks of 64 tiles
need), contexts of one geometry are shared, the references behind a filter are computed once per module, and the
grid-stride batch repeats three contents over its 64 captures: if its reference ever becomes the slow part, shrink the
number of distinct contents, not the batch."""
import numpy as np
import pytest

from tests import run_level_seams_inputs as S
from tests.clean_contract import clean_of
from tests.helpers import edges_of, golden_path
from tests.run_levels_contract import (RATE, THR, SEAM_NU, assert_same_bits, assert_targets, oracle_fir, padded,
                                       seam_filtered, seam_narrow, seam_tuned, tiles_filtered_of)
from tests.test_gpu_run_levels import check
from tests.test_survey_host import oracle_power
from tests.tuned_contract import contract_rx, lib_stages, moved
from tests.tuned_survey_contract import contract_power

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


@pytest.fixture(scope="module")
def plain(ok):
    """unfiltered contexts by (samples, samples per buffer, sample format), shared by the tests of this module"""
    made = {}

    def get(n, spb, fmt="sc16q11"):
        if (n, spb, fmt) not in made:
            made[n, spb, fmt] = ok.Receiver(None, None, max_samples=n, samples_per_buffer=spb, threshold=THR,
                                            edge_capacity=n + 64, sample_format=fmt)
        return made[n, spb, fmt]
    yield get
    for rx in made.values():
        rx.close()


def lib_filter(ok, shape):
    if shape == "three":
        return ok.Filter.from_stages(S.three_stages())
    if shape.startswith("narrow"):
        return ok.Filter.from_stages(S.narrow_stages(int(shape[6:])))
    return ok.Filter.load(golden_path("filters", shape))


def run_case(rx, oracle, case):
    """the laid capture through an unfiltered context: check(), the laid edge list, the tile the layout assumes"""
    iq = S.lay(case)
    rx.rx(iq)
    lv, e = check(rx, 0, oracle_power(oracle, None, padded(iq, case.spb)), what=case.name)
    assert lv["tile_outputs"] == S.T, "the cases are laid for tiles of 1024 outputs"
    assert e.tolist() == S.edges_of_case(case), case.name
    assert rx.stats()["decimated_samples"] == case.n
    return lv, e


# ------------------------------------------------------------------------------------------ 1 - 6. no filter ----

@pytest.mark.parametrize("case", S.seam_cases(), ids=lambda c: c.name)
def test_seams(plain, oracle, case):
    lv, e = run_case(plain(case.n, case.spb), oracle, case)
    assert lv["tiles_total"] == -(-case.n // S.T) and case.n % S.T


@pytest.mark.parametrize("case", S.dense_cases(), ids=lambda c: c.name)
def test_dense(plain, oracle, case):
    lv, e = run_case(plain(case.n, case.spb), oracle, case)
    assert lv["num_runs"] >= case.n // 5 and lv["tiles_filtered"] == lv["tiles_total"] == 9


@pytest.mark.parametrize("case", S.on_throughout_cases(), ids=lambda c: c.name)
def test_tile_on_throughout_without_an_edge(plain, oracle, case):
    lv, e = run_case(plain(case.n, case.spb), oracle, case)
    assert lv["tiles_filtered"] == 1 + 2 + 1


@pytest.mark.parametrize("case,tiles", S.ballot_cases(), ids=lambda x: x.name if isinstance(x, S.Case) else "")
def test_ballot_ends(plain, oracle, case, tiles):
    lv, e = run_case(plain(case.n, case.spb), oracle, case)
    assert lv["tiles_filtered"] == len(tiles) and len(tiles) in (1, 2)
    assert lv["tiles_total"] == 130


@pytest.mark.parametrize("case", S.long_run_cases(), ids=lambda c: c.name)
def test_run_over_more_than_64_tiles(plain, oracle, case):
    lv, e = run_case(plain(case.n, case.spb), oracle, case)
    assert lv["num_runs"] == 1 and lv["tiles_filtered"] == 71
    top = np.float32(S.amplitude(0)) * np.float32(1.0 / 2048.0)
    assert lv["peaks"].tolist() == [top * top]


def test_four_runs_on_one_context(plain, oracle):
    """dense, sparse, empty, dense: nothing of an earlier answer or segment table survives"""
    runs = []
    for case in S.sequence_cases():
        lv, e = run_case(plain(case.n, case.spb), oracle, case)
        runs.append(lv["num_runs"])
    assert runs[0] == 4250 and runs[1] == 3 and runs[2] == 0 and runs[3] > 2800
    assert lv["hist"].sum() == runs[3]


# ------------------------------------------------------------------------------------------------ 7. 8-bit ----

@pytest.mark.parametrize("fmt", ["cs8", "cu8"])
def test_8bit_seams_equal_the_widened_capture(plain, oracle, fmt):
    for case in S.seam_cases():
        v = S.lay(case, S.AMP8)
        assert 0 <= v.min() and v.max() <= 127
        raw = v.astype(np.int8) if fmt == "cs8" else (v + 128).astype(np.uint8)
        wide = (v * 16).astype(np.int16)
        power = oracle_power(oracle, None, padded(wide, case.spb))
        rx8, rx16 = plain(case.n, case.spb, fmt), plain(case.n, case.spb)
        rx8.rx(raw)
        lv8, e8 = check(rx8, 0, power, what="%s %s" % (case.name, fmt))
        rx16.rx(wide)
        lv16, e16 = check(rx16, 0, power, what=case.name)
        assert e8.tolist() == e16.tolist() == S.edges_of_case(case)
        assert_same_bits(lv8["peaks"], lv16["peaks"])
        for key in ("num_runs", "tiles_total", "tiles_filtered", "tile_outputs"):
            assert lv8[key] == lv16[key], key
        assert lv8["hist"].tolist() == lv16["hist"].tolist()


# --------------------------------------------------------------------------------------- 8. slot parity ----

def test_batch_of_odd_and_even_lists(ok, oracle):
    import torch
    cases = S.parity_cases()
    caps, n, spb, stride = len(cases), S.PARITY_N, S.PARITY_SPB, S.PARITY_N + 500
    host = np.zeros((caps, 2 * stride), dtype=np.int16)
    host[:, 0::2] = 30000                                       # the gaps are loud
    iqs = [S.lay(c) for c in cases]
    for c in range(caps):
        host[c, :2 * n] = iqs[c]
    rx = ok.Receiver(None, None, max_samples=n, max_captures=caps, samples_per_buffer=spb, threshold=THR)
    dev_t = torch.from_numpy(host).cuda()
    rx.rx_device(dev_t.data_ptr(), n, num_captures=caps, stride=stride)
    for c in (4, 8, 0, 3, 7, 1, 6, 2, 5):
        lv, e = check(rx, c, oracle_power(oracle, None, padded(iqs[c], spb)), what="capture %d" % c)
        assert e.tolist() == S.edges_of_case(cases[c]) and e.size % 2 == S.PARITY[c] % 2 and lv["tile_outputs"] == S.T
    # a shorter run of two captures on the same context: both end on at their new last output
    m = S.PARITY_SHORT
    rx.rx_device(dev_t.data_ptr(), m, num_captures=2, stride=stride)
    for c in (1, 0):
        lv, e = check(rx, c, oracle_power(oracle, None, padded(iqs[c][:2 * m], spb)), what="short capture %d" % c)
        assert e.tolist() == S.edges_of_case(S.truncated(cases[c], m)) and e.size % 2 == 1
    with pytest.raises(ok.OokdError):
        rx.run_levels(2)
    rx.close()


# ------------------------------------------------------------------------ 9, 10. tiles narrower than a wave ----

@pytest.mark.parametrize("tile", sorted(S.NARROW_TAPS))
def test_narrow_tiles(ok, oracle, tile):
    iq, n, spb, targets = seam_narrow(oracle, tile)
    rx = ok.Receiver(lib_filter(ok, "narrow%d" % tile), None, max_samples=n, threshold=THR)
    rx.rx(iq)
    lv, e = check(rx, 0, oracle_power(oracle, oracle_fir(oracle, "narrow%d" % tile), padded(iq)), what="tile %d" % tile)
    assert lv["tile_outputs"] <= tile and lv["tile_outputs"] < 64
    assert_targets(e, n, targets)
    assert lv["num_runs"] == 4 and 0 < lv["tiles_filtered"] < lv["tiles_total"]
    rx.close()


def test_grid_stride(ok, oracle):
    """every workgroup walks at least two chunks: the segment table and the count of filtered tiles are reused"""
    import torch
    tile, caps = 4, S.GRID_CAPTURES
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    bound, n = S.grid_stride_samples(cus, tile)
    stride = n + 256
    fir = oracle_fir(oracle, "narrow4")
    contents = [S.grid_stride_capture(n, k) for k in range(S.GRID_CONTENTS)]
    power = [oracle_power(oracle, fir, c) for c in contents]
    host = np.zeros((caps, 2 * stride), dtype=np.int16)
    host[:, 0::2] = 30000
    for c in range(caps):
        host[c, :2 * n] = contents[S.grid_stride_content(c)]
    rx = ok.Receiver(lib_filter(ok, "narrow4"), None, max_samples=n, max_captures=caps, threshold=S.GRID_THR)
    dev_t = torch.from_numpy(host).cuda()
    rx.rx_device(dev_t.data_ptr(), n, num_captures=caps, stride=stride)
    lv = rx.run_levels(0)
    assert lv["tile_outputs"] <= tile
    chunks = -(-lv["tiles_total"] // 64)
    # launch_run_levels starts at most ceil(cus 8 / captures) workgroups per capture
    assert chunks >= 2 * bound and bound == -(-cus * 8 // caps), (chunks, bound, cus)
    filtered = []
    for c in range(caps):
        k = S.grid_stride_content(c)
        lv, e = check(rx, c, power[k], what="capture %d" % c)
        assert int(e[0]) < 64 * lv["tile_outputs"] and e.size == 5, (c, e)      # on in the first chunk and in the last
        assert lv["tiles_filtered"] == tiles_filtered_of(e, n, lv["tile_outputs"])
        filtered.append(lv["tiles_filtered"])
    assert len(set(filtered[:S.GRID_CONTENTS])) == S.GRID_CONTENTS
    rx.close()


# --------------------------------------------------------------------------------- 11, 12. filtered seams ----

@pytest.mark.parametrize("which", sorted(S.FILTERED_TARGETS))
@pytest.mark.parametrize("shape", sorted(S.SHAPE_D))
def test_filtered_seams(ok, oracle, shape, which):
    iq, n, spb, targets = seam_filtered(oracle, shape, which)
    rx = ok.Receiver(lib_filter(ok, shape), None, max_samples=n, samples_per_buffer=spb, threshold=THR)
    rx.rx(iq)
    lv, e = check(rx, 0, oracle_power(oracle, oracle_fir(oracle, shape), padded(iq, spb)), what="%s %s" % (shape, which))
    assert rx.stats()["decimated_samples"] == S.FILTERED_OUT and S.T % lv["tile_outputs"] == 0
    assert_targets(e, S.FILTERED_OUT, targets, shape)
    rx.close()


@pytest.mark.parametrize("which", sorted(S.FILTERED_TARGETS))
def test_tuned_seams(ok, which):
    f = lib_filter(ok, "fs32_fs4")
    iq, n, spb, targets, stages = seam_tuned(f, which)
    rx = ok.Receiver(f, None, max_samples=n, samples_per_buffer=spb, threshold=THR, tune=SEAM_NU)
    rx.rx(iq)
    lv, e = check(rx, 0, contract_power(padded(iq, spb), stages), what="tuned %s" % which)
    assert_targets(e, S.FILTERED_OUT, targets, "tuned")
    rx.close()


# ------------------------------------------------------------------------------------------- 13. cleaned lists ----

def _cleaned_and_raw(rx, c, power, deleted, what):
    raw, e_raw = check(rx, c, power, what=what + " raw")
    lv, e = check(rx, c, power, clean=True, what=what + " cleaned")
    assert e.tolist() == clean_of(e_raw, S.CLEAN_MIN_ON, 0)[0].tolist(), what
    assert e_raw.size - e.size == 2 * deleted and raw["num_runs"] - lv["num_runs"] == deleted, (what, e_raw.size, e.size)
    assert int(e_raw[-1]) > 2 * S.B
    check(rx, c, power, what=what + " raw again")
    return lv, e


@pytest.mark.parametrize("debounced", [False, True], ids=["clean_edges", "debounced-context"])
def test_cleaned_lists_of_a_batch(ok, oracle, debounced):
    import torch
    caps, n, stride = len(S.CLEAN_GLITCHES), S.CLEAN_N, S.CLEAN_STRIDE
    f, fir = lib_filter(ok, "fs32_fs4"), oracle_fir(oracle, "fs32_fs4")
    iqs = [S.clean_capture(c) for c in range(caps)]
    host = np.zeros((caps, 2 * stride), dtype=np.int16)
    host[:, 0::2] = 30000
    for c in range(caps):
        host[c, :2 * n] = iqs[c]
    rx = ok.Receiver(f, None, max_samples=n, max_captures=caps, threshold=THR, min_on=S.CLEAN_MIN_ON if debounced else 0)
    dev_t = torch.from_numpy(host).cuda()
    rx.rx_device(dev_t.data_ptr(), n, num_captures=caps, stride=stride)
    if not debounced:
        info = rx.clean_edges(S.CLEAN_MIN_ON, 0)
        assert [i["deleted"] for i in info] == [[0, g] for g in S.CLEAN_GLITCHES]
    for c in (2, 0, 3, 1):
        _cleaned_and_raw(rx, c, oracle_power(oracle, fir, padded(iqs[c])), S.CLEAN_GLITCHES[c], "capture %d" % c)
    rx.close()


def test_cleaned_lists_of_two_carriers(ok):
    nus = (SEAM_NU, -900e3 / RATE)
    f = lib_filter(ok, "fs32_fs4")
    parts = [moved(S.clean_capture(c), nu, scale=0.5).astype(np.int32) for c, nu in zip((2, 3), nus)]
    iq = np.clip(parts[0] + parts[1], -32768, 32767).astype(np.int16)
    n = iq.size // 2
    rx = ok.Receiver(f, None, max_samples=n, carriers=[nus[0], (nus[1], THR)], threshold=THR, min_on=S.CLEAN_MIN_ON)
    rx.rx(iq)
    for k, (c, nu) in enumerate(zip((2, 3), nus)):
        stages = lib_stages(f, nu)
        want = clean_of(edges_of(contract_rx(iq, stages, THR)[0]), S.CLEAN_MIN_ON, 0)[1]
        assert want == [0, S.CLEAN_GLITCHES[c]]
        _cleaned_and_raw(rx, k, contract_power(padded(iq), stages), S.CLEAN_GLITCHES[c], "carrier %d" % k)
    rx.close()
