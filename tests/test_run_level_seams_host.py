"""Every capture of tests/run_level_seams_inputs.py really has the property it was laid for -- proved on the reference
alone: the oracle's power and threshold (tests/run_levels_contract.py: ref_edges, peaks_of), or the tuned contract for
the tuned cases.  Nothing here asks the library's kernels anything; test_gpu_run_level_seams.py does."""
import numpy as np
import pytest

from tests import run_level_seams_inputs as S
from tests.clean_contract import clean_of
from tests.helpers import edges_of, golden_path
from tests.run_levels_contract import (SPB, THR, assert_targets, oracle_fir, padded, peaks_of, ref_edges, runs_of,
                                       seam_filtered, seam_narrow, seam_tuned, tiles_filtered_of)
from tests.test_survey_host import oracle_power

LAID = (S.seam_cases() + S.dense_cases() + S.on_throughout_cases() + [c for c, _ in S.ballot_cases()]
        + S.long_run_cases() + S.sequence_cases()[2:3] + S.parity_cases())


def _proved(oracle, case, scheme=S.AMP16, widen=1):
    """the designed edges are the reference's, the claims hold on them, and every run has one largest output, where
    the case says; -> (edges, power)"""
    iq = (S.lay(case, scheme) * widen).astype(np.int16)
    e = ref_edges(oracle, None, iq, case.spb)
    assert e.tolist() == S.edges_of_case(case), case.name
    assert_targets(e, case.n, [c if c[0] != "open" else ("open", case.n) for c in case.claims], case.name)
    power = oracle_power(oracle, None, padded(iq, case.spb))
    assert power.size == case.n
    runs = runs_of(e, case.n)
    assert len(runs) == len(case.runs)
    peaks = peaks_of(power, e, case.n)
    for (a, f), (_, _, at), top in zip(runs, case.runs, peaks):
        assert a <= at < f and power[at] == top and int((power[a:f] == top).sum()) == 1, (case.name, a, f, at)
    return e, power, peaks


@pytest.mark.parametrize("case", LAID, ids=lambda c: c.name)
def test_laid_cases_on_the_reference(oracle, case):
    e, power, peaks = _proved(oracle, case)
    # neighbouring runs differ, no peak repeats within a tile's worth of runs (512), and no run's smaller outputs
    # equal a neighbour's peak
    p = peaks.view(np.uint32).tolist()
    for r in range(len(p)):
        assert p[r] not in p[r + 1:r + 512], (case.name, r)
    i = S.lay(case)[0::2]
    assert not i.size or i.max() <= 2047 and (i[i != 0].min() >= 600 if i.any() else True)


def test_amplitudes():
    for scheme, top in ((S.AMP16, 2047), (S.AMP8, 127)):
        a = [S.amplitude(r, scheme) for r in range(2 * scheme[1])]
        assert len(set(a[:scheme[1]])) == scheme[1] and a[:scheme[1]] == a[scheme[1]:]
        assert all(x % 2 == 0 and scheme[0] <= x <= top for x in a)
    assert S.AMP16[1] > 512 and S.AMP16[0] - 1 >= 600
    assert (S.AMP8[0] - 1) * 16 > THR * 2048                      # the smallest 8-bit sample laid is on


def test_seam_cases_meet_every_seam():
    """every seam of the list is met by every layout that applies to it, and the capture has a partial last tile"""
    assert S.SEAM_N % S.T and S.SEAM_N > S.C + S.T and S.SEAM_N % S.SEAM_SPB == 0
    cases = S.seam_cases()
    assert len(cases) == sum(len(v) for v in S.LAYOUTS.values())
    by = {c.name: c for c in cases}
    for s in S.SEAMS:
        if s >= S.L:
            assert (("fall", s) if s < S.SEAM_N else ("open",)) in by["seams-ends-last"].claims
        if s < S.SEAM_N:
            assert ("rise", s) in by["seams-starts-first"].claims and ("rise", s) in by["seams-singles_on-first"].claims
        if 1 <= s < S.SEAM_N:
            assert ("rise", s - 1) in by["seams-pair-first"].claims and ("fall", s + 1) in by["seams-pair-last"].claims
        if s >= 1:
            assert ("rise", s - 1) in by["seams-singles_before-first"].claims
        if S.L <= s < S.SEAM_N:
            got = {v: [at for a, f, at in by["seams-across-" + v].runs if a < s < f] for v in S.LAYOUTS["across"]}
            assert got == {"first": [s - S.L], "last": [s + S.L - 1], "before": [s - 1], "behind": [s]}, s
    # the open runs: E is odd where a run ends the capture
    for name in ("seams-ends-first", "seams-ends-last", "seams-singles_before-first"):
        assert len(S.edges_of_case(by[name])) % 2 == 1, name


def test_dense_cases_fill_the_tiles():
    even, odd = S.dense_cases()[:2]
    assert S.DENSE_N >= 2 * S.T + 1 and S.DENSE_N % S.T
    for case in (even, odd):
        e = S.edges_of_case(case)
        per_tile = [len([a for a, f in runs_of(e, case.n) if t * S.T <= a < (t + 1) * S.T]) for t in range(2)]
        assert per_tile == [512, 512]                              # and 32 in every wave of 64 outputs
    # runs of 2 and 3: tiles that start on with an odd and with an even number of edges inside, and tiles that start off
    have = set()
    for case in S.dense_cases()[2:]:
        mine = {(on, inside & 1) for on, inside in S.tile_starts(S.edges_of_case(case), case.n)}
        assert {on for on, _ in mine} == {0, 1}, case.name         # both patterns have tiles that start on, and off
        have |= mine
    assert have == {(1, 0), (1, 1), (0, 0), (0, 1)}


def test_on_throughout_case():
    for case in S.on_throughout_cases():
        e = S.edges_of_case(case)
        starts = S.tile_starts(e, case.n)
        assert starts[1][0] == 0 and 2 * S.T - 1 not in range(*case.runs[0][:2])       # tile 1 ends off
        assert starts[2] == (1, 0) and 2 * S.T in e[0::2]           # the rise is AT tile 2's first output: not inside it
        assert not [x for x in e if 2 * S.T < x < 3 * S.T]          # no edge inside, and on throughout
        assert starts[3][0] == 1 and min(x for x in e if x > 3 * S.T) in e[1::2]       # tile 3's first edge is a fall
    at = [c.runs[1][2] for c in S.on_throughout_cases()]
    assert at == [2 * S.T, 3 * S.T + 299, 3 * S.T - 1, 3 * S.T]


def test_ballot_and_long_run_cases():
    assert S.BALLOT_N >= 2 * S.C + S.T and S.BALLOT_N % S.T
    seen = set()
    for case, tiles in S.ballot_cases():
        e = S.edges_of_case(case)
        on = sorted({j // S.T for a, f in runs_of(e, case.n) for j in range(a, f)})
        assert on == tiles and tiles_filtered_of(e, case.n, S.T) == len(tiles) in (1, 2), case.name
        seen.add(tuple(tiles))
    assert seen == {(0,), (64,), (63,), (127,), (63, 64)}
    a, f = S.LONG_RUN
    assert f // S.T - a // S.T + 1 > 64 and a // S.C == 0 and (f - 1) // S.C == 1
    tiles = [c.runs[0][2] // S.T for c in S.long_run_cases()]
    assert a // S.T in tiles and (f - 1) // S.T in tiles and any(a // S.T < t < 63 for t in tiles)
    assert [c.runs[0][2] for c in S.long_run_cases()][3:] == [a, f - 1, S.C - 1, S.C]


def test_parity_slots_are_disjoint():
    """[run_peak_base(lo_c, c), + ceil(E_c / 2)) of the nine captures, and of the two of the shorter run"""
    for cases in (S.parity_cases(), [S.truncated(c, S.PARITY_SHORT) for c in S.parity_cases()[:2]]):
        E = [len(S.edges_of_case(c)) for c in cases]
        if len(cases) == 9:
            assert [x % 2 if x else None for x in E] == [1, 1, 0, 1, None, 1, 1, 0, 1]
        lo, taken = 0, []
        for c, case in enumerate(cases):
            e = S.edges_of_case(case)
            if E[c] % 2:
                assert case.runs[-1][1] == case.n                   # it ends on at its last output
            if c and E[c - 1] % 2 and E[c]:
                assert e[0] == 0                                    # behind such a capture: on at output 0
            base = S.peak_base(lo, c)
            taken.append((base, base + (E[c] + 1) // 2))
            lo += E[c]
        for (a0, f0), (a1, f1) in zip(taken, taken[1:]):
            assert f0 <= a1, taken
        assert taken[-1][1] <= S.peak_slots(sum(E), len(cases)), taken
        # the rounding moves: both parities of lo + c occur among the captures that hold runs
        if len(cases) == 9:
            los = np.concatenate([[0], np.cumsum(E)[:-1]])
            assert {int(l + c) & 1 for c, l in enumerate(los) if E[c]} == {0, 1}
            # ... and a capture whose last slot is the one right below its neighbour's first
            assert any(f0 == a1 for (a0, f0), (a1, f1) in zip(taken, taken[1:]))


def test_parity_short_run_is_the_long_one_cut(oracle):
    for case in S.parity_cases()[:2]:
        iq = S.lay(case)[:2 * S.PARITY_SHORT]
        cut = S.truncated(case, S.PARITY_SHORT)
        e = ref_edges(oracle, None, iq, case.spb)
        assert e.tolist() == S.edges_of_case(cut) and e.size % 2 == 1


def test_8bit_seam_cases_on_the_reference(oracle):
    """the seam captures in 8-bit amplitudes, as the SC16Q11 capture of the same values (16 v)"""
    for case in S.seam_cases():
        v = S.lay(case, S.AMP8)
        assert v.max() <= 127 and v.min() >= 0
        _proved(oracle, case, S.AMP8, widen=16)


# ------------------------------------------------------------------------------------------- behind a filter ----

@pytest.mark.parametrize("tile", sorted(S.NARROW_TAPS))
def test_narrow_captures_on_the_reference(oracle, tile):
    iq, n, spb, targets = seam_narrow(oracle, tile)
    e = ref_edges(oracle, oracle_fir(oracle, "narrow%d" % tile), iq)
    assert_targets(e, n, targets)
    chunk = 64 * tile
    kinds = {(kind, j % chunk == 0) for kind, j in targets}
    assert all(j % tile == 0 for _, j in targets)
    assert kinds == {("rise", True), ("rise", False), ("fall", True), ("fall", False)}        # tile and chunk seams
    h = S.narrow_stages(tile)[0][1]
    assert h.dtype == np.float32 and abs(float(h.astype(np.float64).sum()) - 1.0) < 1e-4 and h.size == S.NARROW_TAPS[tile]


def test_grid_stride_captures_on_the_reference(oracle):
    """at 256 compute units and a tile of 4: every content is on in its first, a middle and its last chunk, and the
    batch's neighbours differ"""
    tile = 4
    bound, n = S.grid_stride_samples(256, tile)
    chunk = 64 * tile
    chunks = n // chunk
    assert bound == 32 and chunks >= 2 * bound and n % SPB == 0
    fir = oracle_fir(oracle, "narrow4")
    lists = []
    for k in range(S.GRID_CONTENTS):
        e = ref_edges(oracle, fir, S.grid_stride_capture(n, k), thr=S.GRID_THR)
        on = {j // chunk for a, f in runs_of(e, n) for j in (a, f - 1)}
        assert 0 in on and chunks - 1 in on and any(chunks // 4 < c < 3 * chunks // 4 for c in on), (k, e)
        lists.append(e.tolist())
    assert len({tuple(x) for x in lists}) == S.GRID_CONTENTS
    content = [S.grid_stride_content(c) for c in range(S.GRID_CAPTURES)]
    assert all(a != b for a, b in zip(content, content[1:])) and set(content) == set(range(S.GRID_CONTENTS))


@pytest.mark.parametrize("which", sorted(S.FILTERED_TARGETS))
@pytest.mark.parametrize("shape", sorted(S.SHAPE_D))
def test_filtered_seams_on_the_reference(oracle, shape, which):
    iq, n, spb, targets = seam_filtered(oracle, shape, which)
    assert n <= 200000 and n % spb == 0
    fir = oracle_fir(oracle, shape)
    assert fir.total_decimation == S.SHAPE_D[shape]
    e = ref_edges(oracle, fir, iq, spb)
    n_out = n // S.SHAPE_D[shape]
    assert n_out == S.FILTERED_OUT and n_out % S.T
    assert_targets(e, n_out, targets, shape)


def test_filtered_targets_cover_the_seams():
    assert len(S.DROPPED) <= 1
    want = {("rise", S.T), ("fall", S.T), ("rise", S.B), ("fall", S.B), ("rise", S.FILTERED_OUT - 1), ("open", S.FILTERED_OUT)}
    have = {t for ts in S.FILTERED_TARGETS.values() for t in ts}
    assert want <= have


@pytest.mark.parametrize("which", sorted(S.FILTERED_TARGETS))
def test_tuned_seams_on_the_contract(which):
    import ookiedokie_amd as ok
    from ookiedokie_amd import build as okbuild
    from tests.tuned_contract import contract_rx
    okbuild.build()
    f = ok.Filter.load(golden_path("filters", "fs32_fs4"))
    iq, n, spb, targets, stages = seam_tuned(f, which)
    e = edges_of(contract_rx(iq, stages, THR, spb)[0])
    assert_targets(e, n, targets)
    # the pulses sit on the carrier: the untuned filter does not see them
    assert iq[1::2].any()


# ------------------------------------------------------------------------------------------- cleaned lists ----

def test_clean_captures_on_the_reference(oracle):
    fir = oracle_fir(oracle, "fs32_fs4")
    assert len(set(S.CLEAN_GLITCHES)) == len(S.CLEAN_GLITCHES) and 0 in S.CLEAN_GLITCHES
    near_seam = 0
    for c, want in enumerate(S.CLEAN_GLITCHES):
        e = ref_edges(oracle, fir, S.clean_capture(c))
        assert int(e[-1]) > 2 * S.B                                 # more than two blocks of outputs
        cleaned, deleted = clean_of(e, S.CLEAN_MIN_ON, 0)
        assert deleted == [0, want], (c, deleted)
        gone = sorted(set(e.tolist()) - set(cleaned.tolist()))
        near_seam += sum(1 for x in gone if min(x % S.B, S.B - x % S.B) < 100)
    assert near_seam >= 4


def test_clean_carriers_on_the_contract():
    """captures 2 and 3 at half level on two carriers: each carrier's contract list loses its own glitches"""
    import ookiedokie_amd as ok
    from ookiedokie_amd import build as okbuild
    from tests.run_levels_contract import RATE, SEAM_NU
    from tests.tuned_contract import contract_rx, lib_stages, moved
    okbuild.build()
    f = ok.Filter.load(golden_path("filters", "fs32_fs4"))
    nus = (SEAM_NU, -900e3 / RATE)
    parts = [moved(S.clean_capture(c), nu, scale=0.5).astype(np.int32) for c, nu in zip((2, 3), nus)]
    iq = np.clip(parts[0] + parts[1], -32768, 32767).astype(np.int16)
    for c, nu in zip((2, 3), nus):
        e = edges_of(contract_rx(iq, lib_stages(f, nu), THR)[0])
        assert clean_of(e, S.CLEAN_MIN_ON, 0)[1] == [0, S.CLEAN_GLITCHES[c]] and int(e[-1]) > 2 * S.B
