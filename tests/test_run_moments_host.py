"""The pulse moments on the host (no GPU): ookd_run_moments_of and ookd_message_carriers against the numpy
restatement of their contract (tests/run_moments_contract.py), what the carrier estimate is worth on the contract
alone, and the proof, on the reference alone, that the seam captures of tests/run_moment_seams_inputs.py hold the
edges they are laid for."""
import numpy as np
import pytest

from tests import run_level_seams_inputs as S
from tests import run_moment_seams_inputs as M
from tests.helpers import edges_of, golden_path
from tests.run_levels_contract import RATE, SPB, THR, assert_targets, oracle_fir, padded, ref_edges, runs_of
from tests.run_moments_contract import (ONE, TWO_NU, TWO_TUNE, message_carriers_of, moments_of, moved_seam, oracle_y, q, terms_of,
                                        two_carrier_capture)


@pytest.fixture(scope="module")
def ok():
    from ookiedokie_amd import build as okbuild
    okbuild.build()
    import ookiedokie_amd as okm
    okm.lib()
    return okm


def same_moments(ok, y, edges, what=""):
    y = np.ascontiguousarray(y, dtype=np.float32).reshape(-1, 2)
    got = ok.run_moments_of(y, edges)
    want = moments_of(y, edges, y.shape[0])
    for k, key in enumerate(("power", "lag_re", "lag_im")):
        assert got[key].dtype == np.int64 and got[key].tolist() == want[:, k].tolist(), (what, key)
    return want


def random_edges(rng, n_out, count):
    count = min(count, n_out)
    return np.sort(rng.choice(n_out, size=count, replace=False)).astype(np.uint64)


# ------------------------------------------------------------------------------------------------------- T1 ----

def test_q_of_the_restatement():
    """ties to even, the clamp, a NaN: what every other comparison here rests on"""
    h = 2.0 ** -30
    assert q(np.float32([0.5 * h, 1.5 * h, 2.5 * h, -0.5 * h, -1.5 * h, -2.5 * h])).tolist() == [0, 2, 2, 0, -2, -2]
    assert q(np.float32([1.0, -1.0, 2.0 ** -7, 2.0 ** 32, 1e30, -1e30, np.inf, -np.inf, np.nan])).tolist() == \
        [1 << 30, -(1 << 30), 1 << 23, 1 << 62, 1 << 62, -(1 << 62), 1 << 62, -(1 << 62), 0]


def test_run_moments_of_random(ok):
    rng = np.random.default_rng(5)
    for trial in range(40):
        n_out = int(rng.integers(1, 400))
        scale = (1.0, 1e-4, 30.0)[trial % 3]
        y = (rng.standard_normal((n_out, 2)) * scale).astype(np.float32)
        e = random_edges(rng, n_out, int(rng.integers(0, 40)))
        want = same_moments(ok, y, e, "trial %d" % trial)
        assert want.shape[0] == (e.size + 1) // 2
        if trial % 3 == 0 and want.shape[0] > 3:
            assert (want[:, 1] < 0).any() or (want[:, 2] < 0).any()          # negative products occur
    # neighbouring runs of one output and an open last run of one output
    y = rng.standard_normal((9, 2)).astype(np.float32)
    want = same_moments(ok, y, [0, 1, 2, 3, 8], "singles")
    assert (want[:, 1:] == 0).all() and (want[:, 0] > 0).all()              # a run of one output has lag 0


def test_run_moments_of_designed(ok):
    h = np.float32(2.0 ** -30)
    # E = 0
    got = ok.run_moments_of(np.ones((5, 2), np.float32), [])
    assert got["power"].size == 0 and got["lag_re"].size == 0
    got = ok.run_moments_of(np.zeros((0, 2), np.float32), [])
    assert got["power"].size == 0
    # an open last run, to n_out
    y = np.array([[0, 0], [1, 0], [0, 1], [-1, 0], [0, -1]], np.float32)
    want = same_moments(ok, y, [1], "open")
    assert want.tolist() == [[4 << 30, 0, 3 << 30]]                         # a quarter turn per output
    want = same_moments(ok, y[::-1].copy(), [0, 4], "the other way round")
    assert want.tolist() == [[4 << 30, 0, -(3 << 30)]]
    # q's ties to even in the lag term: zr = v * 1 + 0 * 0
    for v, r in ((0.5, 0), (1.5, 2), (2.5, 2), (-0.5, 0), (-1.5, -2), (-2.5, -2), (3.5, 4)):
        y = np.array([[1, 0], [np.float32(v) * h, 0]], np.float32)
        want = same_moments(ok, y, [0], "tie %g" % v)
        assert want[0, 1] == r and want[0, 2] == 0, (v, want)
    # ... and in the power: 2^-32 + 2^-32 = half a step, 2^-30 + 2^-31 = a step and a half
    a, b = np.float32(2.0 ** -16), np.float32(2.0 ** -15)
    assert same_moments(ok, np.array([[a, a]], np.float32), [0])[0, 0] == 0
    c = np.float32(np.sqrt(np.float32(2.0 ** -31)))
    y = np.array([[b, c]], np.float32)
    same_moments(ok, y, [0], "power tie")
    # the clamp, an infinity, a NaN
    big = np.float32(1e10)
    y = np.array([[big, 0], [big, 0], [-big, 0], [np.inf, 1], [np.nan, 1], [1, np.nan], [1, 1]], np.float32)
    want = same_moments(ok, y, [0], "clamp")
    assert want[0, 0] == 1 << 31                    # four terms at the clamp are 2^64 = 0, two NaN are 0, and 2.0
    for e in ([0, 2], [1, 3], [2, 4], [3, 5], [4, 6], [5]):
        same_moments(ok, y, e, "clamp %s" % e)
    same_moments(ok, y, [0, 1, 2, 3, 4, 5, 6], "clamp singles")
    # a wrap modulo 2^64: eight outputs at the clamp are 2^65 = 0, three are -2^62
    y = np.tile(np.array([[big, 0]], np.float32), (8, 1))
    assert same_moments(ok, y, [0], "wrap 8").tolist() == [[0, (7 << 62) % (1 << 64) - (1 << 64), 0]]
    assert same_moments(ok, y, [0, 3], "wrap 3").tolist() == [[-(1 << 62), -(1 << 63), 0]]


def test_run_moments_of_refusals(ok):
    y = np.ones((8, 2), np.float32)
    for e in ([3, 3], [4, 2], [8], [0, 9]):
        with pytest.raises(ok.OokdError) as err:
            ok.run_moments_of(y, e)
        assert err.value.code == -1 and "ascend" in str(err.value)
    e = np.array([1, 5], np.uint64)
    out = np.zeros((2, 3), np.int64)
    lib = ok.lib()
    assert lib.ookd_run_moments_of(y.ctypes.data, 8, e.ctypes.data, 2, out.ctypes.data, 2) == -1      # R != ceil(E / 2)
    assert lib.ookd_run_moments_of(y.ctypes.data, 8, None, 2, out.ctypes.data, 1) == -1
    assert lib.ookd_run_moments_of(None, 8, e.ctypes.data, 2, out.ctypes.data, 1) == -1
    assert lib.ookd_run_moments_of(y.ctypes.data, 8, e.ctypes.data, 2, None, 1) == -1
    assert lib.ookd_run_moments_of(y.ctypes.data, 8, e.ctypes.data, 2, out.ctypes.data, 1) == 0


# ------------------------------------------------------------------------------------------------------- T2 ----

def same_carriers(ok, edges, moments, msg, pulses, D, nu, n_out, what=""):
    got = ok.message_carriers(edges, moments, msg, pulses, D, nu, n_out)
    want = message_carriers_of(edges, moments, msg, pulses, D, nu, n_out)
    assert got["outputs"].dtype == np.uint64 and got["outputs"].tolist() == [w[3] for w in want], what
    for k, key in enumerate(("carrier", "mean_power", "coherence")):
        assert got[key].dtype == np.float64
        assert got[key] == pytest.approx([w[k] for w in want], rel=1e-12, abs=1e-15), (what, key)
    return got


@pytest.mark.parametrize("D", [1, 4])
def test_message_carriers_against_the_restatement(ok, D):
    rng = np.random.default_rng(17 + D)
    for trial in range(30):
        n_out = int(rng.integers(50, 3000))
        e = random_edges(rng, n_out, int(rng.integers(0, 60)))
        R = (e.size + 1) // 2
        mo = rng.integers(-(1 << 45), 1 << 45, size=(R, 3))
        mo[:, 0] = np.abs(mo[:, 0]) + (1 << 45)
        msg = np.sort(rng.integers(0, n_out, size=int(rng.integers(0, 6)))).astype(np.uint64)
        nu = float(rng.uniform(-0.5, 0.5))
        got = same_carriers(ok, e, mo, msg, int(rng.integers(1, 9)), D, nu, n_out, "trial %d" % trial)
        # the branch nearest nu
        assert (np.abs(got["carrier"] - nu) <= 0.5 / D + 1e-12).all()
    # the same through the dict Receiver.run_moments returns
    y = rng.standard_normal((64, 2)).astype(np.float32)
    e = [3, 20, 30, 64 - 5]
    d = ok.run_moments_of(y, e)
    a = ok.message_carriers(e, d, [40], 2, D, 0.1, 64)
    b = ok.message_carriers(e, moments_of(y, e, 64), [40], 2, D, 0.1, 64)
    assert a["carrier"].tolist() == b["carrier"].tolist() and a["outputs"].tolist() == [17 + 29]


@pytest.mark.parametrize("D", [1, 4])
def test_message_carriers_of_a_tone(ok, D):
    """y advances by 2 pi f D per output whatever nu is: a tone at f read back near a context tuned beside it, and an
    open last run counted up to n_out"""
    n_out, f, nu = 600, 0.2031 / D, 0.2 / D
    j = np.arange(n_out)
    y = np.stack([0.7 * np.cos(2 * np.pi * f * D * j), 0.7 * np.sin(2 * np.pi * f * D * j)], axis=1).astype(np.float32)
    e = [10, 200, 300, 450, 500]
    mo = ok.run_moments_of(y, e)
    got = same_carriers(ok, e, mo, [250, 599], 4, D, nu, n_out, "tone")
    assert got["outputs"].tolist() == [190, 250]
    assert np.abs(got["carrier"] - f).max() < 1e-6 / D
    assert np.abs(got["mean_power"] - 0.49).max() < 1e-6 and (got["coherence"] > 0.99).all() and (got["coherence"] < 1.0).all()
    # a context tuned a whole 1 / D away reads the alias nearest to itself
    far = same_carriers(ok, e, mo, [250], 4, D, nu + 1.0 / D, n_out, "alias")
    assert abs(far["carrier"][0] - (f + 1.0 / D)) < 1e-6 / D


def test_message_carriers_no_pair_and_refusals(ok):
    # runs of one output: no pair -> carrier = nu, coherence = 0, the mean power stays
    y = np.full((8, 2), 0.5, np.float32)
    e = [1, 2, 4, 5]
    mo = ok.run_moments_of(y, e)
    got = same_carriers(ok, e, mo, [6], 5, 4, -0.125, 8, "no pair")
    assert got["carrier"].tolist() == [-0.125] and got["coherence"].tolist() == [0.0]
    assert got["mean_power"].tolist() == [0.5] and got["outputs"].tolist() == [2]
    # a message without a run
    got = same_carriers(ok, e, mo, [0, 6], 5, 1, 0.25, 8, "no run")
    assert got["outputs"].tolist() == [0, 2] and got["carrier"][0] == 0.25 and got["mean_power"][0] == 0.0
    # all power zero
    got = same_carriers(ok, e, np.zeros((2, 3), np.int64), [6], 5, 1, 0.0, 8, "zero")
    assert got["coherence"].tolist() == [0.0] and got["mean_power"].tolist() == [0.0]
    for args, text in ((([1, 2, 4, 5], mo, [6], 0, 1, 0.0, 8), "pulses"),
                       (([1, 2, 4, 5], mo, [6], 3, 0, 0.0, 8), "decimation"),
                       (([1, 2, 4, 5], mo, [6, 5], 3, 1, 0.0, 8), "ascend"),
                       (([1, 2, 4], mo, [6], 3, 1, 0.0, 4), "n_out"),
                       (([1, 2, 4, 5, 6], mo, [6], 3, 1, 0.0, 8), "on-runs")):
        with pytest.raises(ok.OokdError) as err:
            ok.message_carriers(*args)
        assert err.value.code == -1 and text in str(err.value), text
    lib = ok.lib()
    e = np.array([1, 2], np.uint64)
    assert lib.ookd_message_carriers(None, 2, 8, np.zeros(3, np.int64).ctypes.data, 1, None, 0, 1, 1, 0.0, None) == -1
    assert lib.ookd_message_carriers(e.ctypes.data, 2, 8, None, 1, None, 0, 1, 1, 0.0, None) == -1
    assert lib.ookd_message_carriers(e.ctypes.data, 2, 8, np.zeros(3, np.int64).ctypes.data, 1, None, 1, 1, 1, 0.0, None) == -1
    assert lib.ookd_message_carriers(e.ctypes.data, 2, 8, np.zeros(3, np.int64).ctypes.data, 1, None, 0, 1, 1, 0.0, None) == 0


# ------------------------------------------------------------------------------------------------------- T3 ----

WORST = {}


@pytest.mark.parametrize("filt", ["fs32_fs4", "fs128_fs16_dec4"])
def test_two_transmitters_6_khz_apart_on_the_contract(ok, oracle, vectors, filt):
    """What the estimate is worth, on the float32 contract alone (no GPU): golden G1 at +600 kHz at nominal level, then
    G1 at +606 kHz at 1/4 level, both with a DC term of 300+200j and +-40 LSB of noise, through a context tuned to
    603 kHz.  Every decoded message's carrier lies within 1.5 kHz of its own transmitter -- a quarter of the spacing
    the case is built to resolve -- and its coherence is at least 0.99.

    The worst error of a message's carrier this contract shows (Hz), by filter and level:
        fs32_fs4           nominal 1.5     1/4 level 62.8
        fs128_fs16_dec4    nominal 8.2     1/4 level 7.7
    and the lowest coherence 0.99896 (fs128_fs16_dec4, 1/4 level)."""
    from tests.tuned_contract import contract_rx, lib_stages
    from tests.tuned_survey_contract import oracle_device
    g, iq, half = two_carrier_capture(vectors)
    f = ok.Filter.load(golden_path("filters", filt))
    D = f.total_decimation
    d = ok.Device.load(golden_path("devices", g["device"]), RATE // D)
    bits, y = contract_rx(iq, lib_stages(f, TWO_TUNE), THR)
    n_out = bits.size
    e = edges_of(bits).astype(np.uint64)
    msg, _, errs = oracle.sm_stream(oracle_device(oracle, g["device"], D), bits, SPB // D)
    assert msg.size == 6 and errs.size == 0, (msg, errs)
    mo = ok.run_moments_of(y, e)
    want = moments_of(y, e, n_out)
    assert mo["power"].tolist() == want[:, 0].tolist() and mo["lag_re"].tolist() == want[:, 1].tolist() \
        and mo["lag_im"].tolist() == want[:, 2].tolist()
    got = same_carriers(ok, e, mo, msg, d.num_bits + 2, D, TWO_TUNE, n_out, filt)
    own = np.where(msg < half // D, TWO_NU[0], TWO_NU[1])
    assert own.tolist() == [TWO_NU[0]] * 3 + [TWO_NU[1]] * 3
    err_hz = np.abs(got["carrier"] - own) * RATE
    print("%s: carrier errors %s Hz, coherence %s" % (filt, np.round(err_hz, 2).tolist(), np.round(got["coherence"], 5).tolist()))
    assert (err_hz <= 1500.0).all(), err_hz
    assert (got["coherence"] >= 0.99).all(), got["coherence"]
    # the mean power is the transmitter's level: within 1.5 of its nominal on power (0.95 scale)^2
    level = np.where(msg < half // D, 0.95 ** 2, (0.95 * 0.25) ** 2)
    assert (got["mean_power"] / level > 1 / 1.5).all() and (got["mean_power"] / level < 1.5).all()


# ------------------------------------------------------------------------------------------------------- T4 ----

LAID = M.seam_cases() + M.dense_cases() + [M.long_run_case()] + S.parity_cases()


@pytest.mark.parametrize("case", LAID, ids=lambda c: c.name)
def test_hashed_cases_on_the_reference(oracle, case):
    """the laid edges are the reference's, and neighbouring terms of a run differ"""
    iq = M.lay_hashed(case)
    e = ref_edges(oracle, None, iq, case.spb)
    assert e.tolist() == S.edges_of_case(case), case.name
    rail = np.abs(iq.astype(np.int64))
    assert not rail.any() or (rail.max() <= 2047 and rail[rail != 0].min() >= M.MIN_RAIL)
    qp, qr, qi = terms_of(oracle_y(oracle, None, padded(iq, case.spb)))
    for a, f in runs_of(e, case.n):
        if f - a >= 3:
            assert (np.diff(qp[a:f]) != 0).mean() > 0.95 and (np.diff(qr[a + 1:f]) != 0).mean() > 0.9, (case.name, a, f)


def test_hashed_8bit_cases_on_the_reference(oracle):
    for case in M.seam_cases():
        v = M.lay_hashed(case, M.MIN_RAIL8, M.SPAN8)
        assert np.abs(v).max() <= 120
        e = ref_edges(oracle, None, (v * 16).astype(np.int16), case.spb)
        assert e.tolist() == S.edges_of_case(case), case.name


def test_hashed_cases_hold_the_moments_seams():
    """S1 .. S6, S9, S10 by the layouts' own claims (tests/test_run_level_seams_host.py proves the catalogue); here: the
    layouts the moments need are all present, and the batch of S8 has a capture that ends on in front of one that
    begins on"""
    names = {c.name for c in M.seam_cases()}
    assert names == {"seams-%s-first" % k for k in S.LAYOUTS}
    by = {c.name: c for c in M.seam_cases()}
    for s in (S.T, 2 * S.T, S.B, 2 * S.B, S.C):
        assert ("rise", s) in by["seams-starts-first"].claims                          # S2
        assert ("rise", s - 1) in by["seams-pair-first"].claims                        # S4
        assert ("fall", s) in by["seams-ends-first"].claims                            # S3: a fall at j0
        singles = [a for a, f, _ in by["seams-singles_before-first"].runs]
        assert s - 1 in singles and s not in singles                                   # S3: on at j0 - 1, off at j0
        assert any(a < s < f for a, f, _ in by["seams-across-first"].runs)             # S1, S6
    assert ("rise", 0) in by["seams-starts-first"].claims                              # S5
    cases = S.parity_cases()
    ends_on = [len(S.edges_of_case(c)) % 2 == 1 for c in cases]
    begins_on = [bool(c.runs) and c.runs[0][0] == 0 for c in cases]
    assert any(a and b for a, b in zip(ends_on, begins_on[1:]))                        # S8
    a, f, _ = M.long_run_case().runs[0]
    assert (f - 1) // S.T - a // S.T + 1 > 64                                          # S10


def test_open_pad_capture_on_the_reference(oracle):
    """S7: the last run is open through the zero padding up to n_out, and n is no multiple of the buffer"""
    iq, n, spb = M.open_pad_capture()
    assert n % spb == spb - M.PAD
    fir = oracle_fir(oracle, "fs32_fs4")
    e = ref_edges(oracle, fir, iq, spb)
    n_out = -(-n // spb) * spb
    assert n_out == n + M.PAD and n_out % S.T
    assert e.size == 3 and int(e[0]) < S.T < int(e[1]) and int(e[2]) < n        # one run across a tile seam, one open
    y = oracle_y(oracle, fir, padded(iq, spb))
    assert y.shape[0] == n_out and (y[n:, 0] ** 2 + y[n:, 1] ** 2 >= THR * THR).all()
    qp, qr, qi = terms_of(y)
    assert (np.diff(qp[int(e[2]):]) != 0).all()


@pytest.mark.parametrize("which", sorted(S.FILTERED_TARGETS))
@pytest.mark.parametrize("shape", sorted(S.SHAPE_D))
def test_moved_seams_on_the_reference(oracle, shape, which):
    """behind a filter: the turning pulses' edges sit on a tile seam, on a block seam and at the capture's end, and
    both rails of the filter's output move inside every run"""
    iq, n, spb, targets = moved_seam(oracle, shape, which)
    fir = oracle_fir(oracle, shape)
    e = ref_edges(oracle, fir, iq, spb)
    assert n // S.SHAPE_D[shape] == S.FILTERED_OUT and n % spb == 0 and iq[1::2].any()
    assert_targets(e, S.FILTERED_OUT, targets, shape)
    qp, qr, qi = terms_of(oracle_y(oracle, fir, padded(iq, spb)))
    for a, f in runs_of(e, S.FILTERED_OUT):
        if f - a >= 3:
            assert (np.diff(qp[a:f]) != 0).mean() > 0.9 and (qi[a + 1:f] != 0).mean() > 0.9, (shape, a, f)
