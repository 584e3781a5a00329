"""The debounced decode on the GPU (ookd_rx_set_debounce): the clean pass in the run's chain, its per-block
prefix (clean.hip: clean_block_prefix_kernel), the level from the list (kernels.hpp: fsm_level_at) and the state machine
on the cleaned view in every form.  The reference everywhere is the CPU oracle's state machine on the bit stream painted
from the cleaned list (tests/debounce_contract.py); the cleaned list itself is held against tests/clean_contract.py fed
with the run's own `rx.edges(c)`.  Every comparison is equality."""
import numpy as np
import pytest

from tests import dense_devices as dd
from tests.clean_contract import clean_of, info_of
from tests.debounce_contract import cleaned, decode_cleaned
from tests.debounce_inputs import FULL, GRID, PART, glitched_burst_runs
from tests.helpers import golden_path
from tests.pulse_contract import RATE, SPB, THR, assert_same_hist, golden_iq, hist_of
from tests.symbol_contract import assert_same_survey, survey_of
from tests.test_gpu_clean import ROLES, T, TABLE, capture_of, random_capture
from tests.test_gpu_dense_results import _batch
from tests.test_gpu_parity import _sync_walk_forced
from tests.tuned_contract import golden_capture, moved

pytestmark = pytest.mark.gpu

B = 4096                        # outputs of an edge block (kBlockWords * 64): the grain of the per-block prefix
BURST = dd.burst(8)             # pulses of 20 us, gaps of 20 / 50 us, at 1 Msps: one sample per microsecond
DSPB = GRID                     # samples_per_buffer of the designed streams: a segment of the round form is 64 samples


@pytest.fixture(scope="module")
def ok():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from ookiedokie_amd import build as okbuild
    okbuild.build()
    import ookiedokie_amd as okm
    okm.lib()
    return okm


def same_decode(rx, got, fsm, mins, buf_len, tag, captures=1):
    """the run's messages, payloads, error count and every error position against the reference on the cleaned lists of
    the run's own edge lists; returns (messages, errors) of the reference"""
    n_out = got.stats["decimated_samples"]
    per_cap, total = [], 0
    for c in range(captures):
        m, p, errs = decode_cleaned(fsm, rx.edges(c), n_out, mins, buf_len)
        gc = got.for_capture(c) if captures > 1 else got
        assert list(gc.msg_samples) == m.tolist(), (tag, c, mins)
        assert gc.payloads.shape == p.shape and (gc.payloads == p).all(), (tag, c, mins)
        per_cap.append(errs.tolist())
        total += m.size
    errs_want = sum(per_cap, [])                    # capture-major
    errs, nerr = rx.errors(len(errs_want) + 8)
    assert nerr == len(errs_want) == got.stats["num_errors"], (tag, mins, nerr, len(errs_want))
    if captures > 1 and got.stats["fsm_path"] == 3:
        # (the contract of ookd_rx_get_errors: the errors of the captures the scan refused follow all the others')
        orders = [sum([per_cap[c] for c in range(captures) if not (r >> c) & 1], []) +
                  sum([per_cap[c] for c in range(captures) if (r >> c) & 1], []) for r in range(1, 1 << captures)]
        assert list(errs) in orders, (tag, mins)
    else:
        assert list(errs) == errs_want, (tag, mins)
    assert total == len(got.msg_samples), (tag, mins)
    return total, len(errs_want)


def same_lists(rx, mins, tag, captures=1):
    """the cleaned list the chain made, and what the clean readers and the counts say about it, with no clean_edges
    call in front; then clean_edges with the same minimums, which launches nothing"""
    n_out = rx.stats()["decimated_samples"]
    assert rx.clean_kernel_ms == 0.0, tag
    for c in range(captures):
        e = rx.edges(c)
        want = clean_of(e, *mins)[0]
        got = rx.edges(c, clean=True)
        assert got.dtype == np.uint64 and got.tolist() == want.tolist(), (tag, c, e.size, got.size, want.size)
        assert_same_hist(rx.pulse_hist(c, clean=True), hist_of(want, n_out), "%s capture %d" % (tag, c))
        assert_same_hist(rx.pulse_hist(c), hist_of(e, n_out), "%s capture %d, the run's own" % (tag, c))
        assert_same_survey(rx.symbol_survey(TABLE, ROLES, c, clean=True), survey_of(want, TABLE, ROLES), "%s %d" % (tag, c))
    infos = rx.clean_edges(*mins)
    assert infos == [info_of(rx.edges(c), *mins) for c in range(captures)], tag
    assert rx.clean_kernel_ms == 0.0, tag
    assert rx.stats()["num_edges"] == sum(rx.edges(c).size for c in range(captures)), tag


# ------------------------------------------------------------------------ 1. the per-block prefix ----

def _layouts():
    """name -> (closed runs, lead): edge lists around the block boundary, with the minimums (5, 5)"""
    rng = np.random.default_rng(23)
    out = {
        # edges at 4095, 4096, 4097: a chain of two short runs across the boundary leaves its last edge, 4097
        "4095_4096_4097": ([1, 1, 30, 40, 30], B - 1),
        # ... kept: every run is long enough
        "4095_kept": ([7, 9, 30], B - 1),
        "4096_kept": ([7, 9, 30], B),
        "4097_kept": ([7, 9, 30], B + 1),
        # a deleted gap 4094 .. 4098 and a deleted pulse 2 * 4096 - 2 .. + 2: both straddle a boundary
        "straddling_gap": ([14, 4, 30, 2 * B - 2 - (B + 2 + 30), 4, 60, 30], B - 2 - 14),
        # blocks without an edge, raw and cleaned, and blocks whose only edges are deleted
        "empty_blocks": ([20, 3 * B, 20, 2, 20, 2 * B + 5, 3, B + 1, 30, 40, 3 * B], 100),
        # nothing is left: an odd chain of short runs vanishes
        "all_deleted": ([2, 3, 2, 4, 1], B - 3),
        "one_edge": ([], 2 * B),
    }
    for E in (T - 1, T, T + 1, 2 * T + 1):
        out["E=%d" % E] = (rng.integers(1, 12, size=E - 1), int(rng.integers(0, 9)))
    return out


LAYOUTS = _layouts()


def test_block_prefix_layouts(ok, oracle):
    """no filter: every layout on a context without a device (the lists and their readers) and, with burst(8) behind
    it, in the round form with a segment every 64 samples and in the scan -- every segment start asks the prefix for its
    first edge and fsm_level_at for its level"""
    mins = (5, 5)
    n = -(-(12 * (2 * T + 2)) // SPB) * SPB
    fsm = dd.fsm_desc(oracle, BURST)
    d = dd.ok_device(ok, BURST)
    plain = ok.Receiver(None, None, max_samples=n, threshold=THR, edge_capacity=n, min_on=mins[0], min_off=mins[1])
    assert plain.debounce == mins
    kw = dict(max_samples=n, threshold=THR, edge_capacity=n, samples_per_buffer=DSPB, message_slots=64, min_on=mins[0],
              min_off=mins[1])
    rounds = ok.Receiver(None, d, fsm_rounds=True, quiet_skip=False, segment_buffers=1, **kw)
    scan = ok.Receiver(None, d, **kw)
    for name, (closed, lead) in LAYOUTS.items():
        iq, want_e = capture_of(np.asarray(closed, dtype=np.int64), lead=lead)
        plain.rx(iq)
        assert plain.edges(0).tolist() == want_e.tolist(), name
        same_lists(plain, mins, name)
        for leg, rx in (("rounds", rounds), ("scan", scan)):
            got = rx.rx(iq)
            assert rx.edges(0).tolist() == want_e.tolist(), (name, leg)
            same_decode(rx, got, fsm, mins, DSPB, (name, leg))
            assert got.stats["fsm_path"] in ((2,) if leg == "rounds" else (1, 3)), (name, leg, got.stats)
            assert rx.edges(0, clean=True).tolist() == clean_of(want_e, *mins)[0].tolist(), (name, leg)
    assert plain.edges(0, clean=True).size == 2 * T + 1 - 2 * sum(info_of(want_e, *mins)["deleted"])
    for rx in (plain, rounds, scan):
        rx.close()
    d.close()


def test_block_prefix_in_a_batched_run(ok, oracle):
    """three captures with different edge counts in one run: [T + 1 random edges, all deleted, edges around 4096]"""
    import torch
    mins = (5, 5)
    rng = np.random.default_rng(29)
    n = -(-(12 * (T + 2)) // SPB) * SPB
    parts = [random_capture(T + 1, rng, n=n), capture_of(np.asarray(LAYOUTS["all_deleted"][0]), lead=B - 3, n=n),
             capture_of(np.asarray(LAYOUTS["straddling_gap"][0]), lead=LAYOUTS["straddling_gap"][1], n=n)]
    host = np.stack([p[0] for p in parts])
    dev_t = torch.from_numpy(host).cuda()
    torch.cuda.synchronize()
    fsm = dd.fsm_desc(oracle, BURST)
    d = dd.ok_device(ok, BURST)
    kw = dict(max_samples=n, max_captures=3, threshold=THR, edge_capacity=3 * (T + 64), min_on=mins[0], min_off=mins[1])
    plain = ok.Receiver(None, None, **kw)
    plain.rx_device(dev_t.data_ptr(), n, num_captures=3)
    for c in range(3):
        assert plain.edges(c).tolist() == parts[c][1].tolist(), c
    same_lists(plain, mins, "batch", captures=3)
    assert [plain.edges(c, clean=True).size for c in range(3)][1] == 0
    plain.close()
    for leg, extra in (("rounds", dict(fsm_rounds=True, quiet_skip=False, segment_buffers=1)), ("scan", dict())):
        rx = ok.Receiver(None, d, samples_per_buffer=DSPB, message_slots=64, **kw, **extra)
        got = rx.rx_device(dev_t.data_ptr(), n, num_captures=3)
        same_decode(rx, got, fsm, mins, DSPB, ("batch", leg), captures=3)
        rx.close()
    d.close()


# ------------------------------------------------------------------------ 2. decode on every leg ----

LEGS = (("default", dict()), ("tables", dict(scan_tables=True)), ("sims", dict(scan_sims=True)),
        ("rounds", dict(fsm_rounds=True, quiet_skip=False, segment_buffers=1)))


@pytest.mark.parametrize("leg", [name for name, _ in LEGS])
def test_decode_on_every_leg(ok, oracle, leg):
    """the designed stream at the minimums (8, 3), where every glitch goes and the decode is the unglitched stream's,
    and at (3, 0), where the pulses of 7 and the dropouts stay and cost errors; the walk forced"""
    runs, plain = glitched_burst_runs()
    iq, iq_plain = dd.iq_of(runs), dd.iq_of(plain)
    n = -(-(iq.size // 2) // DSPB) * DSPB
    fsm = dd.fsm_desc(oracle, BURST)
    want_plain = oracle.rx(iq_plain, None, dd.THR, fsm, DSPB)
    assert len(want_plain.msg_samples) == 40
    d = dd.ok_device(ok, BURST)
    kw = dict(LEGS)[leg]
    with _sync_walk_forced(True):
        rx = ok.Receiver(None, d, max_samples=n, threshold=dd.THR, samples_per_buffer=DSPB, message_slots=64,
                         min_on=FULL[0], min_off=FULL[1], **kw)
    got = rx.rx(iq)
    msgs, nerr = same_decode(rx, got, fsm, FULL, DSPB, leg)
    assert list(got.msg_samples) == list(want_plain.msg_samples) and (got.payloads == want_plain.payloads).all()
    assert (msgs, nerr) == (40, len(want_plain.err_samples))
    assert got.stats["fsm_path"] == (2 if leg == "rounds" else 1), (leg, got.stats)
    assert got.stats["pipeline_chunks"] == 0
    rx.set_debounce(*PART)
    assert rx.debounce == PART
    got = rx.rx(iq)
    msgs2, nerr2 = same_decode(rx, got, fsm, PART, DSPB, leg)
    print("debounce leg %-8s (8, 3): %d messages %d errors; (3, 0): %d messages %d errors, fsm_path %d reason %d"
          % (leg, msgs, nerr, msgs2, nerr2, got.stats["fsm_path"], got.stats["fsm_fallback_reason"]))
    assert (msgs2, nerr2) != (msgs, nerr)
    assert got.stats["fsm_path"] in ((2,) if leg == "rounds" else (1, 3)), (leg, got.stats)
    assert rx.edges(0, clean=True).tolist() == cleaned(rx.edges(0), PART).tolist()
    rx.close()
    d.close()


# ------------------------------------------------------------- 3. a deleted gap that holds quiet tiles ----

def test_a_deleted_gap_with_quiet_tiles(ok, oracle, vectors):
    """through fs32_fs4: two pulses of 150 outputs, the gap between them G = 5000 outputs from 50 in front of a block
    boundary, min_off above G and below G1's own gaps (5997) -- the block [2 * 4096, 3 * 4096), whole quiet tiles of the
    front end, lies inside the deleted gap, and the round form's segments of 2048 outputs start at 2 * 4096 + 2048 and
    3 * 4096, inside it.  The machine sees one long pulse, then G1's messages."""
    f = ok.Filter.load(golden_path("filters", "fs32_fs4"))
    dec = f.total_decimation
    rate = RATE // dec
    G = 5000
    first = 2 * B - 50 - 150
    head = np.zeros(2 * dec * (first + 150 + G + 150 + 3 * B), dtype=np.int16)
    for a in (first, first + 150 + G):
        head[2 * dec * a:2 * dec * (a + 150):2] = dd.AMP
    g1 = golden_iq(vectors, "G1")
    iq = np.concatenate([head, g1])
    n = iq.size // 2
    fsm = oracle.load_device_json(golden_path("devices", "p3l-nexa2012"), rate)[0]
    d = ok.Device.load(golden_path("devices", "p3l-nexa2012"), rate)
    mins = (0, G + 500)
    alone = ok.Receiver(f, d, max_samples=n, threshold=THR)
    want_g1 = alone.rx(g1)
    alone.close()
    assert len(want_g1.msg_samples) > 0
    for leg, kw in (("rounds", dict(fsm_rounds=True, segment_buffers=1)), ("scan", dict())):
        rx = ok.Receiver(f, d, max_samples=n, threshold=THR, min_off=mins[1], **kw)
        got = rx.rx(iq)
        raw, kept = rx.edges(0), rx.edges(0, clean=True)
        assert raw.size - kept.size == 2 and kept[0] == raw[0] and kept[1] == raw[3]    # one pulse over the gap
        assert raw[1] < 2 * B and raw[2] > 3 * B and raw[2] - raw[1] < mins[1]
        msgs, nerr = same_decode(rx, got, fsm, mins, SPB // dec, leg)
        # G1 lies whole buffers behind: its messages, that much later
        shift = (head.size // 2) // dec
        assert (got.msg_samples - shift).tolist() == want_g1.msg_samples.tolist(), leg
        assert got.stats["fsm_path"] == (2 if leg == "rounds" else 1), (leg, got.stats)
        rx.close()
    d.close()


# ------------------------------------------------------------------------------ 4. refused captures ----

def _stretch_runs(nmsg=30, seed=77):
    """burst(8) with, in one 50 us gap, seven pulses of 2 us one sample apart from 25 us on (outside both bit windows) --
    fourteen edges on which nothing fires, deeper than the scan's stuck codes hold (tests/test_gpu_dense_results.py:
    _refused_burst_capture, whose pulses are 1 us) -- and a pulse of 1 us in every fourth pause"""
    runs = dd.burst_runs(8, nmsg, seed=seed)
    at = next(i for i in range(2, len(runs)) if runs[i] == 50 and runs[i - 1] == 20 and i > 200)
    runs[at:at + 1] = [25] + [2, 1] * 6 + [2] + [50 - 25 - 20]
    return _with_single_glitches(runs)


def _with_single_glitches(runs):
    out, k = [], 0
    for i, r in enumerate(runs):
        if i and i % 2 == 0 and r >= 230:
            k += 1
            if k % 4 == 0:
                out += [r - 41, 1, 40]
                continue
        out.append(r)
    return out


def test_refused_capture_is_redone_on_the_cleaned_view(ok, oracle):
    import torch
    fsm = dd.fsm_desc(oracle, BURST)
    d = dd.ok_device(ok, BURST)
    caps = [dd.iq_of(_with_single_glitches(dd.burst_runs(8, 40, seed=810))), dd.iq_of(_stretch_runs()),
            dd.iq_of(_with_single_glitches(dd.burst_runs(8, 40, seed=811)))]
    host, n, stride = _batch(caps)
    dev_t = torch.from_numpy(host).cuda()
    torch.cuda.synchronize()
    rx = ok.Receiver(None, d, max_samples=n, max_captures=3, threshold=dd.THR, message_capacity=256, min_on=2)
    # min_on = 2, not above the stretch's pulses of 2 (the comparison is strict): the stretch stays, the scan refuses that capture alone, and the
    # round form redoes it on the cleaned view (the pulses of 1 us are gone from every capture)
    got = rx.rx_device(dev_t.data_ptr(), n, num_captures=3, stride=stride)
    assert got.stats["fsm_path"] == 3 and got.stats["fsm_fallback_reason"] != 0, got.stats
    total, _ = same_decode(rx, got, fsm, (2, 0), 8192, "stretch kept", captures=3)
    assert total == 40 + 30 + 40
    assert all(rx.edges(c, clean=True).size < rx.edges(c).size for c in range(3))
    # min_on = 5, above it: the stretch vanishes and the scan keeps every capture
    rx.set_debounce(5, 0)
    got = rx.rx_device(dev_t.data_ptr(), n, num_captures=3, stride=stride)
    assert got.stats["fsm_path"] == 1 and got.stats["fsm_fallback_reason"] == 0, got.stats
    total, nerr = same_decode(rx, got, fsm, (5, 0), 8192, "stretch deleted", captures=3)
    assert (total, nerr) == (110, 0)
    rx.close()
    d.close()


# ---------------------------------------------------------------------------------- 5. other runs ----

@pytest.mark.parametrize("filt", ["fs32_fs4", "fs128_fs16_dec4"])
def test_synthetic_capture_keeps_its_messages(ok, filt):
    """2^24 samples at 3 Msps, seed 5, p3l-nexa2012 with pauses of 4 .. 20 ms and a glitch ahead of every eighth
    message, made on the GPU: 37 messages and no error with min_on = 250 us -- the messages of the capture without
    glitches -- and 34 with 60 errors on the same context with the debounce off (tests/test_debounce_host.py pins both
    for the reference)"""
    import torch
    n = 1 << 24
    f = ok.Filter.load(golden_path("filters", filt))
    rate = RATE // f.total_decimation
    min_on = int(250e-6 * rate)
    d = ok.Device.load(golden_path("devices", "p3l-nexa2012"), RATE)
    dd_ = ok.Device.load(golden_path("devices", "p3l-nexa2012"), rate)
    cap = torch.empty(2 * n + 64, dtype=torch.int16, device="cuda")
    rx = ok.Receiver(f, dd_, max_samples=n, threshold=THR, min_on=min_on)
    seen = {}
    for glitch_every in (0, 8):
        syn = ok.Synth(d, n, seed=5, sample_rate=RATE, gap_us=(4000, 20000), glitch_every=glitch_every)
        syn.fill_device(cap.data_ptr())
        torch.cuda.synchronize()
        syn.close()
        seen[glitch_every] = rx.rx_device(cap.data_ptr(), n)
        assert rx.clean_kernel_ms == 0.0
    plain, deb = seen[0], seen[8]
    assert (len(deb.msg_samples), deb.stats["num_errors"]) == (37, 0)
    assert list(deb.msg_samples) == list(plain.msg_samples) and (deb.payloads == plain.payloads).all()
    assert deb.stats["num_edges"] > plain.stats["num_edges"] and deb.stats["pipeline_chunks"] == 0
    assert rx.edges(0, clean=True).size == plain.stats["num_edges"]
    rx.set_debounce(0, 0)
    raw = rx.rx_device(cap.data_ptr(), n)
    assert (len(raw.msg_samples), raw.stats["num_errors"]) == (34, 60)
    with pytest.raises(ok.OokdError) as e:
        rx.edges(0, clean=True)
    assert "no cleaned list of the last run" in str(e.value)
    rx.close()
    d.close()
    dd_.close()


def test_carriers_are_the_tuned_contexts(ok):
    nu1, nu2 = 600e3 / RATE, -900e3 / RATE
    g1, _ = golden_capture("G1")
    g2, _ = golden_capture("G2")
    ext = np.zeros_like(g1)
    ext[:g2.size] = g2
    z = moved(g1, nu1, scale=0.5).astype(np.int32) + moved(ext, nu2, 400.0 * (1 + 0.5j), 40, seed=11, scale=0.5).astype(np.int32)
    iq = np.clip(z, -32768, 32767).astype(np.int16)
    n = iq.size // 2
    f = ok.Filter.load(golden_path("filters", "fs32_fs4"))
    d = ok.Device.load(golden_path("devices", "p3l-nexa2012"), RATE // f.total_decimation)
    carriers = [(nu1, 0.1), (nu2, 0.12)]
    for mins in ((200, 0), (1600, 1700)):       # nothing of the captures is short / G1's pulses and G2's short gaps are
        rx = ok.Receiver(f, d, max_samples=n, carriers=carriers, min_on=mins[0], min_off=mins[1])
        got = rx.rx(iq)
        errs, nerr = rx.errors()
        seen_errs = []
        for k, (nu, thr) in enumerate(carriers):
            one = ok.Receiver(f, d, max_samples=n, threshold=thr, tune=nu, min_on=mins[0], min_off=mins[1])
            alone = one.rx(iq)
            gk = got.for_capture(k)
            assert list(gk.msg_samples) == list(alone.msg_samples) and (gk.payloads == alone.payloads).all(), (mins, k)
            seen_errs += one.errors()[0].tolist()
            assert one.edges(0).tolist() == rx.edges(k).tolist()
            assert one.edges(0, clean=True).tolist() == rx.edges(k, clean=True).tolist() == \
                clean_of(rx.edges(k), *mins)[0].tolist(), (mins, k)
            one.close()
        assert errs.tolist() == seen_errs and nerr == len(seen_errs), mins
        if mins == (200, 0):
            assert len(got.for_capture(0).msg_samples) > 0
        rx.close()
    d.close()


def test_two_debounced_contexts_in_flight(ok, oracle):
    import torch
    runs, _ = glitched_burst_runs()
    other, _ = glitched_burst_runs(nmsg=30, seed=9)
    fsm = dd.fsm_desc(oracle, BURST)
    d = dd.ok_device(ok, BURST)
    iqs = [dd.iq_of(runs), dd.iq_of(other)]
    n = max(-(-(x.size // 2) // DSPB) * DSPB for x in iqs)
    devs = []
    for x in iqs:
        h = np.zeros(2 * n, dtype=np.int16)
        h[:x.size] = x
        devs.append(torch.from_numpy(h).cuda())
    torch.cuda.synchronize()
    ctx = [ok.Receiver(None, d, max_samples=n, threshold=dd.THR, samples_per_buffer=DSPB, message_slots=64, min_on=FULL[0],
                       min_off=FULL[1]) for _ in iqs]
    alone = []
    for rx, t in zip(ctx, devs):
        r = rx.rx_device(t.data_ptr(), n)
        alone.append((r, rx.errors()[0].tolist()))
    for rx, t in zip(ctx, devs):
        rx.submit_device(t.data_ptr(), n)
    with pytest.raises(ok.OokdError) as e:
        ctx[0].set_debounce(4, 4)
    assert e.value.code == -1 and "in flight" in str(e.value)
    for rx in ctx:
        rx.wait()
    for k, rx in enumerate(ctx):
        got = rx.result()
        assert rx.debounce == FULL
        assert list(got.msg_samples) == list(alone[k][0].msg_samples) and (got.payloads == alone[k][0].payloads).all()
        assert rx.errors()[0].tolist() == alone[k][1]
        same_decode(rx, got, fsm, FULL, DSPB, "in flight %d" % k)
        assert rx.edges(0, clean=True).tolist() == cleaned(rx.edges(0), FULL).tolist()
        rx.close()
    d.close()


# ------------------------------------------------------------------- 6. refusals and the off state ----

def test_refusals_and_the_off_state(ok, oracle, vectors):
    import torch
    g = vectors["G1"]
    giq = golden_iq(vectors, "G1")
    n = giq.size // 2
    f = ok.Filter.load(golden_path("filters", g["filter"]))
    d = ok.Device.load(golden_path("devices", g["device"]), RATE // f.total_decimation)
    dev_t = torch.from_numpy(giq).cuda()
    torch.cuda.synchronize()
    # shards
    rx = ok.Receiver(f, d, max_samples=n, threshold=THR, min_on=200)
    with pytest.raises(ok.OokdError) as e:
        rx.shard_begin(dev_t.data_ptr(), n, None, True, None)
    assert e.value.code == -1 and "debounce" in str(e.value)
    with pytest.raises(ok.OokdError) as e:
        rx.shard_refine(ok.FsmState())
    assert e.value.code == -1 and "debounce" in str(e.value)
    rx.set_debounce(1, 1)                                       # off: the context takes shards again
    rx.shard_begin(dev_t.data_ptr(), n, None, True, None)
    rx.close()
    # a debounced context never chunks
    never = ok.Receiver(f, d, max_samples=n)
    want = never.rx(giq)
    assert len(want.msg_samples) > 0 and never.debounce == (0, 0)
    chunked = ok.Receiver(f, d, max_samples=n, pipeline_chunk_samples=4 * SPB)
    assert chunked.rx(giq).stats["pipeline_chunks"] >= 2        # (otherwise the next lines show nothing)
    chunked.set_debounce(200, 0)
    got = chunked.rx(giq)
    assert got.stats["pipeline_chunks"] == 0
    assert list(got.msg_samples) == list(want.msg_samples) and (got.payloads == want.payloads).all()
    assert chunked.edges(0, clean=True).tolist() == chunked.edges(0).tolist()      # nothing of G1 is that short
    chunked.close()
    # off: no cleaned list, and the results of a context never given minimums
    for mins in ((0, 0), (1, 0), (1, 1)):
        rx = ok.Receiver(f, d, max_samples=n, min_on=mins[0], min_off=mins[1])
        rx.set_debounce(*mins)
        assert rx.debounce == mins
        got = rx.rx(giq)
        with pytest.raises(ok.OokdError) as e:
            rx.edges(0, clean=True)
        assert e.value.code == -1 and "no cleaned list of the last run" in str(e.value)
        assert list(got.msg_samples) == list(want.msg_samples) and (got.payloads == want.payloads).all()
        ga, wa = dict(got.stats), dict(want.stats)
        for key in ("fir_kernel_ms", "total_device_ms"):
            ga.pop(key), wa.pop(key)
        assert ga == wa, mins
        assert rx.edges(0).tolist() == never.edges(0).tolist()
        rx.close()
    never.close()
    d.close()


def test_set_debounce_after_a_clean_by_hand(ok):
    """run, clean_edges, set_debounce: the setter replaces the small buffers the hand-made list lay in by the chain's,
    sized by the capacity -- the run has no cleaned list any more (not whatever the new buffers hold), until the next"""
    iq, want_e = capture_of(np.asarray(LAYOUTS["E=%d" % (T + 1)][0], dtype=np.int64), lead=LAYOUTS["E=%d" % (T + 1)][1])
    n = iq.size // 2
    rx = ok.Receiver(None, None, max_samples=n, threshold=THR, edge_capacity=n)
    rx.rx(iq)
    infos = rx.clean_edges(4, 6)
    by_hand = rx.edges(0, clean=True)
    assert infos == [info_of(want_e, 4, 6)] and by_hand.tolist() == clean_of(want_e, 4, 6)[0].tolist()
    assert by_hand.size > 0 and rx.clean_kernel_ms > 0.0
    rx.pulse_hist(0, clean=True)
    rx.set_debounce(5, 5)
    for call in (lambda: rx.edges(0, clean=True), lambda: rx.pulse_hist(0, clean=True),
                 lambda: rx.symbol_survey(TABLE, ROLES, 0, clean=True)):
        with pytest.raises(ok.OokdError) as e:
            call()
        assert e.value.code == -1 and "no cleaned list of the last run" in str(e.value)
    assert rx.clean_kernel_ms == 0.0
    assert rx.edges(0).tolist() == want_e.tolist()                       # the run's own list is what it was
    # a clean by hand answers the old run again, in the chain's buffers; the next run makes its own list
    assert rx.clean_edges(4, 6) == infos and rx.edges(0, clean=True).tolist() == by_hand.tolist()
    rx.set_debounce(5, 5)                                               # nothing to replace now: the list stays
    assert rx.edges(0, clean=True).tolist() == by_hand.tolist()
    rx.rx(iq)
    same_lists(rx, (5, 5), "after a clean by hand")
    rx.close()


def test_c_example_takes_each_minimum_for_its_own_level(ok, vectors, tmp_path):
    """examples/ookd_rx.c on G1 behind a 100 us pulse: --min-on-us deletes the pulse and reports it as min_on,
    --min-off-us deletes no pulse; the printed messages are those of Receiver(min_on=...)"""
    import subprocess
    from tests.test_host import _build_c_example
    exe = _build_c_example(tmp_path)
    g1 = golden_iq(vectors, "G1")
    head = np.zeros(2 * 8192, dtype=np.int16)
    head[2 * 4000:2 * 4300:2] = dd.AMP
    iq = np.concatenate([head, g1])
    cap = tmp_path / "glitch.sc16q11"
    iq.tofile(str(cap))
    f = ok.Filter.load(golden_path("filters", "fs32_fs4"))
    rate = RATE // f.total_decimation
    m = int(250e-6 * rate)
    d = ok.Device.load(golden_path("devices", "p3l-nexa2012"), rate)
    rx = ok.Receiver(f, d, max_samples=iq.size // 2, threshold=THR, min_on=m)
    want = rx.rx(iq)
    info = rx.clean_edges(m, 0)[0]
    assert info["deleted"] == [0, 1] and len(want.msg_samples) > 0
    rx.close()
    d.close()
    args = [str(cap), golden_path("devices", "p3l-nexa2012"), golden_path("filters", "fs32_fs4"), str(RATE), "csv"]
    on = subprocess.run([exe, "--min-on-us", "250"] + args, capture_output=True, text=True, timeout=120)
    assert on.returncode == 0, on.stderr
    assert "debounce %d / 0 samples: 1 pulses and 0 gaps deleted, %d edges decoded" % (m, info["edges_out"]) in on.stderr, on.stderr
    assert len(on.stdout.strip().split("\n")) == 1 + len(want.msg_samples)
    off = subprocess.run([exe, "--min-off-us", "250"] + args, capture_output=True, text=True, timeout=120)
    assert off.returncode == 0, off.stderr
    assert "debounce 0 / %d samples: 0 pulses and 0 gaps deleted, %d edges decoded" % (m, info["edges_in"]) in off.stderr, off.stderr
    both = subprocess.run([exe, "--min-off-us", "100", "--min-on-us", "250"] + args, capture_output=True, text=True, timeout=120)
    assert both.returncode == 0 and "debounce %d / " % m in both.stderr and " samples: 1 pulses and 0 gaps" in both.stderr, both.stderr
    fields = lambda text: [ln.split(",", 1)[1] for ln in text.strip().split("\n")]      # (the first is the wall clock)
    assert fields(both.stdout) == fields(on.stdout)
    plain = subprocess.run([exe] + args, capture_output=True, text=True, timeout=120)
    assert plain.returncode == 0 and "debounce" not in plain.stderr
