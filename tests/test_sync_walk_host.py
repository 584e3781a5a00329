"""CPU-side checks of tests/sync_walk_inputs.py (no GPU): every case holds what test_gpu_sync_walk.py needs it to hold.
The builder put each silence and hold on the leaf the case names; the restatement of "sync leaf" -- the oracle's state
machine poked into every entry code -- finds a sync leaf there and none inside the dense stretches; the regions have
the distance, tail, length, split the case is named for; whether the walk holds is the case's expected form; and the
oracle decodes messages in every region, with payloads that tell a wrong entry code from the right one."""
import ctypes as C

import numpy as np
import pytest

from tests import dense_devices as dd
from tests import sync_walk_inputs as sw
from tests.helpers import edges_of

import ookiedokie_amd as ok
from ookiedokie_amd import build as okbuild


@pytest.fixture(scope="module")
def depth():
    """LTab::depth of burst(8), as tests/test_host.py::test_scan_domain_of_the_shipped_devices derives it"""
    okbuild.build()
    ok.lib()
    d = dd.ok_device(ok, sw.DEVICE)
    out = (C.c_uint32 * 8)()
    assert ok.lib().ookd_scan_domain_info(d._h, 4096, 1, out) == 0
    built, _, _, _, nstuck, _, domain, states = list(out)
    d.close()
    base = states * (sw.DEVICE["max_bits"] + 2) + 3
    depth = (domain - base) // nstuck
    assert built == 1 and domain == base + depth * nstuck and 1 <= depth <= sw.MAX_STUCK_DEPTH
    return depth


def test_the_cases_cover_the_depth_the_tables_have(depth):
    """the stuck cases are named for distances 1 .. MAX_STUCK_DEPTH + 1: depth and depth + 1 are among them"""
    assert {depth, depth + 1} <= set(sw.STUCK_D)
    assert {d for _, d in sw.ACROSS} == {depth, depth + 1}
    assert len(set(sw.NAMES)) == len(sw.NAMES)


def test_the_closure_of_entry_codes(oracle):
    """burst(8): a low leaf is entered in reset, idle or off with 0 .. 7 bits, a high one in reset, idle or on with
    0 .. 8 -- `off` is never entered at the high level but stuck"""
    rs = sw.restatement(oracle, sw.DEVICE)
    names = sw.DEVICE["state_names"]
    assert {names[s] for s, _ in rs.reach[0]} == {"reset", "idle", "off"}
    assert {names[s] for s, _ in rs.reach[1]} == {"reset", "idle", "on"}
    assert {nb for s, nb in rs.reach[1] if names[s] == "on"} == set(range(9))


def test_building_blocks(oracle):
    """what the module's docstring says of a silence, a hold, a dense leaf, a stuck stretch and a short pulse"""
    rs = sw.restatement(oracle, sw.DEVICE)
    on, idle = sw.DEVICE["state_names"].index("on"), sw.DEVICE["state_names"].index("idle")
    far = 10 ** 6
    image, stuck, skips = rs.leaf_info(0, sw.SILENCE - 1, far)
    assert image == {("n", on, 0)} and not stuck and skips == (("skip", 0), ("skip", 1))
    assert len(sw.candidates(rs.leaf_info(0, sw.SILENCE - 1, far))) == 3
    assert len(sw.candidates(rs.leaf_info(0, sw.SILENCE - 1, 100))) == 1        # a buffer boundary inside
    image, stuck, _ = rs.leaf_info(1, sw.HOLD - 1, far)
    assert image == {("n", idle, 0)} and not stuck
    for L, n in ((1, 19), (0, 19), (0, 49)):
        info = rs.leaf_info(L, n, far)
        assert len(info[0]) >= 9 and not info[1] and sw.candidates(info) is None
    for n in (24, 0):                   # the low leaves of a stuck stretch
        assert rs.leaf_info(0, n, far)[1]
    assert not rs.leaf_info(1, 0, far)[1]           # its pulses: entered in `on` an error, in `idle` nothing
    image, stuck, _ = rs.leaf_info(1, sw.SHORT_PULSE - 1, far)
    assert image == {("skip", 0), ("n", idle, 0)} and not stuck


def test_candidate_counts_over_every_leaf_of_the_family(oracle):
    """Over every (level, length, place of the buffer boundary) the restatement knows for burst(8) and gated(8): sync
    leaves with 1, 2, 3 and 4 candidates exist, and none whose image of at most three plus its skip results makes five
    -- an image holds a skip code only through an error on the leaf's last sample, and both skip results then end the
    same way or go on dropping.  (the fifth candidate stays without a case.)"""
    for dev in (sw.DEVICE, dd.gated(8)):
        rs = sw.restatement(oracle, dev)
        counts, five = set(), 0
        for L in (0, 1):
            for n in list(range(0, 60)) + list(range(195, 206)):
                for off in sorted({0, 1, n // 2, n, n + 1}):
                    info = rs.leaf_info(L, n, off)
                    c = sw.candidates(info)
                    if c is not None:
                        counts.add(len(c))
                    elif 1 <= len(info[0]) <= 3 and all(e[0] in ("n", "skip") for e in list(info[0]) + list(info[2])):
                        five += 1
        assert counts == {1, 2, 3, 4} and five == 0, (dev["name"], counts, five)


def _regions_by_block(a):
    return {r.block: r for r in a.regions}


@pytest.mark.parametrize("name", sw.NAMES)
def test_case(oracle, depth, name):
    c = sw.case(name)
    an = sw.analysed(oracle, c, depth)
    streams = sw.streams(c)
    od = dd.fsm_desc(oracle, sw.DEVICE)
    assert len(an) == len(streams) and all(s.size % c.spb == 0 for s in streams)
    assert max(s.size for s in streams) <= 4200000 and max(a.ne for a in an) <= 140000
    errors_placed = c.meta.get("errors", []) if c.kind == "single" else []
    for k, (a, stream) in enumerate(zip(an, streams)):
        e = edges_of(stream)
        assert a.ne == e.size
        laid = [s for cap, s in c.syncs if cap == k]
        dirty = [s for cap, s in c.dirty if cap == k]
        # the builder put each silence and hold on the leaf the case names
        for s in laid + dirty:
            want = sw.SILENCE if s % 2 == 0 else sw.HOLD
            if s == c.meta.get("s") and name.startswith("nc_"):
                want = 201
            if s in c.meta.get("stretched", ()):        # (a silence made longer to move a buffer's end)
                assert want <= e[s] - e[s - 1] < want + c.spb
                want = e[s] - e[s - 1]
            assert e[s] - e[s - 1] == want and stream[e[s] - 1] == s % 2, (name, k, s)
        # ... the restatement finds a sync leaf there, a leaf of the shape but no sync leaf where a stuck stretch is
        # too close, and no other one but a short pulse: none inside the dense stretches
        found = set(np.nonzero(a.sync)[0].tolist())
        assert set(laid) <= found, (name, k, sorted(set(laid) - found))
        assert all(a.shaped[s] and not a.sync[s] for s in dirty), (name, k)
        assert found - set(laid) <= set(errors_placed), (name, k, sorted(found - set(laid)))
        assert all(a.first_sync[b] is None or b == 0 or a.sync[sw.leaf_at(b, a.first_sync[b])] for b in range(a.nblk))
        # every region holds a message the oracle decodes (one long enough for one), and payloads differ
        want = oracle.rx(dd.iq_of(stream), None, dd.THR, od, c.spb, msg_cap=1 << 17)
        ms = np.asarray(want.msg_samples, np.int64)
        for r in a.regions:
            if r.length >= 3 * sw.MSG_LEAVES and not errors_placed:
                lo, hi = e[r.first - 1], e[min(r.first + r.length - 1, a.ne - 1)]
                assert ((ms > lo) & (ms <= hi)).any(), (name, k, r)
        if a.ne > 3 * sw.MSG_LEAVES:
            assert len(ms) >= 1
            distinct = len({bytes(p) for p in want.payloads})
            assert distinct >= min(len(ms), 200) * 0.6, (name, distinct, len(ms))
        if not errors_placed:
            assert len(want.err_samples) == 0, (name, k)
    # whether the walk holds is the form the case expects
    assert sw.expected_form(oracle, c, depth) == c.form, (name, [a.holds for a in an])
    a, reg = an[-1] if name == "batch_small" else an[0], None
    by = _regions_by_block(a)
    if name.startswith("split_"):
        split = int(name[6:])
        assert by[2].split == split and by[2].first == sw.leaf_at(2, split) and a.nblk == 6
        if split == 64:
            assert sw.block_lane(by[2].first) == (3, 0)
    elif name == "second_sync_in_block":
        assert by[1].split == 11 and a.sync[sw.leaf_at(1, 41)] and by[1].dist == 1
        assert by[1].first < sw.leaf_at(1, 41) < by[1].first + by[1].length       # walked through
    elif name.startswith("run_"):
        assert by[1].dist == int(name[4:]) and a.nblk <= 12
        assert all(r.tail <= sw.SYNC_MAX_RUN for r in a.regions if r.dist is None)
    elif name.startswith("tail_"):
        p = name.split("_")
        assert a.regions[-1].block == 1 and a.regions[-1].tail == int(p[1]) and a.nblk <= 12
        last = (a.ne - 1) - sw.LB * (a.nblk - 1)
        assert last == (int(p[2][4:]) if len(p) > 2 else 30)
    elif name.startswith("first_block_only_"):
        assert len(a.regions) == 1 and a.nblk == int(name[17:]) and a.regions[0].length == a.ne - 1
    elif name.startswith("len_"):
        assert by[1].length == int(name[4:]) and by[1].split == 21
    elif name.startswith("stuck_") and name != "stuck_inside_region":
        m = c.meta
        (first, x, last), = m["stuck"]
        assert x == m["x"] and m["s"] - x == m["d"]
        # of the stretch's leaves the low ones can end stuck, x is the last of them, and no other leaf of the capture can;
        # the last inert edge is that of the pulse behind x (entered stuck, it ends stuck: `off` has no falling edge)
        assert set(np.nonzero(a.stuckable)[0].tolist()) == set(range(first, x + 1, 2))
        bx, lx = sw.block_lane(x)
        bs, ls = sw.block_lane(m["s"])
        if "across" in name:
            assert bs == bx + 1 and lx >= sw.LB - depth and ls <= depth
        else:
            assert bs == bx
        assert a.shaped[m["s"]] and a.sync[m["s"]] == (m["d"] > depth)
        if m["alone"]:
            assert a.holds == (m["d"] > depth) and a.nblk == 12
            assert [r.block for r in a.regions] == ([0, 1, bs, 10] if m["d"] > depth else [0, 1, 10])
        else:
            # the silence further on in s's block is the region start when s is none
            assert by[bs].split == (ls + 1 if m["d"] > depth else 42 if "across" in name else 56)
    elif name == "stuck_inside_region":
        assert [last - first for first, _, last in c.meta["stuck"]] == [2, 4, 2 * (depth // 2)]
        for first, x, last in c.meta["stuck"]:
            assert by[1].first < first and last < by[1].first + by[1].length
        assert len(a.regions) == 3
    elif name.startswith("error_"):
        at, = c.meta["errors"]
        s = c.meta["s"]
        e = edges_of(streams[0])
        want = oracle.rx(dd.iq_of(streams[0]), None, dd.THR, od, c.spb)
        assert list(want.err_samples) == [e[at]]                # the short pulse's falling edge, and no other error
        boundary = (int(e[at]) // c.spb + 1) * c.spb
        if name == "error_pulse_starts_region":
            assert a.sync[at] and sw.block_lane(by[2].first - 1) == sw.block_lane(at) and boundary > e[s] + 1
        else:
            assert by[1].first < at < by[1].first + by[1].length and not a.first_sync[1] == sw.block_lane(at)[1]
            assert by[2].first == s + 1
        if name == "error_in_region":
            assert e[at] < boundary < e[s - 8]
        elif name == "error_on_sync_leaf":
            assert e[s - 1] + 1 < boundary <= e[s] and a.nc[s] == 1
        elif name == "error_across_regions":
            assert boundary > e[s] + 1 and a.nc[s] == 3
    elif name.startswith("nc_"):
        s = c.meta["s"]
        assert a.nc[s] == c.meta["nc"] and by[2].first == s + 1
    elif name.startswith("pick_"):
        per, seams = sw.pick_seams(a.nblk)
        if name == "pick_wave_seam":
            assert a.nblk <= 1024 and by[60].dist == 8 and by[126].dist == 1 and by[127].dist == 4
            seams = [64, 128]
        else:
            assert a.nblk == int(name[5:]) and per == {1023: 1, 1024: 1, 1025: 2, 2049: 3}[a.nblk]
            assert (-(-a.nblk // per) < sw.PICK_THREADS) == (a.nblk in (1023, 1025, 2049))     # threads without blocks
            assert 64 * per in seams and (a.nblk < 2049 or {512 * per, 1024} <= set(seams))
        dists = [r.dist for r in a.regions if r.dist is not None]
        assert max(dists) == sw.SYNC_MAX_RUN and sum(3 <= d <= sw.SYNC_MAX_RUN for d in dists) >= 0.9 * len(dists)
        for S in seams:         # a region that starts in front of block S (another thread's, another wave's) and ends behind
            assert any(r.dist is not None and r.block < S < r.block + r.dist for r in a.regions), (name, S)
        assert set(a.nc[a.sync].tolist()) >= {1, 3}
        # the regions across the seams (and the last one) start in a candidate that is not the first: their sync leaf
        # lies wholly in the dropped rest of a buffer, it ends in the skip code it was entered in, and that is no code
        # of its image -- the candidates are the image, then the skip results.  The blocks behind, up to the next
        # split, take their leaves' codes from that candidate's plane
        e = edges_of(streams[0])
        errs = oracle.rx(dd.iq_of(streams[0]), None, dd.THR, od, c.spb).err_samples
        rs = sw.restatement(oracle, sw.DEVICE)
        starts = c.meta["skip_starts"]
        assert len(starts) == len(seams) + (name != "pick_wave_seam")
        for s0 in starts:
            kk = sw.dropped_through(errs, e, c.spb, s0)
            image = rs.leaf_info(int(a.level[s0]), int(a.length[s0]), 10 ** 6)[0]
            r = by[sw.block_lane(s0)[0]]
            assert kk is not None and ("skip", kk) not in image and a.nc[s0] == 3 and r.first == s0 + 1, (name, s0)
        for S, s0 in zip(seams, starts):
            r = by[sw.block_lane(s0)[0]]
            assert r.block < S < r.block + r.dist, (name, S, r)     # it starts in front of block S and ends behind it
        if name != "pick_wave_seam":
            assert by[sw.block_lane(starts[-1])[0]].dist is None and a.regions[-1].tail >= 1       # the last region
    elif name == "batch_small":
        assert [x.ne for x in an[:7]] == [0, 1, 2, 3, 65, 66, 129] and [x.nblk for x in an[:7]] == [0, 0, 1, 1, 1, 2, 2]
        assert by[1].dist == 8
    elif name == "batch_mixed":
        assert [x.holds for x in an] == [True, False, True]
    else:
        pytest.fail("no check for case %s" % name)


@pytest.mark.parametrize("name", sw.CHUNK_NAMES)
def test_chunks_case(oracle, depth, name):
    """the pipelined cases, chunk by chunk: chunk 1 starts high, its x is lane 56 of block 0 -- `depth` leaves in front of
    block 1 --, its only sync-shaped leaf lies d leaves behind x, and it has ten blocks"""
    c = sw.case(name)
    stream, = sw.streams(c)
    bounds = sw.chunk_bounds(stream.size, c.spb)
    an = sw.analysed(oracle, c, depth)
    m = c.meta
    assert len(bounds) == len(an) == 3 and all((b - a) == sw.CHUNK_BUFFERS * c.spb for a, b in bounds)
    lo, hi = bounds[1]
    assert stream[lo - 1] == 1 and stream[lo] == 1                  # has_prev, lvl0 = 1, and no edge on its first sample
    a = an[1]
    assert a.nblk == sw.SYNC_MAX_RUN + 2 and a.level[1] == 0 and a.level[2] == 1
    assert np.nonzero(a.stuckable)[0].tolist() == [m["x"] - 2, m["x"]] and sw.block_lane(m["x"]) == (0, sw.LB - depth)
    assert m["s"] - m["x"] == m["d"] and a.shaped[m["s"]]
    # (the stretch's one-sample pulses have the shape too; like s at d <= depth they lie too close behind a stuck leaf)
    assert np.nonzero(a.sync)[0].tolist() == ([m["s"]] if m["d"] > depth else [])
    if m["d"] <= depth:
        assert sw.block_lane(m["s"]) == (1, 0) and not a.sync[m["s"]] and not a.holds
        assert [(r.block, r.tail) for r in a.regions] == [(0, sw.SYNC_MAX_RUN + 1)]
    else:
        assert sw.block_lane(m["s"]) == (1, 1) and a.sync[m["s"]] and a.holds
        assert [(r.block, r.tail) for r in a.regions] == [(0, sw.SYNC_MAX_RUN + 1), (1, sw.SYNC_MAX_RUN)]
    assert an[0].holds and an[2].holds and len(an[0].regions) >= 3 and len(an[2].regions) >= 3
    assert sw.expected_form(oracle, c, depth) == c.form == (2 if m["d"] <= depth else 1)
    want = oracle.rx(dd.iq_of(stream), None, dd.THR, dd.fsm_desc(oracle, sw.DEVICE), c.spb)
    assert len(want.err_samples) == 0
    ms = np.asarray(want.msg_samples)
    assert all(((ms >= a0) & (ms < b0)).sum() >= 5 for a0, b0 in bounds)
    assert len({bytes(p) for p in want.payloads}) >= 0.6 * len(ms)
