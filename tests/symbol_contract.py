"""The symbol survey's contract (include/ookiedokie_amd.h, "Symbol survey") restated in numpy and Python integers,
independent of the library: class table, edges -> kinds and frames, the coding rule and the device rule.  Shared by
tests/test_symbols_host.py and tests/test_gpu_symbols.py."""
import numpy as np

from tests.pulse_contract import py_bin_lower

NONE = 16
SIDE = 17
FRAME_BINS = 512
OTHER, SYNC, ZERO, ONE = 0, 1, 2, 3
OK, KINDS, NOT_DISTANCE, AMBIGUOUS, NO_SYNC, NO_FRAMES, TOO_LONG = range(7)
MAX_BITS = 256


def table_from_pulses(sug):
    """the classes' lower / upper per level (0 = off, 1 = on), from pulse_contract.py_suggest's dict or the library's"""
    return dict(lower=[[int(k["lower"]) for k in sug["classes"][lv]] for lv in (0, 1)],
                upper=[[int(k["upper"]) for k in sug["classes"][lv]] for lv in (0, 1)])


def table_ok(table):
    for lv in (0, 1):
        lo, up = table["lower"][lv], table["upper"][lv]
        if len(lo) != len(up) or len(lo) > NONE:
            return False
        if any(a > b for a, b in zip(lo, up)) or any(lo[k] <= up[k - 1] for k in range(1, len(lo))):
            return False
    return True


def classes_of(d, lower, upper):
    """class of every length: the range that holds it, 16 for none"""
    d = np.asarray(d, dtype=np.uint64)
    out = np.full(d.size, NONE, dtype=np.int64)
    for k, (lo, up) in enumerate(zip(lower, upper)):
        out[(d >= np.uint64(lo)) & (d <= np.uint64(up))] = k
    return out


def survey_of(edges, table, roles=None):
    """the contract, symbol by symbol"""
    assert table_ok(table)
    e = np.asarray(edges, dtype=np.uint64)
    E = int(e.size)
    S = (E - 1) // 2 if E >= 3 else 0
    kinds = np.zeros((SIDE, SIDE), dtype=np.uint64)
    frames = np.zeros((2, FRAME_BINS), dtype=np.uint64)
    out = dict(num_symbols=S, kinds=kinds, num_syncs=0, head_symbols=0, tail_symbols=0, frames=frames)
    if S == 0:
        return out
    assert (e[1:] > e[:-1]).all(), "an edge list is strictly increasing"
    on = classes_of(e[1:2 * S:2] - e[0:2 * S:2], table["lower"][1], table["upper"][1])
    off = classes_of(e[2:2 * S + 1:2] - e[1:2 * S:2], table["lower"][0], table["upper"][0])
    assert on.size == S and off.size == S
    np.add.at(kinds, (on, off), np.uint64(1))
    if roles is None:
        return out
    role = np.asarray(roles, dtype=np.uint8)[on, off]
    p = np.nonzero(role == SYNC)[0]
    out["num_syncs"] = int(p.size)
    out["head_symbols"] = int(p[0]) if p.size else S
    out["tail_symbols"] = S - int(p[-1]) if p.size else 0
    data = (role == ZERO) | (role == ONE)
    for a, b in zip(p[:-1].tolist(), p[1:].tolist()):
        clean = bool(data[a + 1:max(b - 1, a + 1)].all())        # symbols a + 1 .. b - 2; none when b - a <= 2
        frames[int(clean), min(b - a, FRAME_BINS - 1)] += np.uint64(1)
    return out


def assert_same_survey(got, want, what=""):
    for key in ("num_symbols", "num_syncs", "head_symbols", "tail_symbols"):
        assert got[key] == want[key], (what, key, got[key], want[key])
    for key in ("kinds", "frames"):
        g, w = np.asarray(got[key]), np.asarray(want[key])
        assert g.shape == w.shape and g.dtype == np.uint64, (what, key)
        diff = np.argwhere(g != w)
        assert diff.size == 0, (what, key, diff[:6].tolist(), g[g != w][:6], w[g != w][:6])


def py_coding(sug, kinds):
    """rules 1 to 4: (coding dict, roles [17, 17])"""
    roles = np.zeros((SIDE, SIDE), dtype=np.uint8)
    out = dict(found=0, reason=OK)
    order = sorted(((int(kinds[a][b]), a, b) for a in range(NONE) for b in range(NONE) if int(kinds[a][b])),
                   key=lambda k: (-k[0], k[1], k[2]))
    if len(order) < 3:
        out["reason"] = KINDS
        return out, roles
    zero, one = order[0], order[1]
    if zero[1] != one[1]:
        out["reason"] = NOT_DISTANCE
        return out, roles
    if zero[2] > one[2]:
        zero, one = one, zero
    t0, t1 = sug["classes"][0][zero[2]]["mean_us"], sug["classes"][0][one[2]]["mean_us"]
    out.update(data_on_class=zero[1], zero_off_class=zero[2], one_off_class=one[2], zero_count=zero[0], one_count=one[0],
               t0_us=t0, t1_us=t1)
    if not 1.15 * t0 < 0.85 * t1:
        out["reason"] = AMBIGUOUS
        return out, roles
    sync = next((k for k in order[2:] if k[0] >= 2), None)
    if sync is None:
        out["reason"] = NO_SYNC
        return out, roles
    out.update(sync_on_class=sync[1], sync_off_class=sync[2], sync_count=sync[0], found=1)
    roles[zero[1], zero[2]], roles[one[1], one[2]], roles[sync[1], sync[2]] = ZERO, ONE, SYNC
    return out, roles


def _us(mean, rate):
    x = mean / rate * 1e6
    return int(np.floor(x + 0.5))               # llround of a positive number


def py_device(sug, survey, coding, rate):
    """rules 5 and 6"""
    out = dict(found=0, reason=coding["reason"], num_bits=0, frame_symbols=0, num_syncs=int(survey["num_syncs"]),
               frames_seen=0, frames_counted=0, frames_clean=0, sync_on_us=0, sync_off_us=0, bit_on_us=0, zero_off_us=0, one_off_us=0)
    if not coding["found"]:
        return out
    fr = survey["frames"]
    counted = int(fr[:, 3:FRAME_BINS - 1].sum())            # a frame of 1 or 2 symbols, or a clamped one, is no message
    L = max(range(3, FRAME_BINS - 1), key=lambda d: (int(fr[1][d]), -d))
    out.update(frames_seen=int(fr.sum()), frames_counted=counted, frames_clean=int(fr[1][L]))
    if int(fr[1][L]) < 1 or 2 * int(fr[1][L]) < counted:
        out["reason"] = NO_FRAMES
        return out
    on, off = sug["classes"][1], sug["classes"][0]
    out.update(frame_symbols=L, num_bits=L - 2,
               sync_on_us=_us(on[coding["sync_on_class"]]["mean"], rate), sync_off_us=_us(off[coding["sync_off_class"]]["mean"], rate),
               bit_on_us=_us(on[coding["data_on_class"]]["mean"], rate), zero_off_us=_us(off[coding["zero_off_class"]]["mean"], rate),
               one_off_us=_us(off[coding["one_off_class"]]["mean"], rate))
    if L - 2 > MAX_BITS:
        out["reason"] = TOO_LONG
        return out
    out["found"] = 1
    return out


def py_tables(s):
    """rule 7: the six states as flat tables (what ookd_device_create takes)"""
    return dict(
        max_bits=s["num_bits"],
        state_duration_us=[0, 0, s["sync_on_us"], s["sync_off_us"], s["bit_on_us"], 0],
        state_timeout_us=[0, 0, 2 * s["sync_on_us"], 2 * s["sync_off_us"], 2 * s["bit_on_us"], 2 * s["one_off_us"]],
        trig_begin=[0, 1, 2, 4, 6, 9, 12],
        #          reset idle  sync_pulse sync_gap  bit_pulse   bit_gap
        trig_cond=[1,    2,    3, 4,      2, 4,     5, 3, 4,    2, 2, 4],
        trig_action=[1,  1,    1, 1,      1, 1,     4, 1, 1,    2, 3, 1],
        trig_next=[1,    2,    3, 0,      4, 0,     0, 5, 0,    4, 4, 0],
        trig_duration_us=[0, 0, 0, 0, 0, 0, 0, 0, 0, s["zero_off_us"], s["one_off_us"], 0])


def py_chain(edges, n_out, rate):
    """pulse histogram -> classes -> kinds -> coding -> frames -> device, all by the restatements:
    (suggestion, coding, survey with roles, pulse suggestion)"""
    from tests.pulse_contract import hist_of, py_suggest
    sug = py_suggest(hist_of(edges, n_out), rate)
    table = table_from_pulses(sug)
    coding, roles = py_coding(sug, survey_of(edges, table)["kinds"])
    survey = survey_of(edges, table, roles)
    return py_device(sug, survey, coding, rate), coding, survey, sug


def frames_dict(survey, clean=None):
    """{distance: count} of the occupied frame bins (clean = 1, 0 or both)"""
    fr = survey["frames"]
    rows = fr.sum(axis=0) if clean is None else fr[clean]
    return {int(d): int(rows[d]) for d in np.nonzero(rows)[0]}


assert py_bin_lower(512) - 1 == (1 << 35) - 1          # the upper bound a class that ends in bin 511 keeps
