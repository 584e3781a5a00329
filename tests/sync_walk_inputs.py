"""Streams laid against the constants of the scan's walk from synchronising spans (scan_sync_kernel,
scan_syncwalk_kernel, scan_syncpick_kernel), for test_gpu_sync_walk.py; checked on the CPU by test_sync_walk_host.py.
Numpy and the oracle only.

Geometry: a capture with ne edges has ne - 1 regular leaves; leaf i, 1 <= i < ne, holds the samples behind
edge i - 1 up to and including edge i, so it is run i of the run list (shifted by one sample) and high when i is odd.
Block lb holds leaves 1 + 64 lb ...; lane l of a block is leaf 1 + 64 lb + l.

What a "sync leaf" is, is restated here from its definition and from the oracle's state machine alone (`leaf_info`,
`analyse`): the machine is put (ook_sm_poke) into every (state, bit count) a leaf of that level can be entered in --
the closure of what leaves of every length leave behind, `reachable` --, fed the leaf, and looked at (ook_sm_peek).
The IMAGE is the set of ends; a leaf CAN END STUCK when one of them is an end with no trigger fired on the final edge,
in a state in which time matters; the two SKIP results are those of a machine that is dropping the rest of a buffer
when the leaf begins (it restarts from reset at the next buffer boundary, with the level of the error's sample for
its previous level).  A sync leaf has an image of 1 to 3 ends, at most 4 candidates with the skip results, and none of
the `depth` leaves before it can end stuck.  Nothing here is copied from the kernels.

The streams: burst(8) at 1 Msps.
  dense stretch   pulses of 20 us with 20 or 50 us between them, never another length: nine pulses are a message for
                  a machine in step, one out of step appends on -- every leaf's image is a state times many bit counts
  silence         a low run of 250 us (off's time-out is 200): every entry ends in `on` with no bits
  hold            a pulse of 100 us (on's time-out is 60): every entry ends in `idle`.  The silence of the other
                  parity: a silence is an even leaf, an odd lane; leaves at even lanes (split 1, 63) are pulses
  stuck stretch   g pulses of 1 us inside a 50 us bit gap, [25, 1 x (2 g - 1), 26 - 2 g]: 2 g edges on which nothing
                  fires.  Of its leaves the LOW ones can end stuck (entered in `off`, a state a leaf is entered in at
                  the low level only); x, the last of them, is the second last leaf of the stretch
  error           a pulse of 8 us: too short for `on`, the rest of its buffer is dropped"""
import ctypes as C
from collections import namedtuple

import numpy as np

from tests import dense_devices as dd
from tests import shard_cut_inputs as sci
from tests.helpers import stream_from_runs

LB = 64                     # leaves per block
SYNC_K = 4                  # kSyncK: candidates per sync leaf
SYNC_MAX_RUN = 8            # kSyncMaxRun: blocks a walk runs on beyond its own
PICK_THREADS = 1024         # threads of scan_syncpick_kernel
PICK_PER = 32               # kPickPer: blocks per thread, at most
MAX_STUCK_DEPTH = 8         # kStuckDepth: the most LTab::depth can be (the tests take depth from ookd_scan_domain_info)
REASON_SYNC = 16            # fsm_fallback_reason: the walk gave up and the scan composed

LEAD = 300
SILENCE = 250
HOLD = 100
SHORT_PULSE = 8
MSG_LEAVES = 18             # leaves of one burst(8) message and the gap behind it


def leaf_at(block, lane):
    return 1 + LB * block + lane


def block_lane(leaf):
    return (leaf - 1) // LB, (leaf - 1) % LB


# ------------------------------------------------------------------------------- the restatement: one leaf ----

class _Machine:
    def __init__(self, oracle, dev):
        self.fsm = dd.fsm_desc(oracle, dev)
        self.L = oracle.lib()
        self.cs = self.fsm.c_struct()
        self.h = self.L.ook_sm_new(C.byref(self.cs))
        self.max_bits = int(dev["max_bits"])
        self.timed = [sci.k_matters(self.fsm, s) for s in range(len(dev["state_names"]))]
        self._np, self._st, self._nb = C.c_uint(0), C.c_uint32(0), C.c_uint32(0)
        self._el, self._pb = C.c_double(0), C.c_int(0)
        self._zero = bytes(40)

    def run(self, state, nb, elapsed, prev, samples):
        """The machine poked into (state, nb, elapsed, previous level) and fed `samples`; how it ends:
        ("n", state, bits)           a trigger fired on the last sample, or time does not matter in the state
        ("stuck", state, bits, el)   nothing fired on the last sample, in a state with a duration or a time-out
        ("skip", level)              an error on the last sample: the rest of the buffer is dropped from there
        ("posdep",)                  an error before the last sample: what follows depends on the buffer boundary"""
        L = self.L
        L.ook_sm_poke(self.h, state, nb, float(elapsed), prev, self._zero, len(self._zero))
        pos, n = 0, samples.size
        base = samples.ctypes.data
        while pos < n:
            r = L.ook_sm_process(self.h, base + pos, n - pos, C.byref(self._np))
            pos += self._np.value
            if r == -1:
                return ("skip", int(samples[pos - 1])) if pos == n else ("posdep",)
        L.ook_sm_peek(self.h, C.byref(self._st), C.byref(self._nb), C.byref(self._el), C.byref(self._pb))
        st, nb, el = self._st.value, self._nb.value, self._el.value
        nb = 0 if st == 0 else min(nb, self.max_bits + 1)       # (reset zeroes the count on its next sample)
        if el > 0 and self.timed[st]:
            return ("stuck", st, nb, el)
        return ("n", st, nb)


_spans = {}


def _span(L, n):
    """n samples at level L and the edge behind them"""
    if (L, n) not in _spans:
        _spans[L, n] = np.ascontiguousarray(np.concatenate([np.full(n, L, np.uint8), [L ^ 1]]).astype(np.uint8))
    return _spans[L, n]


class Restatement:
    """Per device: the codes a leaf of either level can be entered in, and per (level, length, where the buffer boundary
    falls) what the leaf does to them.  One per device table set (`restatement`)."""

    def __init__(self, oracle, dev):
        self.m = _Machine(oracle, dev)
        self.dev = dev
        us = [int(x) for k in ("state_duration_us", "state_timeout_us", "trig_duration_us") for x in dev[k]]
        self.nmax = max(us) * dev["sample_rate"] // 1000000 * 115 // 100 + 4      # beyond: every time-out has run out
        # elapsed values around which a trigger starts or stops firing (the windows are +-15 %)
        marks = set()
        for u in us:
            if u:
                for v in (u * 0.85, u, u * 1.15):
                    marks.update(int(v) + d for d in (-1, 0, 1, 2))
        self.marks = sorted(x for x in marks if x >= 0)
        self.reach = {0: set(), 1: set()}
        self._leaf = {}
        self._closure()

    def _closure(self):
        m, todo, seen = self.m, [], set()

        def chase(end, L, hops):
            # the machine sits stuck in end[1:]; the next leaf is at level L.  (Lengths around the marks and the
            # shortest; a stretch of more than 2 * MAX_STUCK_DEPTH inert edges is not followed)
            key = (end[1], end[2], int(round(end[3])), L)
            if key in seen or hops > 2 * MAX_STUCK_DEPTH:
                return
            seen.add(key)
            for n in sorted({0} | {a - key[2] for a in self.marks if a >= key[2]}):
                add(m.run(end[1], end[2], end[3], L, _span(L, n)), L, hops + 1)

        def add(end, L, hops=0):
            # `end` is how a leaf at level L ended: the next one, at level L ^ 1, is entered in it
            if end[0] == "n":
                if end[1:] not in self.reach[L ^ 1]:
                    self.reach[L ^ 1].add(end[1:])
                    todo.append((end[1:], L ^ 1))
            elif end[0] == "stuck":
                chase(end, L ^ 1, hops)

        # a capture's first span, and a machine that starts again behind a dropped rest-of-buffer: from reset
        for prev in (0, 1):
            for L in (0, 1):
                for n in range(self.nmax):
                    add(m.run(0, 0, 0.0, prev, _span(L, n)), L)
        while todo:
            (st, nb), L = todo.pop()
            for n in range(self.nmax):
                add(m.run(st, nb, 0.0, L, _span(L, n)), L)

    def leaf_info(self, L, n, off):
        """(image, can end stuck, the two skip results) of a leaf of n samples at level L whose first sample lies `off`
        samples in front of the next buffer boundary (off > n: no boundary inside, a skip goes on through the leaf)"""
        ncl = min(int(n), self.nmax)                                # (no time-out is longer)
        rem = -1 if off > n else min(int(n) - int(off), self.nmax)  # samples between the boundary and the edge
        key = (L, ncl, rem)
        if key not in self._leaf:
            image = frozenset(self.m.run(st, nb, 0.0, L, _span(L, ncl)) for st, nb in self.reach[L])
            skips = tuple(("skip", kk) if rem < 0 else self.m.run(0, 0, 0.0, kk, _span(L, rem)) for kk in (0, 1))
            self._leaf[key] = (image, any(e[0] == "stuck" for e in image), skips)
        return self._leaf[key]


def candidates(info):
    """the candidates of a leaf that has the shape of a sync leaf (1 to 3 ends in the image, none stuck or position
    dependent; with the skip results at most SYNC_K, none of them stuck or position dependent), else None"""
    image, _, skips = info
    if not 1 <= len(image) <= 3 or any(e[0] not in ("n", "skip") for e in image):
        return None
    if any(e[0] not in ("n", "skip") for e in skips):
        return None
    cand = set(image) | set(skips)
    return cand if len(cand) <= SYNC_K else None


_restatements = {}


def restatement(oracle, dev):
    if dev["name"] not in _restatements:
        _restatements[dev["name"]] = Restatement(oracle, dev)
    return _restatements[dev["name"]]


# ---------------------------------------------------------------------------- the restatement: a capture ----

Region = namedtuple("Region", "block split first dist tail length")
# block, split: where it starts (leaves of the block from lane `split` on; block 0: split 0); first: its first leaf;
# dist: blocks to the next region start (None: there is none); tail: blocks behind `block` in the capture;
# length: leaves it walks -- through the next region's sync leaf, or to the capture's last leaf

Analysis = namedtuple("Analysis", "ne nblk level length shaped nc stuckable sync first_sync regions holds")


def analyse(oracle, dev, stream, spb, depth, lvl0=0):
    """The restatement over one capture (or one chunk of a pipelined run: lvl0 is the level in front of it)."""
    rs = restatement(oracle, dev)
    bits = np.asarray(stream, np.uint8)
    e = np.nonzero(np.diff(np.concatenate([[lvl0], bits.astype(np.int8)])))[0].astype(np.int64)
    ne = int(e.size)
    nleaf = max(ne - 1, 0)
    nblk = -(-nleaf // LB)
    level = np.zeros(ne + 1, np.int64)
    length = np.zeros(ne + 1, np.int64)
    shaped = np.zeros(ne + 1, bool)
    nc = np.zeros(ne + 1, np.int64)
    stuckable = np.zeros(ne + 1, bool)
    if nleaf:
        i = np.arange(1, ne)
        level[1:ne] = (i & 1) ^ lvl0
        length[1:ne] = e[1:] - e[:-1] - 1
        pos0 = e[:-1] + 1
        off = ((pos0 - 1) // spb + 1) * spb - pos0
        ln = length[1:ne]
        keys = np.stack([level[1:ne], np.minimum(ln, rs.nmax), np.where(off > ln, -1, np.minimum(ln - off, rs.nmax))],
                        axis=1)
        uniq, inv = np.unique(keys, axis=0, return_inverse=True)
        inv = inv.reshape(-1)
        u_shaped, u_nc, u_stuck = [], [], []
        for L, n, rem in uniq:
            info = rs.leaf_info(int(L), int(n), int(n) - int(rem) if rem >= 0 else int(n) + 1)
            c = candidates(info)
            u_shaped.append(c is not None)
            u_nc.append(len(c) if c is not None else 0)
            u_stuck.append(info[1])
        shaped[1:ne] = np.array(u_shaped)[inv]
        nc[1:ne] = np.array(u_nc)[inv]
        stuckable[1:ne] = np.array(u_stuck)[inv]
    # none of the `depth` leaves before it can end stuck (leaf 0, the capture's first span, is no regular leaf)
    dirty = np.zeros(ne + 1, bool)
    for d in range(1, depth + 1):
        dirty[1 + d:ne] |= stuckable[1:ne - d] if ne - d > 1 else False
    sync = shaped & ~dirty
    first_sync = []
    for b in range(nblk):
        lanes = np.nonzero(sync[leaf_at(b, 0):min(leaf_at(b + 1, 0), ne)])[0]
        first_sync.append(int(lanes[0]) if lanes.size else None)
    starts = [(0, 0)] + [(b, first_sync[b] + 1) for b in range(1, nblk) if first_sync[b] is not None] if nblk else []
    regions, holds = [], nblk <= PICK_PER * PICK_THREADS
    for k, (b, split) in enumerate(starts):
        f0 = b * LB + split                         # leaf f0 + 1 is the region's first
        if k + 1 < len(starts):
            b2, split2 = starts[k + 1]
            dist, fend = b2 - b, b2 * LB + split2
        else:
            dist, fend = None, ne - 1
        tail = nblk - 1 - b
        if dist is None or dist > SYNC_MAX_RUN:
            # no sync leaf in the SYNC_MAX_RUN blocks behind: to the capture's end, if that is no further
            if tail > SYNC_MAX_RUN:
                holds = False
            fend = ne - 1
        regions.append(Region(b, split, f0 + 1, dist, tail, max(fend - f0, 0)))
    return Analysis(ne, nblk, level, length, shaped, nc, stuckable, sync, first_sync, regions, holds)


# ------------------------------------------------------------------------------------------- the builder ----

def place(ne, syncs=(), stuck=(), errors=(), seed=0, spb=4096, lead=LEAD, whole=True, lengths=None):
    """Run list of a capture with `ne` edges (leaves 1 .. ne - 1 and the tail behind the last edge): dense messages with
    a silence (even leaf) or a hold (odd leaf) on every leaf of `syncs`, a stuck stretch of g pulses from the first bit
    gap at or behind leaf j for every (j, g) of `stuck`, a short pulse on the first pulse at or behind every leaf of
    `errors`.  Returns (runs, {"stuck": [(first leaf, x, last leaf)], "errors": [leaf]}).  The builder follows the
    machine in step -- leaf `ph` of MSG_LEAVES since the message began -- to know a bit gap from the gap between two
    messages; behind an error it knows nothing until the next silence."""
    rng = np.random.default_rng(seed)
    syncs, errors = set(int(s) for s in syncs), sorted(int(x) for x in errors)
    stuck = sorted((int(j), int(g)) for j, g in stuck)
    runs = [lead] + [0] * ne
    fill, placed, last = {}, {"stuck": [], "errors": []}, 0
    ph = 1                                          # leaf 1 is the first pulse of a message
    for i in range(1, ne):
        if i in syncs:
            runs[i] = (lengths or {}).get(i, SILENCE if i % 2 == 0 else HOLD)
            ph = 1 if i % 2 == 0 else MSG_LEAVES    # of the next leaf: a first pulse / the gap in front of one
            continue
        if i in fill:
            runs[i] = fill[i]
            if i < last:
                continue                            # (the stretch is one bit gap: the phase moves on behind it)
        elif stuck and i >= stuck[0][0] and i % 2 == 0 and ph is not None and 2 <= ph <= MSG_LEAVES - 2 \
                and not any(i <= s <= i + 2 * stuck[0][1] - 2 for s in syncs):
            j, g = stuck.pop(0)
            runs[i] = 25
            for q in range(1, 2 * g):
                fill[i + q] = 1
            fill[i + 2 * g] = 50 - 25 - (2 * g - 1)
            last = i + 2 * g
            placed["stuck"].append((i, i + 2 * g - 2, last))
            continue
        elif errors and i >= errors[0] and i % 2 == 1 and ph != MSG_LEAVES - 1:     # (a ninth pulse ends in reset: no error)
            errors.pop(0)
            runs[i] = SHORT_PULSE
            placed["errors"].append(i)
            ph = None
            continue
        elif i % 2 == 1:
            runs[i] = 20
        else:
            runs[i] = 50 if rng.integers(0, 2) else 20
        if ph is not None:
            ph = ph % MSG_LEAVES + 1
    assert not stuck and not errors, "not everything was placed"
    runs[ne] = 30
    if whole:
        runs[ne] += -sum(runs) % spb                # whole buffers: a run pads with low samples, here nothing is added
    return runs, placed


# ---------------------------------------------------------------------------------------------- the cases ----
# form: scan_entry_form the walk leg must report (1: the walk held; 2: it gave up, reason 16, and the scan composed).
# syncs: [(capture, leaf)] the silences and holds that are laid to be sync leaves; dirty: those that have the shape
# but lie within `depth` leaves behind a leaf that can end stuck.  kind: "single", "batch" (one call, several
# captures) or "chunks" (pipelined, 4 buffers a chunk).

Case = namedtuple("Case", "name kind spb captures syncs dirty form meta")


def _one(name, ne, syncs=(), form=1, dirty=(), spb=4096, seed=None, **kw):
    seed = sum(name.encode()) if seed is None else seed
    runs, placed = place(ne, tuple(syncs) + tuple(dirty), seed=seed, spb=spb, **kw)
    return Case(name, "single", spb, [runs], [(0, s) for s in syncs], [(0, s) for s in dirty], form, placed)


def _ne(nblk, last=30):
    """edges of a capture of nblk blocks, the last of which holds `last` leaves"""
    return LB * (nblk - 1) + last + 1


def _run(dist):
    nblk = 12 if dist >= SYNC_MAX_RUN - 1 else dist + 4     # (never more than SYNC_MAX_RUN blocks behind the last start)
    return dict(ne=_ne(nblk), syncs=[leaf_at(1, 5), leaf_at(1 + dist, 7)], form=1 if dist <= SYNC_MAX_RUN else 2)


def _tail(t, last=30):
    return dict(ne=_ne(2 + t, last), syncs=[leaf_at(1, 9)], form=1 if t <= SYNC_MAX_RUN else 2)


def _len(n, lane=20):
    # a region that starts behind lane `lane` of block 1 and is n leaves long: its last leaf is the next sync leaf
    flat = LB + lane + 1 + n
    return dict(ne=_ne(5), syncs=[leaf_at(1, lane), flat, leaf_at(4, 3)])


def _pick_blocks(nblk, seams, seed):
    """blocks with a silence: every 3 to 8 blocks, and around every seam S (blocks S - 1 | S belong to two threads of
    scan_syncpick_kernel) one region from block S - 4 to block S + 3"""
    rng = np.random.default_rng(seed)
    blocks, b = [], 0
    while True:
        b += int(rng.integers(3, 9))
        if b >= nblk:
            break
        blocks.append(b)
    for S in seams:
        blocks = [b for b in blocks if not S - 4 <= b <= S + 3] + [S - 4, S + 3]
    blocks, out = sorted(set(b for b in blocks if 0 < b < nblk)), [0]
    for b in blocks + [nblk - 1]:                   # (the last block: the tail rule)
        while b - out[-1] > SYNC_MAX_RUN:           # (a seam's region moved its neighbours apart)
            out.append(out[-1] + SYNC_MAX_RUN)
        out.append(b)
    return out[1:-1]


def pick_seams(nblk):
    """(blocks per thread, seams): the first block of thread 64 and of thread 512 -- wave boundaries --, and block 1024
    where the capture goes on behind it"""
    per = -(-nblk // PICK_THREADS)
    seams = [S for S in (64 * per, 512 * per, 1024) if S + 3 + SYNC_MAX_RUN < nblk]
    return per, sorted(set(seams))


def _pick_case(name, nblk, blocks, seams, last=True):
    """Silences and holds at any lane of `blocks`.  The region across every seam S -- the one that starts in the last of
    `blocks` in front of S -- and the capture's last region start in a candidate that is NOT the first: their sync leaf
    s0 is a silence at lane 3 with a short pulse seven (or five) leaves in front of it (in the block before) and the buffer's end
    200 samples behind it, so s0 is left still dropping -- a skip result, never a code of its image.  (A silence further
    in front is stretched to move the buffer's end there.)  The pick kernel's maps, its scan over threads and waves and
    the look-back of the blocks behind s0 then carry an index other than 0, and the plane below the next split is not
    plane 0."""
    rng = np.random.default_rng(nblk)
    spb = 4096
    if last:
        blocks = [b for b in blocks if b < nblk - 1]            # (the last block stays below the last region's end)
    skip_blocks = sorted({max(b for b in blocks if b < S) for S in seams} | ({blocks[-1]} if last else set()))
    lanes = {b: 3 if b in skip_blocks else int(rng.integers(0, LB if b < nblk - 1 else 17)) for b in blocks}
    syncs = [leaf_at(b, lanes[b]) for b in blocks]
    starts = [leaf_at(b, 3) for b in skip_blocks]
    runs, placed = place(_ne(nblk, 17), syncs, errors=[s0 - 7 for s0 in starts], seed=nblk, spb=spb, whole=False)
    assert all(s0 - at in (7, 5) for s0, at in zip(starts, placed["errors"]))
    stretched = []
    for k, s0 in enumerate(starts):
        target = sum(runs[:s0 + 1]) + 200           # where the buffer is to end: behind s0's edge
        # (a silence behind the start before this one, or that start's buffer end would move too)
        stretch = max(q for q in syncs if q % 2 == 0 and q < s0 - 64 and (k == 0 or q > starts[k - 1] + 64))
        runs[stretch] += -target % spb
        stretched.append(stretch)
    runs[-1] += -sum(runs) % spb
    return Case(name, "single", spb, [runs], [(0, q) for q in syncs], [], 1, dict(placed, skip_starts=starts, stretched=stretched))


def dropped_through(err_samples, e, spb, leaf):
    """the level of the error's sample if leaf `leaf` (edges e) lies wholly in the dropped rest of an error's buffer --
    the machine enters and leaves it in that skip code --, else None"""
    for p in err_samples:
        if p <= e[leaf - 1] and (int(p) // spb + 1) * spb > e[leaf] + 1:
            return int(np.searchsorted(e, p, side="right")) & 1       # (edges before or at p: odd = high)
    return None


STUCK_D = tuple(range(1, MAX_STUCK_DEPTH + 2))
ACROSS = ((57, MAX_STUCK_DEPTH), (57, MAX_STUCK_DEPTH + 1), (63, MAX_STUCK_DEPTH), (63, MAX_STUCK_DEPTH + 1))


def _stuck_case(name, x_want, d, nblk, others, alone_form=None):
    """A stuck stretch of two pulses whose x is the first possible leaf at or behind x_want, and a silence or hold d
    leaves behind x; `others`: further sync leaves.  The phase of the messages is chosen (by a silence in block 1) so
    that x falls on x_want exactly."""
    seed = sum(name.encode())
    for anchor in range(leaf_at(1, 0) + 1, leaf_at(1, 0) + 1 + 2 * MSG_LEAVES, 2):
        s = x_want + d
        extra = [s + 1] if d == 1 else []           # (d = 1: a hold in place of the last pulse; a silence ends the gap)
        syncs = sorted(set([anchor] + list(others)))
        runs, placed = place(_ne(nblk), syncs + [s] + extra, stuck=[(x_want - 2, 2)], seed=seed)
        if placed["stuck"] and placed["stuck"][0][1] == x_want:
            return runs, placed, syncs, [s] + extra
    raise AssertionError("no phase puts the stretch on leaf %d" % x_want)


def _build(name):
    if name.startswith("split_"):
        lane = int(name[6:]) - 1
        return _one(name, _ne(6), [leaf_at(2, lane), leaf_at(4, 10)])
    if name == "second_sync_in_block":
        return _one(name, _ne(4), [leaf_at(1, 10), leaf_at(1, 41), leaf_at(2, 21)])
    if name.startswith("run_"):
        return _one(name, **_run(int(name[4:])))
    if name.startswith("tail_"):
        p = name.split("_")
        last = int(p[2][4:]) if len(p) > 2 else 30
        return _one(name, **_tail(int(p[1]), last))
    if name.startswith("first_block_only_"):
        nblk = int(name[17:])
        return _one(name, _ne(nblk), [], form=1 if nblk <= SYNC_MAX_RUN + 1 else 2)
    if name.startswith("len_"):
        return _one(name, **_len(int(name[4:])))
    if name.startswith("stuck_") and name != "stuck_inside_region":
        # stuck_before_D, stuck_across_block_xL_dD: an anchor silence in block 1, then x -- block 2 lane 31, or lane L of
        # block 1 --, s = x + D, a silence further on in s's block (the region start when s is none) and one in block 3.
        # stuck_alone_D, stuck_across_alone_xL_dD: region starts in blocks 1 and 10 only, and s in block 5 (x in block 5
        # lane 21, or in lane L of block 4): the walk holds if and only if s is a region start
        p = name.split("_")
        alone, across = p[1] == "alone" or p[2] == "alone", p[1] == "across"
        d = int(p[-1].lstrip("d"))
        lane = int(p[-2][1:]) if across else None
        if alone:
            x, nblk, others = leaf_at(4, lane) if across else leaf_at(5, 21), 12, [leaf_at(10, 3)]
        elif across:
            x, nblk, others = leaf_at(1, lane), 4, [leaf_at(2, 41), leaf_at(3, 2)]
        else:
            x, nblk, others = leaf_at(2, 31), 4, [leaf_at(2, 55), leaf_at(3, 11)]
        runs, placed, syncs, s = _stuck_case(name, x, d, nblk, others)
        form = 2 if alone and d <= MAX_STUCK_DEPTH else 1
        clean = d > MAX_STUCK_DEPTH                 # (s + 1, the silence behind a hold at d = 1, is at d = 2)
        return Case(name, "single", 4096, [runs], [(0, q) for q in syncs + (s if clean else [])],
                    [(0, q) for q in ([] if clean else s)], form, dict(placed, d=d, s=s[0], x=x, alone=alone))
    if name == "stuck_inside_region":
        return _one(name, _ne(4), [leaf_at(1, 3), leaf_at(3, 9)],
                    stuck=[(leaf_at(1, 20), 1), (leaf_at(1, 50), 2), (leaf_at(2, 30), MAX_STUCK_DEPTH // 2)])
    if name.startswith("error_"):
        return _error_case(name)
    if name.startswith("pick_") and name != "pick_wave_seam":
        nblk = int(name[5:])
        seams = pick_seams(nblk)[1]
        return _pick_case(name, nblk, _pick_blocks(nblk, seams, nblk), seams)
    if name == "pick_wave_seam":
        # one region from block 60 through the sync leaf of block 68 (thread 68 looks back over a wave boundary to
        # thread 60), one that ends in block 127, the last thread of a wave, and one that starts there
        blocks = list(range(4, 60, 4)) + [60, 68] + list(range(73, 120, 5)) + [120, 127, 131]
        return _pick_case(name, 135, blocks, [64, 128], last=False)
    if name.startswith("nc_"):
        # the candidate counts a silence or a hold in the middle of a buffer does not reach (1 with a buffer boundary
        # inside, 3 with none).  nc_4: a low run of 201 samples -- `off` times out ON the rising edge, the machine ends
        # in reset and never sees the pulse begin: an image of two, and with no boundary inside the two skip codes.
        # nc_2: the same run with the boundary on its first sample (both skips restart in it: one end more)
        s = leaf_at(2, 13)
        c = _one(name, _ne(5), [leaf_at(1, 5), s, leaf_at(3, 30)], lengths={s: 201})
        runs = c.captures[0]
        start = sum(runs[:s])                       # the run's first sample
        shift = (-start - 1 if name == "nc_2" else 1000 - start) % c.spb
        runs[0] += shift
        runs[-1] += -shift % c.spb
        return c._replace(meta=dict(c.meta, s=s, nc=int(name[3:])))
    if name.startswith("chunks_"):
        return _chunks_case(name)
    if name == "batch_small":
        caps = [place(ne, seed=40 + ne, whole=False)[0] if ne else [200] for ne in (0, 1, 2, 3, 65, 66, 129)]
        caps.append(_build("run_8").captures[0])
        return Case(name, "batch", 4096, caps, [(7, s) for _, s in _build("run_8").syncs], [], 1, {})
    if name == "batch_mixed":
        parts = [_build(n) for n in ("run_8", "run_9", "tail_8")]
        return Case(name, "batch", 4096, [p.captures[0] for p in parts],
                    [(c, s) for c, p in enumerate(parts) for _, s in p.syncs], [], 2, {})
    raise KeyError(name)


ERROR_SPB = 1024
CHUNK_BUFFERS = 4


def chunk_bounds(n, spb):
    """[(first sample, one past the last)] of the chunks a pipelined run of n samples makes at
    pipeline_chunk_samples = CHUNK_BUFFERS * spb (spb a multiple of 4096, no filter): whole chunks while more than one
    and a half are left, the rest in one"""
    size, out, at = CHUNK_BUFFERS * spb, [], 0
    while n - at > size + size // 2:
        out.append((at, at + size))
        at += size
    return out + [(at, n)]


def _chunks_case(name):
    """Three chunks of four buffers of 4096.  Chunk 0 ends with a silence and the first ten samples of a pulse: chunk 1
    starts HIGH (has_prev, lvl0 = 1), its odd leaves are the low ones.  In chunk 1 a stuck stretch whose x is lane 56
    of block 0 -- the one leaf only the `pre` lookup `depth` leaves in front of a block sees -- and, the only sync leaf
    of the chunk, a silence at lane 0 of block 1 (d = 8: no region start; the chunk's ten blocks are one more than block
    0's region walks: the walk gives up) or a hold at lane 1 (d = 9: a region start with eight blocks behind it, which
    the chunk's end cuts: the walk holds).  Chunk 2 has a silence every 200 leaves."""
    d = int(name.rsplit("_d", 1)[1])
    spb, size = 4096, CHUNK_BUFFERS * 4096
    for seed in range(200):
        rng = np.random.default_rng(1000 * d + seed)
        gap = lambda: 50 if rng.integers(0, 2) else 20
        runs = [LEAD]
        while sum(runs) + 20 + 50 + SILENCE + 70 <= size - 10:
            runs += [20, SILENCE if len(runs) % 200 == 199 else gap()]
        runs += [20, size - 10 - sum(runs) - 20, 20]            # the silence that fills chunk 0, and the cut pulse
        assert runs[-2] >= SILENCE
        first = len(runs) - 1                       # run of chunk 1's leaf 0; its leaf i is run first + i
        x, s = leaf_at(0, 56), leaf_at(0, 56) + d
        for i in range(1, 3 * size // 20):
            if i == x - 2:
                runs += [25, 1, 1, 1, 22]           # leaves x - 2 .. x + 2: low 25, pulse, low 1 (x), pulse, low 22
            elif x - 2 < i <= x + 2:
                continue
            elif i == s:
                runs.append(SILENCE if i % 2 else HOLD)
            elif sum(runs) > 2 * size + 400 and i % 200 == 0:
                runs.append(SILENCE if i % 2 else HOLD)
            else:
                runs.append(gap() if i % 2 else 20)
            if sum(runs) >= 3 * size - 400:
                break
        if len(runs) % 2 == 0:
            runs.append(20)                         # (end low)
        runs.append(3 * size - sum(runs))
        if runs[-1] < 1:
            continue
        c = Case(name, "chunks", spb, [runs], [], [], 2 if d <= MAX_STUCK_DEPTH else 1, dict(d=d, x=x, s=s, first=first))
        stream = stream_from_runs(runs)
        lo, hi = chunk_bounds(stream.size, spb)[1]
        ne1 = int(np.count_nonzero(np.diff(stream[lo - 1:hi].astype(np.int8))))
        if -(-(ne1 - 1) // LB) == SYNC_MAX_RUN + 2:             # chunk 1 has ten blocks
            return c
    raise AssertionError("no seed gives chunk 1 ten blocks")


def _error_case(name):
    """spb 1024: a region from lane 5 of block 1 through the silence s at lane 3 of block 2, another behind.  The short
    pulse stands in block 1, behind the region's start, a few leaves in front of where the rest of its buffer ends:
      error_in_region             40 leaves in front of s, the buffer ends 300 samples on: well in front of s
      error_on_sync_leaf          6 leaves in front of s, the buffer ends inside s's silence
      error_across_regions        6 leaves in front of s, the buffer ends 200 samples behind s: s is left still
                                  dropping, and the next region starts in a skip code
      error_pulse_starts_region   s at lane 41 and the short pulse 6 leaves in front of it, in s's block: entered in
                                  `on` it ends dropping, entered in `idle` it ends there -- an image of two, and the
                                  first sync leaf of its block (the buffer ends behind s)"""
    s = leaf_at(2, 41 if name == "error_pulse_starts_region" else 3)
    syncs = [leaf_at(1, 5), s, leaf_at(4, 11)]
    at = s - 40 if name == "error_in_region" else s - 6
    at -= 1 - at % 2                                # a pulse
    seed = sum(name.encode())
    runs, placed = place(_ne(6), syncs, errors=[at], seed=seed, spb=ERROR_SPB, whole=False)
    end = np.cumsum(runs)                           # end[i]: first sample of run i + 1
    if name == "error_in_region":
        target = int(end[at]) + 300                 # where the buffer is to end
    elif name == "error_on_sync_leaf":
        target = int(end[s - 1]) + 100
    elif name in ("error_across_regions", "error_pulse_starts_region"):
        target = int(end[s]) + 200
    else:
        raise KeyError(name)
    runs[0] += -target % ERROR_SPB
    runs[-1] += -sum(runs) % ERROR_SPB
    return Case(name, "single", ERROR_SPB, [runs], [(0, q) for q in syncs], [], 1, dict(placed, s=s))


NAMES = (["split_%d" % s for s in (1, 2, 63, 64)] + ["second_sync_in_block"]
         + ["run_%d" % d for d in (1, 7, 8, 9)]
         + ["tail_%d" % t for t in (0, 1, 8, 9)] + ["tail_8_last1", "tail_8_last64", "tail_9_last1", "tail_9_last64"]
         + ["first_block_only_9", "first_block_only_10"]
         + ["len_%d" % n for n in (63, 64, 65, 128, 129)]
         + ["stuck_before_%d" % d for d in STUCK_D]
         + ["stuck_across_block_x%d_d%d" % xd for xd in ACROSS]
         + ["stuck_alone_%d" % d for d in (MAX_STUCK_DEPTH, MAX_STUCK_DEPTH + 1)]
         + ["stuck_across_alone_x%d_d%d" % xd for xd in ACROSS[:2]]
         + ["stuck_inside_region", "error_in_region", "error_on_sync_leaf", "error_across_regions",
            "error_pulse_starts_region"]
         + ["nc_2", "nc_4"]
         + ["pick_%d" % n for n in (1023, 1024, 1025, 2049)] + ["pick_wave_seam", "batch_small", "batch_mixed"])
# pipelined in chunks of CHUNK_BUFFERS buffers: one Analysis per chunk
CHUNK_NAMES = ["chunks_pre_d%d" % MAX_STUCK_DEPTH, "chunks_pre_d%d" % (MAX_STUCK_DEPTH + 1)]
GIVE_UP_THEN = {"run_9": "run_8", "tail_9": "run_8"}         # the capture run on the same context behind a give-up
_cache = {}


def case(name):
    if name not in _cache:
        _cache[name] = _build(name)
    return _cache[name]


def streams(c):
    """the captures' 0/1 streams; those of a batch at one length, whole buffers: each goes on at its last level (a
    capture with an odd number of edges ends high, and stays so)"""
    out = [stream_from_runs(r) for r in c.captures]
    if c.kind == "batch":
        n = max(x.size for x in out)
        n += -n % c.spb
        out = [np.concatenate([x, np.full(n - x.size, x[-1], np.uint8)]) for x in out]
    return out


_analysed = {}


def analysed(oracle, c, depth):
    """[Analysis] per capture -- per chunk of a pipelined case --; computed once per case"""
    if (c.name, depth) not in _analysed:
        if c.kind == "chunks":
            stream, = streams(c)
            _analysed[c.name, depth] = [analyse(oracle, DEVICE, stream[a:b], c.spb, depth, int(stream[a - 1]) if a else 0)
                                        for a, b in chunk_bounds(stream.size, c.spb)]
        else:
            _analysed[c.name, depth] = [analyse(oracle, DEVICE, s, c.spb, depth) for s in streams(c)]
    return _analysed[c.name, depth]


def expected_form(oracle, c, depth):
    """what the restatement says: 1 when every capture's walk holds"""
    return 1 if all(a.holds for a in analysed(oracle, c, depth)) else 2


DEVICE = dd.burst(8)
