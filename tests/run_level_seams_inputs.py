"""Captures laid against the seams of the pulse levels' kernel (run_levels.hip), for
test_gpu_run_level_seams.py; every property claimed here is proved on the reference alone by
test_run_level_seams_host.py.  Numpy only: what needs the reference's edges takes them through a callback.

The seams, in outputs: W = 64 lanes of the segmented wave maximum, P = 256 outputs of one pass of the workgroup over a
tile, T = 1024 outputs of a tile (without a filter; a filter's tile is a power of two below it, so a multiple of 1024 is
a tile seam of every filter), B = 4096 outputs of a block of the edge list, C = 64 T outputs of the chunk whose tiles
one ballot asks about, and the capture's last output.

Without a filter an output is its sample, so runs are laid by hand.  A peak is a maximum: a lost lane shows only if it
held the maximum, and a wrong slot only if the neighbour's value differs.  So every run has ONE largest output, at a
position the case chooses, every other output of it is one LSB smaller, and run r's largest amplitude is
lo + 2 ((step r) mod count): even, distinct over `count` runs in a row (more than the 512 a tile can hold), the
smaller value odd -- no output of one run equals the largest of another within `count` runs.

Behind a filter the edges cannot be laid by hand: `filtered_capture` shifts one pulse per target by D (target - edge)
input samples until the reference's edge sits on the target.  There a maximum cannot be placed either -- a long
window's response is flat to the last bit around its top -- so every pulse carries +-100 LSB of noise, the same for
every pulse of a capture, which makes neighbouring outputs differ and leaves the shift exact."""
from collections import namedtuple

import numpy as np

THR = 0.1
W, P, T, B = 64, 256, 1024, 4096
C = 64 * T

AMP16 = (602, 723, 5)           # (lo, count, step): 602 .. 2046, the smaller values 601 .. 2045 -- all on at THR
AMP8 = (16, 55, 7)              # CS8 / CU8 values 16 .. 124 (x 16: 256 .. 1984 LSB), the smaller ones from 15 (240 LSB)


def amplitude(r, scheme=AMP16):
    lo, count, step = scheme
    return lo + 2 * ((step * r) % count)


# name; samples (a multiple of spb, so n_out = n); samples per buffer; runs [(start, end, position of the largest)];
# claims the host test proves on the reference: ("rise", j), ("fall", j), ("open",); first_run: the index the
# amplitudes start from
Case = namedtuple("Case", "name n spb runs claims first_run")


def lay(case, scheme=AMP16, dtype=np.int16):
    """the capture: I as laid, Q = 0"""
    i = np.zeros(case.n, dtype)
    for r, (a, f, at) in enumerate(case.runs):
        assert 0 <= a <= at < f <= case.n
        top = amplitude(case.first_run + r, scheme)
        i[a:f] = top - 1
        i[at] = top
    iq = np.zeros(2 * case.n, dtype)
    iq[0::2] = i
    return iq


def edges_of_case(case):
    e = []
    for a, f, _ in case.runs:
        assert not e or a > e[-1], (case.name, a)           # runs stay apart: at least one off output between them
        e += [a] + ([f] if f < case.n else [])
    return e


def _at(a, f, variant, seam):
    """where the run's largest output goes: its first or last output, or the output on either side of the seam inside
    it (a run with no seam inside: first for "before", last for "behind")"""
    inside = seam is not None and a < seam < f
    return {"first": a, "last": f - 1, "before": seam - 1 if inside else a, "behind": seam if inside else f - 1}[variant]


def _case(name, n, spb, spans, variant, claims, first_run=0):
    """spans: [(start, end, seam or None)]"""
    spans = sorted(spans)
    return Case("%s-%s" % (name, variant), n, spb, [(a, f, _at(a, f, variant, s)) for a, f, s in spans], claims, first_run)


# ------------------------------------------------------------------------------------------------ 1. seams ----

SEAM_N, SEAM_SPB = 70000, 1000              # 68 tiles and 368 outputs: more than a chunk, a partial last tile
SEAMS = (0, W, P - W, P, 2 * P, 3 * P, T, 2 * T, B, 2 * B, C, SEAM_N)
L = 20
LAYOUTS = {"ends": ("first", "last"), "starts": ("first", "last"), "pair": ("first", "last"),
           "singles_before": ("first",), "singles_on": ("first",), "across": ("first", "last", "before", "behind")}


def seam_cases(n=SEAM_N, spb=SEAM_SPB, seams=SEAMS):
    """per layout and variant one capture that holds the layout at every seam it applies to:
    ends            a run [s - L, s): a fall at s; at s = n the open run that ends the capture (E odd)
    starts          a run [s, s + L)
    pair            a run over [s - 1, s + 1)
    singles_before  runs of one output at s - 3, s - 1, s + 1
    singles_on      runs of one output at s - 2, s, s + 2
    across          a run [s - L, s + L): its largest output first, last, and on either side of the seam"""
    out = []
    for layout, variants in LAYOUTS.items():
        spans, claims = [], []
        for s in seams:
            if layout == "ends" and s >= L:
                spans.append((s - L, s, None))
                claims.append(("fall", s) if s < n else ("open",))
            elif layout == "starts" and s + L <= n:
                spans.append((s, s + L, None))
                claims.append(("rise", s))
            elif layout == "pair" and 1 <= s < n:
                spans.append((s - 1, s + 1, s))
                claims += [("rise", s - 1), ("fall", s + 1)]
            elif layout in ("singles_before", "singles_on"):
                for j in ((s - 3, s - 1, s + 1) if layout == "singles_before" else (s - 2, s, s + 2)):
                    if 0 <= j < n:
                        spans.append((j, j + 1, None))
                        claims.append(("rise", j))
                        claims.append(("fall", j + 1) if j + 1 < n else ("open",))
            elif layout == "across" and L <= s <= n - L:
                spans.append((s - L, s + L, s))
                claims += [("rise", s - L), ("fall", s + L)]
        for v in variants:
            out.append(_case("seams-" + layout, n, spb, spans, v, claims))
    return out


# ------------------------------------------------------------------------------------------------ 2. dense ----

DENSE_N, DENSE_SPB = 8500, 500              # 8 tiles and 308 outputs


def dense_cases(n=DENSE_N, spb=DENSE_SPB):
    """on at every even output, on at every odd output: 512 runs in a tile of 1024 outputs, 32 in a wave -- the most
    an increasing list allows, half of the segment table's 1024 entries, so its cap cannot bind.  Runs of 2 with gaps of
    1 and runs of 3 with gaps of 2: 1024 is no multiple of 3 or 5, so tiles start at every phase, on ones with an odd
    and with an even number of edges inside"""
    out = [_case("dense-even", n, spb, [(j, j + 1, None) for j in range(0, n, 2)], "first", []),
           _case("dense-odd", n, spb, [(j, j + 1, None) for j in range(1, n, 2)], "first", [])]
    for on, off in ((2, 1), (3, 2)):
        spans = [(j, min(j + on, n), None) for j in range(0, n, on + off)]
        for v in ("first", "last"):
            out.append(_case("dense-%don%doff" % (on, off), n, spb, spans, v, []))
    return out


def tile_starts(edges, n_out, tile=T):
    """per tile (level at its first output, edges strictly inside it) -- tile_runs' on0 and `inside`, restated"""
    e = np.asarray(edges, np.int64)
    out = []
    for j0 in range(0, n_out, tile):
        j1 = min(j0 + tile, n_out)
        out.append((int((e <= j0).sum()) & 1, int(((e > j0) & (e < j1)).sum())))
    return out


# ------------------------------------------------------------------- 3. a tile that is on with no edge inside ----

def on_throughout_cases(n=DENSE_N, spb=DENSE_SPB):
    """tile 1 ends off, the run rises at tile 2's first output, tile 2 holds no edge, tile 3's first edge is the fall"""
    spans = [(100, 130, None), (2 * T, 3 * T + 300, 3 * T), (5 * T + 7, 5 * T + 9, None)]
    claims = [("rise", 2 * T), ("fall", 3 * T + 300)]
    return [_case("on_throughout", n, spb, spans, v, claims) for v in ("first", "last", "before", "behind")]


# ------------------------------------------------------------------------------------ 4. the ballot's ends ----

BALLOT_N, BALLOT_SPB = 133000, 1000         # 2 C + T and more: chunks 0, 1 and a third with a partial last tile


def ballot_cases(n=BALLOT_N, spb=BALLOT_SPB):
    """-> [(case, the tiles that hold an on output)]"""
    out = []
    for name, spans, tiles in (
            ("tile0_chunk0", [(10, 30, None)], [0]),
            ("tile0_chunk1", [(C + 10, C + 30, None)], [64]),
            ("tile63_chunk0", [(C - 30, C - 5, None)], [63]),
            ("tile63_chunk1", [(2 * C - 30, 2 * C - 5, None)], [127]),
            ("beside_C", [(C - 10, C - 1, None), (C + 1, C + 10, None)], [63, 64])):
        out += [(_case("ballot-" + name, n, spb, spans, v, []), tiles) for v in ("first", "last")]
    out += [(_case("ballot-across_C", n, spb, [(C - 10, C + 10, C)], v, [("rise", C - 10), ("fall", C + 10)]), [63, 64])
            for v in ("first", "last", "before", "behind")]
    return out


# --------------------------------------------------------------------------- 5. a run over more than 64 tiles ----

LONG_RUN = (10 * T + 100, 80 * T + 50)      # tiles 10 .. 80: it starts in chunk 0 and ends in chunk 1


def long_run_cases(n=BALLOT_N, spb=BALLOT_SPB):
    """the largest output a in the run's first tile, in its last, in the middle, at its first and at its last output;
    every other output of the run, in 70 other tiles, is a - 1 (one float32 step below a^2 s^2 cannot be reached from
    int16 samples)"""
    a, f = LONG_RUN
    out = []
    for name, at in (("first_tile", 10 * T + 500), ("last_tile", 80 * T + 20), ("middle", 40 * T + 1000),
                     ("first_output", a), ("last_output", f - 1), ("before_C", C - 1), ("behind_C", C)):
        out.append(Case("long_run-" + name, n, spb, [(a, f, at)], [("rise", a), ("fall", f)], 0))
    return out


# ------------------------------------------------------------------------ 6. four runs on one context ----

def sequence_cases():
    """dense, sparse, empty, dense -- all of one length"""
    d = dense_cases()
    return [d[0], on_throughout_cases()[0], Case("empty", DENSE_N, DENSE_SPB, [], [], 0), d[3]]


# --------------------------------------------------------------------------------------- 8. slot parity ----

PARITY = (1, 1, 2, 1, 0, 1, 1, 2, 1)        # E of the nine captures: odd, odd, even, odd, none, odd, odd, even, odd
PARITY_N, PARITY_SPB, PARITY_SHORT = 3000, 500, 1500


def parity_cases(n=PARITY_N, spb=PARITY_SPB):
    """a capture with an odd E ends on at its last output; the capture behind one starts on at output 0 (capture 4,
    which holds no edge, cannot).  The closed runs in between differ in number from capture to capture, so every list
    index parity meets every rounding of run_peak_base.  Amplitudes go on counting from capture to capture."""
    out, first = [], 0
    for c, par in enumerate(PARITY):
        spans = []
        if par:
            if c and PARITY[c - 1] == 1:
                spans.append((0, (1, 2, 9)[c % 3], None))
            for k in range(c % 3 + (1 if par == 2 else 0)):
                spans.append((1000 + 40 * k + c, 1000 + 40 * k + 11 + 2 * c, None))
            # the truncated captures of the shorter run keep a run across their new end
            spans.append((PARITY_SHORT - 20 - c, PARITY_SHORT + 30, PARITY_SHORT))
            if par == 1:
                spans.append((n - 5 - c, n, None))
        case = _case("parity-%d" % c, n, spb, spans, ("last", "first", "before", "behind")[c % 4], [], first)
        e = edges_of_case(case)
        assert len(e) % 2 == par % 2 and bool(e) == bool(par)
        out.append(case)
        first += len(spans) + 3
    return out


def truncated(case, m):
    """the edges of the case cut to its first m samples (its samples are lay(case)[:2 m]: a largest output at or
    behind m is gone, and `at` says nothing here)"""
    runs = [(a, min(f, m), min(at, m - 1)) for a, f, at in case.runs if a < m]
    return Case(case.name + "-cut", m, case.spb, runs, [], case.first_run)


def peak_base(lo, c):
    """run_peak_base (run_levels.hpp)"""
    return (lo + c) >> 1


def peak_slots(edges, captures):
    """run_peak_slots (run_levels.hpp)"""
    return ((edges + captures) >> 1) + 1


# ------------------------------------------------------------------------- 9, 10. tiles narrower than a wave ----

NARROW_TAPS = {32: 3000, 4: 3064}           # taps of a single stage of decimation 1 -> the tile the pass can hold


def window(ntaps):
    """a normalised Hann window, as three_stages() of test_gpu_run_levels.py makes its stages"""
    h = np.hanning(ntaps + 2)[1:-1]
    return (h / h.sum()).astype(np.float32)


def narrow_stages(tile):
    return [(1, window(NARROW_TAPS[tile]))]


NARROW_N = 6 * 8192
# one pulse of 4000 samples per target; a chunk is 64 tiles: 2048 outputs of tiles of 32, 256 of tiles of 4
NARROW_TARGETS = (("rise", 4096), ("fall", 18464), ("rise", 24608), ("fall", 36864))
NARROW_PULSE = 4000

GRID_THR = 0.01                 # a full-scale step passes it 140 outputs into the window: inside the first chunk of 256
GRID_CAPTURES = 64
GRID_CONTENTS = 3


def grid_stride_samples(cus, tile, captures=GRID_CAPTURES, spb=8192):
    """(workgroups per capture at the most, samples per capture): whole buffers with at least twice as many chunks"""
    bound = -(-cus * 8 // captures)
    n = 2 * bound * 64 * tile
    return bound, -(-n // spb) * spb


def grid_stride_capture(n, k):
    """content k: a full-scale step at sample 0, a pulse in the middle and a pulse up to the capture's end, their
    lengths depending on k"""
    i = np.zeros(n, np.int16)
    i[0:60 + 40 * k] = 32000 - 1000 * k
    i[n // 2 + 100 * k:n // 2 + 100 * k + 300 + 50 * k] = 20000 + 3000 * k
    i[n - 700 - 64 * k:] = 30000 - 2000 * k
    iq = np.zeros(2 * n, np.int16)
    iq[0::2] = i
    return iq


def grid_stride_content(c):
    """which content capture c holds: neighbours differ"""
    return c % GRID_CONTENTS


# --------------------------------------------------------------------------------- 11, 12. filtered seams ----

SHAPE_D = {"fs32_fs4": 1, "fs128_fs16_dec4": 4, "three": 30}


def three_stages():
    """decimations 3, 2, 5: three_stages() of test_gpu_run_levels.py"""
    return [(3, window(7)), (2, window(5)), (5, window(11))]



FILTERED_OUT = 4500             # outputs: 4 tiles of 1024 and a partial one; buffers of 500 D samples
FILTERED_PULSE = 300            # outputs
# two captures per shape: a rise and a fall on a tile seam, on a block seam and at the capture's end.  "At the end"
# is a rise at the last output (a run of one output, open) and a run that is on up to the last output (open: nothing
# falls at n_out).  The longest, 135 000 samples of the three-stage filter, is inside the 200 000 the design allows
# itself, so no (shape, seam) pair is dropped.
FILTERED_TARGETS = {"a": (("rise", T), ("fall", 2 * T), ("fall", B), ("rise", FILTERED_OUT - 1)),
                    "b": (("fall", T), ("rise", 2 * T), ("rise", B), ("open", FILTERED_OUT))}
DROPPED = []                    # (shape, seam, reason)


def _pulse(length, seed, amp=1500, noise=100):
    """one pulse's I samples: the same for every pulse of a capture, so a shift moves the response and nothing else"""
    return (amp + np.random.default_rng(seed).integers(-noise, noise + 1, size=length)).astype(np.int16)


def _lay_pulses(n, starts, pulse):
    i = np.zeros(n, np.int16)
    for s in starts:
        a, f = max(int(s), 0), min(int(s) + pulse.size, n)
        i[a:f] = pulse[a - int(s):f - int(s)]
    iq = np.zeros(2 * n, np.int16)
    iq[0::2] = i
    return iq


def filtered_capture(edges_fn, n, D, pulse_out, targets, seed=7, move=None):
    """One pulse of pulse_out * D samples per target, each shifted by D (target - edge) input samples until
    edges_fn(capture) -- the reference's edge list -- has the rise or fall on the target ("open": the pulse runs up to
    the capture's end).  move: what is done to the capture before it is run (a tuned context's carrier).  -> the
    capture as run"""
    move = move or (lambda iq: iq)
    pulse = _pulse(pulse_out * D, seed)
    # the response to one pulse, once: where its edges lie behind its first sample
    at = 2 * pulse_out
    e = [int(x) for x in edges_fn(move(_lay_pulses(n, [at * D], pulse)))]
    assert len(e) == 2, e
    rise, fall = e[0] - at, e[1] - at
    starts = [{"rise": (j - rise) * D, "fall": (j - fall) * D, "open": n - 60 * D}[kind] for kind, j in targets]
    for _ in range(4):
        iq = move(_lay_pulses(n, starts, pulse))
        e = [int(x) for x in edges_fn(iq)]
        # pulse i's edges are e[2 i] and e[2 i + 1]; the last pulse may run into the capture's end
        assert len(e) in (2 * len(targets), 2 * len(targets) - 1), (targets, e)
        off = [0 if kind == "open" else j - e[2 * i + (kind == "fall")] for i, (kind, j) in enumerate(targets)]
        if not any(off):
            return iq
        starts = [s + D * o for s, o in zip(starts, off)]
    raise AssertionError(("no shift puts the edges on", targets, off))


# --------------------------------------------------------------------------------------- 13. cleaned lists ----

CLEAN_N, CLEAN_STRIDE = 20001, 24000        # through fs32_fs4 (decimation 1): 24576 outputs, six blocks
CLEAN_MIN_ON = 20
CLEAN_GLITCHES = (2, 0, 5, 3)               # on-runs shorter than CLEAN_MIN_ON per capture


def clean_capture(c, n=CLEAN_N):
    """pulses of 150 .. 400 samples, and CLEAN_GLITCHES[c] pulses of 4 .. 8 samples between them, some on either side
    of a block seam of the outputs"""
    rng = np.random.default_rng(100 + c)
    i = np.zeros(n, np.int16)
    pos = 200 + 37 * c
    while pos + 500 < n:
        d = int(rng.integers(150, 400))
        i[pos:pos + d] = int(rng.integers(600, 2048))
        pos += d + int(rng.integers(300, 900))
    quiet = [j for j in (4096 - 30, 4096 + 40, 8192 - 60, 8192 + 20, 12288 - 25, 3000, 15000, 17000)
             if not i[j - 80:j + 80].any()]
    assert len(quiet) >= CLEAN_GLITCHES[c], (c, quiet)
    for k, j in enumerate(quiet[:CLEAN_GLITCHES[c]]):
        i[j:j + 4 + k] = 1800 + 20 * k
    iq = np.zeros(2 * n, np.int16)
    iq[0::2] = i
    return iq
