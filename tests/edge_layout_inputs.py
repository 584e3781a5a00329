"""Input builders for the tile-info contract between the front ends and the edge stage (test_gpu_edge_layout.py;
checked on the CPU by test_edge_layout_host.py), numpy only.  Impulse filters turn a laid sequence of levels into
output bits that are known by construction; the layouts place level changes at chosen bit positions of chosen wave
tiles and return the bits with the edge list they must give.  `classify` restates the tile info word from its
definition.  Nothing here knows what the kernels compute."""
import numpy as np

THR = 0.1                       # 204.8 LSB
ON, OFF = 1500, 20              # I of a high / low level (Q = 0): far from any guard band
ON8, OFF8 = 94, 1               # the same as CS8 samples (16 LSB each): 1504 and 16 LSB
BLOCK = 4096                    # bits per block of the edge stage
GROUP = 1024                    # blocks per first-level scan group
SEP = 2                         # constant tiles between two instances of a layout


# ------------------------------------------------------------------------------------------- impulse filters ----

def impulse(ntaps, k):
    h = np.zeros(ntaps, np.float32)
    h[k] = 1.0
    return h


# name -> (stages [(decimation, taps)] or None, total decimation, delay): output bit j = level_out(j - delay) when the
# input level is repeat(level_out, decimation); outputs in front of the capture's first level are 0.
#   one stage, decimation D, unit tap k: y[o] = x[D o + D - 1 - k]
#   two stages of decimation 2, unit taps k1, k2: y[m] = x[4 m + 3 - 2 k2 - k1]
SHAPES = {
    "none": (None, 1, 0),
    "i32k0": ([(1, impulse(32, 0))], 1, 0),
    "i32k31": ([(1, impulse(32, 31))], 1, 31),
    "i255": ([(1, impulse(255, 7))], 1, 7),
    "i16x32k0": ([(2, impulse(16, 0)), (2, impulse(32, 0))], 4, 0),
    "i16x32": ([(2, impulse(16, 3)), (2, impulse(32, 5))], 4, 3),
    "g3x40": ([(3, impulse(40, 5))], 3, 1),                 # a generic shape: y[o] = x[3 o - 3]
}


def capture(bits, shape, on=ON, off=OFF, dtype=np.int16):
    """I,Q samples (Q = 0) whose filtered, thresholded stream is `bits`.  The first `delay` bits must be 0 (they see
    the zeros in front of the capture); the last `delay` input levels repeat the last bit."""
    _, dec, delay = SHAPES[shape]
    bits = np.asarray(bits, np.uint8)
    assert not bits[:delay].any()
    level = np.concatenate([bits[delay:], np.full(delay, bits[-1], np.uint8)]) if delay else bits
    iq = np.zeros(2 * dec * level.size, dtype)
    iq[0::2] = np.repeat(np.where(level != 0, on, off).astype(dtype), dec)
    return iq


def bits_of(toggles, n):
    """the level sequence that starts at 0 and changes at every position of `toggles`"""
    t = np.zeros(n, np.uint8)
    t[np.asarray(toggles, np.int64)] = 1
    return (np.cumsum(t, dtype=np.int64) & 1).astype(np.uint8)


# ---------------------------------------------------------------------------------------------------- layout ----

class _Builder:
    """Instances are sets of level changes (positions relative to the instance's first tile); the level between two
    instances is constant for at least SEP tiles, low or high as the changes so far left it."""

    def __init__(self, tile_bits, first_tile=SEP):
        self.T = tile_bits
        self.tile = first_tile
        self.toggles = []
        self.level = 0
        self.cases = []             # (name, level in front, first tile)

    def add(self, name, rel, span=1):
        self.cases.append((name, self.level, self.tile))
        self.toggles += [self.tile * self.T + int(p) for p in rel]
        self.level ^= len(rel) & 1
        self.tile += span + SEP

    def to_block_end(self):
        """the next instance's first tile is the last tile of a block"""
        tpb = BLOCK // self.T
        while (self.tile + 1) % tpb:
            self.tile += 1

    def flip(self):
        self.add("b", [0])

    def inside_positions(self):
        T = self.T
        return [p for w in range(T // 64) for p in (64 * w, 64 * w + 1, 64 * w + 31, 64 * w + 32, 64 * w + 63) if p]

    def case_a(self, positions=None):
        # one change inside; the list is walked twice and has an odd length, so every position is laid once rising
        # behind a low tile and once falling behind a high one
        ps = self.inside_positions() if positions is None else positions
        assert len(ps) & 1
        for p in ps + ps:
            self.add("a%d" % p, [p])

    def case_f(self):
        T = self.T
        for name, rel in (("f_last", [T - 1, T]), ("f_first", [T, T + 1]), ("f_across", [T - 1, T + 1])):
            self.to_block_end()
            self.add(name, rel, span=2)

    def both_levels(self):
        """(c), (d), (e) and (f), behind a low tile and, all levels inverted, behind a high tile"""
        T = self.T
        W = T // 64
        for _ in range(2):
            # a change at the tile's first bit plus one inside, in every word (and at the tile's last bit)
            for p in [9] + [64 * w + (0, 1, 31, 32, 63)[w % 5] for w in range(1, W)] + [T - 1]:
                self.add("c%d" % p, [0, p])
            self.add("d_pulse1", [1, 2])
            self.add("d_pulse_end", [T - 2, T - 1])
            self.add("d_same_word", [64 + 10, 64 + 40])
            self.add("d_first_last", [20, T - 20])
            self.add("d_last_next", [T - 1, T], span=2)
            self.add("e", [0, 3 * T], span=4)
            self.case_f()
            self.flip()

    def result(self, n_tiles=None):
        need = self.tile                # (the last instance's SEP tiles are in it)
        n_tiles = need if n_tiles is None else n_tiles
        assert n_tiles >= need, "the layout needs %d tiles" % need
        assert self.level == 0
        toggles = np.array(sorted(self.toggles), np.uint64)
        assert np.unique(toggles).size == toggles.size
        return bits_of(toggles, n_tiles * self.T), toggles


def layout(tile_bits, n_tiles=None):
    """-> bits [n_tiles * tile_bits] (uint8), expected edge list (uint64), cases [(name, level in front, tile)].
    n_tiles None: as many tiles as the cases take.  Starts and ends low."""
    b = _Builder(tile_bits)
    b.case_a()
    b.flip()                    # (b) rising: the tile stays high ...
    b.flip()                    # ... and falling
    b.both_levels()
    bits, edges = b.result(n_tiles)
    return bits, edges, b.cases


def tiles_high(bits, tile_bits):
    """per tile: does it hold a high sample (a loud tile; the others are quiet)"""
    n = bits.size
    pad = (-n) % tile_bits
    return np.concatenate([bits, np.zeros(pad, np.uint8)]).reshape(-1, tile_bits).any(axis=1)


def complement(bits, tile_bits):
    """levels inverted inside the loud tiles (those that hold a high sample), the quiet tiles unchanged: what was
    all high is quiet now, over whatever the run before left there"""
    loud = np.repeat(tiles_high(bits, tile_bits), tile_bits)[:bits.size]
    return np.where(loud, 1 - bits, bits).astype(np.uint8)


# ------------------------------------------------------------------------------------------------ ending high ----

ENDING_R = ("1", "31", "32", "33", "63", "64", "65", "T-1", "0")


def ending_r(name, tile_bits):
    return tile_bits - 1 if name == "T-1" else int(name)


def ending_high(tile_bits, r, two_changes):
    """A capture of three whole buffers that ends high, n_out = r (mod tile_bits): -> bits, edges, outputs per buffer
    (samples_per_buffer = that times the decimation), or None where the last tile cannot hold the variant.
    two_changes False: the on-run starts two tiles earlier and the last tile holds only the high level (a change
    counted at n_out would be its one change).  True: the last tile also holds two real changes (r >= 3: they sit
    inside the tile, not at its first bit)."""
    T = tile_bits
    per_buf = (r * pow(3, -1, T)) % T + T           # 3 per_buf = r (mod T); T < per_buf < 2 T: no multiple of the tile
    n_out = 3 * per_buf
    assert n_out % T == r and (per_buf % T or r == 0)
    last = (n_out - 1) // T                         # the tile that holds the last output
    size = n_out - last * T                         # outputs in it: r, or T
    toggles = [(last - 2) * T + 77]
    if two_changes:
        if size < 3:
            return None
        a = last * T + max(1, size // 2 - 1)
        toggles += [a, a + 1] if size < 8 else [a, last * T + size - 2]
    bits = bits_of(toggles, n_out)
    assert bits[-1] == 1
    return bits, np.array(toggles, np.uint64), per_buf


def few_a_cases(tile_bits, n_out, seed):
    """a capture of n_out outputs that ends low: one (a) case rising in its second tile, one falling in its last
    whole tile"""
    T = tile_bits
    tiles = n_out // T
    assert tiles >= 3
    ps = (1, 31, 64, 65, T - 1, T - 64)
    toggles = [T + ps[seed % 6], (tiles - 1) * T + ps[(seed + 1) % 6]]
    return bits_of(toggles, n_out), np.array(toggles, np.uint64)


# ------------------------------------------------------------------------------------- scan-group boundaries ----

F_KINDS = {"f_last": lambda T: [T - 1, T], "f_first": lambda T: [T, T + 1], "f_across": lambda T: [T - 1, T + 1]}


def _f_at(b, boundary_tile, kind):
    """an (f) case whose block boundary is the first bit of tile `boundary_tile`"""
    assert (boundary_tile * b.T) % BLOCK == 0 and b.tile <= boundary_tile - 1
    b.tile = boundary_tile - 1
    b.add(kind, F_KINDS[kind](b.T), span=2)


def _place(b, tile, name, rel):
    assert b.tile <= tile
    b.tile = tile
    b.add(name, rel)


GROUP_BLOCKS = GROUP + 26                           # 4.3 M outputs
GROUP_PER_BUF = 1001                                # outputs per buffer of the group captures: whole buffers that end
                                                    # inside a tile (7 * 11 * 13 shares no factor with a tile)


def _whole_buffers(n_out):
    return -(-n_out // GROUP_PER_BUF) * GROUP_PER_BUF


def group_layout(tile_bits, kind):
    """One capture of more than GROUP blocks that ends inside a tile.  The (f) case `kind` sits on the boundary between
    block GROUP - 1 and block GROUP -- "f_last": edges at the last bit of the one and the first bit of the other;
    "f_across": a run that is high across both -- and the two other kinds on the two block boundaries in front of it;
    (a) cases follow in blocks GROUP, GROUP + 1 and the last block.  -> bits (a multiple of GROUP_PER_BUF), edges"""
    T = tile_bits
    tpb = BLOCK // T
    kinds = [k for k in F_KINDS if k != kind] + [kind]
    b = _Builder(T, first_tile=(GROUP - 3) * tpb)
    for i, k in enumerate(kinds):
        _f_at(b, (GROUP - 2 + i) * tpb, k)
    ps = b.inside_positions()
    _place(b, max(b.tile, GROUP * tpb + SEP), "a", [ps[3]])
    assert (b.tile - SEP - 1) // tpb == GROUP
    _place(b, max(b.tile, (GROUP + 1) * tpb + 1), "a", [ps[-1]])
    assert (b.tile - SEP - 1) // tpb == GROUP + 1
    last = (GROUP_BLOCKS - 1) * tpb
    _place(b, last, "a", [ps[len(ps) // 2]])
    b.tile = last + 2                               # (one constant tile between these two)
    b.add("a", [65])
    n_out = _whole_buffers((last + 2) * T + 333)
    assert b.level == 0 and n_out % T and -(-n_out // BLOCK) == GROUP_BLOCKS
    toggles = np.array(sorted(b.toggles), np.uint64)
    return bits_of(toggles, n_out), toggles


BATCH_BLOCKS = 700


def group_layout_batch(tile_bits, delay=0):
    """Three captures of BATCH_BLOCKS blocks each, the last block ragged, so that the scan-group boundary is the first
    bit of block GROUP - BATCH_BLOCKS of capture 1: "f_last" sits exactly there and "f_across" on the block boundary
    behind.  Capture 0 ends high and capture 1 starts low; capture 1 ends high and capture 2 starts high (an edge at
    its first bit: nothing precedes a capture; behind a filter with a delay, at the first bit that can be high).  -> [bits] * 3 (equal lengths, a multiple of GROUP_PER_BUF), [edges] * 3"""
    T = tile_bits
    tpb = BLOCK // T
    n_out = _whole_buffers((BATCH_BLOCKS - 1) * BLOCK + 2 * T + 333)
    assert n_out % T and -(-n_out // BLOCK) == BATCH_BLOCKS
    end_tile = (n_out - 1) // T
    ps = [1, 31, 64, T - 1, 63]
    out_bits, out_edges = [], []
    for c in range(3):
        b = _Builder(T, first_tile=0 if c == 2 else SEP)
        if c == 2:
            b.add("starts_high", [delay])
        b.add("a", [ps[c]])
        if c == 1:
            b.add("a", [ps[c + 2]])
            _f_at(b, (GROUP - BATCH_BLOCKS) * tpb, "f_last")
            _f_at(b, (GROUP - BATCH_BLOCKS + 1) * tpb, "f_across")
        _place(b, (BATCH_BLOCKS - 2) * tpb, "a", [ps[c + 1]])
        if b.level != (0 if c == 2 else 1):
            _place(b, end_tile - 1, "last", [T - 3])
        toggles = np.array(sorted(b.toggles), np.uint64)
        bits = bits_of(toggles, n_out)
        assert bits[-1] == (0 if c == 2 else 1)
        out_bits.append(bits)
        out_edges.append(toggles)
    return out_bits, out_edges


# ------------------------------------------------------------------------------------------- chunk boundaries ----

def chunk_layout(n_out, chunk_out, tile_bits):
    """Changes around the boundaries k * chunk_out of a pipelined run (n_out = 4 chunk_out): the level high across the
    first with no edge near it, an edge exactly at the first bit of the third chunk, a one-sample pulse at the last
    bit of the third chunk.  -> bits, edges"""
    assert n_out == 4 * chunk_out and chunk_out % tile_bits == 0 and chunk_out >= 4 * tile_bits
    c = chunk_out
    toggles = [c - tile_bits - 100, c + tile_bits + 100, 2 * c, 2 * c + 200, 3 * c - 1, 3 * c]
    return bits_of(toggles, n_out), np.array(toggles, np.uint64)


# --------------------------------------------------------------------------------------------------- classify ----

def classify(bits, tile_bits, n_out=None):
    """The tile info fields of every tile that holds an output, from their definition: `count` level changes inside
    the tile (a change at position j: bit j differs from bit j - 1; the tile's first bit is not inside; positions at
    or beyond n_out do not exist), `word` = index of the 64-bit word of the tile that holds the first of them (0
    without one), `first` and `last` = the tile's first and last bit (bits beyond n_out are 0), `prev_last` = the last
    bit of the tile before (0 in front of the capture)."""
    bits = np.asarray(bits, np.uint8)
    n_out = bits.size if n_out is None else n_out
    T = tile_bits
    tiles = -(-n_out // T)
    padded = np.zeros(tiles * T, np.uint8)
    padded[:n_out] = bits[:n_out]
    change = np.zeros(tiles * T, bool)
    change[1:n_out] = padded[1:n_out] != padded[:n_out - 1]
    change = change.reshape(tiles, T)
    change[:, 0] = False
    rows = padded.reshape(tiles, T)
    count = change.sum(axis=1)
    word = np.where(count > 0, change.argmax(axis=1) // 64, 0)
    first, last = rows[:, 0], rows[:, -1]
    prev_last = np.concatenate([[0], last[:-1]]).astype(np.uint8)
    return dict(count=count, word=word, first=first, last=last, prev_last=prev_last, high=rows.all(axis=1))
