"""CPU checks of tests/edge_layout_inputs.py, the inputs of tests/test_gpu_edge_layout.py: the impulse filters give the
oracle exactly the laid bits, and every layout holds the tile classes it is there for -- as conditions, counted with
`classify`, not as samples."""
import numpy as np
import pytest

from tests import edge_layout_inputs as E
from tests.helpers import edges_of

TILES = [256, 512, 1024]


def _oracle_bits(oracle, shape, iq, spb):
    stages = E.SHAPES[shape][0]
    fir = oracle.make_fir([(d, np.asarray(h, np.float32)) for d, h in stages]) if stages else None
    return oracle.rx(iq, fir, E.THR, None, spb, want_bits=True)


@pytest.mark.parametrize("shape", list(E.SHAPES))
def test_impulse_filters_give_the_laid_bits(oracle, shape):
    """output bit j = level(j - delay) for every impulse shape: the oracle's bits are the layout's, its edges the
    expected list"""
    dec = E.SHAPES[shape][1]
    bits, edges, _ = E.layout(256)
    for laid in (bits, E.complement(bits, 256)):
        want = _oracle_bits(oracle, shape, E.capture(laid, shape), 256 * dec)       # whole buffers
        assert want.decimated == laid.size
        assert (want.bits == laid).all(), np.nonzero(want.bits != laid)[0][:5]
    assert list(edges_of(bits)) == list(edges)
    assert dec * bits.size == E.capture(bits, shape).size // 2


def test_cs8_levels_give_the_laid_bits(oracle):
    bits, _, _ = E.layout(256)
    iq8 = E.capture(bits, "i32k31", E.ON8, E.OFF8, np.int8)
    want = _oracle_bits(oracle, "i32k31", iq8.astype(np.int16) * 16, 256)
    assert (want.bits == bits).all()


@pytest.mark.parametrize("shape", list(E.SHAPES))
@pytest.mark.parametrize("tile_bits", [256, 1024])
def test_captures_that_end_high(oracle, shape, tile_bits):
    """whole buffers, no multiple of the tile, the level still on at the end: the last bit is 1 and there is no edge
    at n_out"""
    dec = E.SHAPES[shape][1]
    seen = 0
    for name in E.ENDING_R:
        r = E.ending_r(name, tile_bits)
        for two in (False, True):
            case = E.ending_high(tile_bits, r, two)
            if case is None:
                assert r < 3 and two
                continue
            bits, edges, per_buf = case
            n_out = bits.size
            assert n_out == 3 * per_buf and n_out % tile_bits == r
            assert r == 0 or (per_buf * dec) % (tile_bits * dec) != 0
            iq = E.capture(bits, shape)
            assert iq.size // 2 == 3 * per_buf * dec            # whole buffers: nothing is padded
            want = _oracle_bits(oracle, shape, iq, per_buf * dec)
            assert want.decimated == n_out and (want.bits == bits).all()
            assert want.bits[-1] == 1
            assert list(edges_of(want.bits)) == list(edges) and (edges < n_out).all()
            c = E.classify(bits, tile_bits)
            assert c["count"][-1] == (2 if two else 0) and c["first"][-1] == c["prev_last"][-1] == 1
            seen += 1
    assert seen == 2 * len(E.ENDING_R) - 1


@pytest.mark.parametrize("tile_bits", TILES)
def test_layout_holds_every_tile_class(tile_bits):
    bits, edges, cases = E.layout(tile_bits)
    assert list(edges_of(bits)) == list(edges) and bits[0] == 0 and bits[-1] == 0
    c = E.classify(bits, tile_bits)
    same = c["first"] == c["prev_last"]
    words = tile_bits // 64
    for w in range(words):
        for rising in (True, False):
            # (a): one change inside, in word w, behind a low tile (rising) and behind a high one
            assert np.any((c["count"] == 1) & same & (c["word"] == w) & (c["first"] == (0 if rising else 1))), (w, rising)
            # (c): the same with a change at the tile's first bit
            assert np.any((c["count"] == 1) & ~same & (c["word"] == w) & (c["first"] == (1 if rising else 0))), (w, rising)
    for level in (0, 1):
        assert np.any((c["count"] == 0) & ~same & (c["first"] == level))            # (b)
        assert np.any((c["count"] >= 2) & (c["prev_last"] == level))                # (d)
    assert np.any((c["count"] == 0) & same & c["high"])                             # (e): all high, no change
    # every position of (a), rising and falling, in a tile that holds nothing else
    tile_of = {(int(e) // tile_bits): int(e) % tile_bits for e in edges}
    for w in range(words):
        for p in (64 * w, 64 * w + 1, 64 * w + 31, 64 * w + 32, 64 * w + 63):
            if p == 0:
                continue
            for lvl in (0, 1):
                hit = [t for name, before, t in cases if name == "a%d" % p and before == lvl]
                assert len(hit) == 1 and tile_of[hit[0]] == p and c["count"][hit[0]] == 1, (p, lvl)
    # instances are apart: a tile with a change has constant tiles on both sides, except inside a two-tile instance
    loud = (c["count"] > 0) | ~same
    names = {t: name for name, _, t in cases}
    for t in np.nonzero(loud)[0]:
        if loud[t - 1]:
            assert names.get(t - 1, "") in ("d_last_next", "f_last", "f_first", "f_across"), (t, names.get(t - 1))
    # (f): pulses on both sides of a block boundary and a run across it
    B = E.BLOCK
    e = set(int(x) for x in edges)
    last = [x for x in e if x % B == B - 1 and x + 1 in e]
    first = [x for x in e if x % B == 0 and x + 1 in e and x - 1 not in e]
    across = [x for x in e if x % B == B - 1 and x + 2 in e and x + 1 not in e]
    assert len(last) == 2 and len(first) == 2 and len(across) == 2
    assert sorted(int(bits[x]) for x in across) == [0, 1]


@pytest.mark.parametrize("tile_bits", TILES)
def test_complement_leaves_stale_tiles_under_quiet_ones(tile_bits):
    bits, _, _ = E.layout(tile_bits)
    comp = E.complement(bits, tile_bits)
    a, b = E.tiles_high(bits, tile_bits), E.tiles_high(comp, tile_bits)
    assert not (b & ~a).any()                   # the quiet tiles are unchanged
    assert (a & ~b).sum() >= 20                 # tiles the first run wrote and the second does not
    c = E.classify(comp, tile_bits)
    assert np.any(c["count"] == 1) and np.any(c["count"] >= 2)


@pytest.mark.parametrize("tile_bits", TILES)
def test_group_layout(tile_bits):
    B = E.GROUP * E.BLOCK
    for kind in E.F_KINDS:
        bits, edges = E.group_layout(tile_bits, kind)
        assert bits.size > B + 2 * E.BLOCK and bits.size % tile_bits and bits[-1] == 0
        e = set(int(x) for x in edges)
        if kind == "f_last":
            assert B - 1 in e and B in e and bits[B - 1] == 1 and bits[B] == 0
        if kind == "f_first":
            assert B - 1 not in e and B in e and B + 1 in e
        if kind == "f_across":
            assert B - 1 in e and B not in e and B + 1 in e and bits[B - 1] == 1 and bits[B] == 1
        blocks = set(x // E.BLOCK for x in e)
        assert {E.GROUP, E.GROUP + 1, (bits.size - 1) // E.BLOCK} <= blocks
        assert list(edges_of(bits)) == list(edges)
    caps, cap_edges = E.group_layout_batch(tile_bits)
    n_out = caps[0].size
    assert all(x.size == n_out for x in caps) and -(-n_out // E.BLOCK) == E.BATCH_BLOCKS and n_out % E.BLOCK
    assert 3 * E.BATCH_BLOCKS > 2 * E.GROUP > 2 * E.BATCH_BLOCKS
    g = (E.GROUP - E.BATCH_BLOCKS) * E.BLOCK        # the group boundary, in capture 1
    e1 = set(int(x) for x in cap_edges[1])
    assert g - 1 in e1 and g in e1
    assert g + E.BLOCK - 1 in e1 and g + E.BLOCK + 1 in e1 and caps[1][g + E.BLOCK] == 1
    assert [int(x[0]) for x in caps] == [0, 0, 1] and [int(x[-1]) for x in caps] == [1, 1, 0]
    assert cap_edges[2][0] == 0 and E.group_layout_batch(tile_bits, 1)[1][2][0] == 1
    for bits, edges in zip(caps, cap_edges):
        assert list(edges_of(bits)) == list(edges)


def test_chunk_layout(oracle):
    for n_out, chunk, tile_bits in ((65536, 16384, 1024), (16384, 4096, 256)):
        bits, edges = E.chunk_layout(n_out, chunk, tile_bits)
        e = set(int(x) for x in edges)
        assert bits[chunk - 1] == bits[chunk] == 1 and not any(abs(x - chunk) < tile_bits for x in e)
        assert 2 * chunk in e and 2 * chunk - 1 not in e and 2 * chunk + 1 not in e
        assert 3 * chunk - 1 in e and 3 * chunk in e
        assert list(edges_of(bits)) == list(edges)
