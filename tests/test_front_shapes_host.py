"""The inputs of the shape sweeps (tests/front_shapes_inputs.py) decide something for every shape the GPU tests run:
on the oracle's result alone, the ones are between 1/16 and 15/16 of the outputs and there are at least 16 edges; the
capture's length is no multiple of a tile or a buffer, nor of a decimation beyond 3.  No GPU."""
import pytest

from tests import front_shapes_inputs as S

SHAPES = [S.fir2_shape(*s) for s in S.FIR2_SHAPES] + list(S.GENERIC_SHAPES.values()) + list(S.LARGE_SHAPES.values())


@pytest.mark.parametrize("shape", SHAPES, ids=[S.shape_id(s) for s in SHAPES])
def test_the_capture_decides_something(oracle, shape):
    st = S.stages(shape)
    dec = S.total_decimation(shape)
    n = S.sweep_len(shape)
    # (3 more than a multiple of the decimation: no multiple of it unless it divides 3)
    assert (n % dec or 3 % dec == 0) and (n // dec) % S.TILE and n % S.SPB and n <= 250000
    for d, h in st:
        assert abs(float(h.astype("float64").sum()) - 1.0) < 1e-6 and h.min() > 0
    iq = S.capture(n, seed=S.capture_seed(shape))
    want = oracle.rx(iq, oracle.make_fir(st), S.THR, None, S.SPB, want_bits=True)
    frac, edges = S.check_oracle_result(want.bits, n, dec)
    assert 0.2 < frac < 0.3, frac
    # what else the GPU tests decode with this shape: a CS8 capture (widened), the other captures of a batch
    name = {S.shape_id(v): k for k, v in dict(S.GENERIC_SHAPES, **S.LARGE_SHAPES).items()}.get(S.shape_id(shape))
    of = oracle.make_fir(st)
    if name in ("d3t40", "d5t3"):
        S.check_oracle_result(oracle.rx(S.to_cs8(iq)[1], of, S.THR, None, S.SPB, want_bits=True).bits, n, dec)
    seeds = (101, 102) if shape == S.fir2_shape(3, 5) else (201, 202) if name in ("d3t40", "d5t3") or S.TILES.get(name, 1024) < 256 else ()
    for seed in seeds:
        S.check_oracle_result(oracle.rx(S.capture(n, seed=seed), of, S.THR, None, S.SPB, want_bits=True).bits, n, dec)


def test_the_small_tile_shapes_leave_whole_tiles_behind():
    for name, shape in S.LARGE_SHAPES.items():
        n_out = S.sweep_len(shape) // S.total_decimation(shape)
        assert n_out % S.TILES[name] and n_out > 3 * S.TILES[name], name
