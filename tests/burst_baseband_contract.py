"""The burst basebands' contract (include/ookiedokie_amd.h, "Burst basebands") restated in numpy and Python integers,
independent of the library: burst table -> baseband table, and table + the filter's complex output -> the cut in
either format.  The table is taken from the output ranges [lo, hi) of tests/bursts_contract.bursts_of clipped at
m = min(n_out, ceil(n / D)) -- on purpose not the library's route, which divides the input-sample table by D.  Shared
by tests/test_burst_baseband_host.py and tests/test_gpu_burst_baseband.py."""
import numpy as np

FIELDS = ("first_output", "num_outputs", "offset")
FORMATS = ("cf32", "sc16q11")


def baseband_table_of(bursts, n_out, D, n):
    """bursts: bursts_of's dicts (with lo and hi) -> a list of dicts (first_output, num_outputs, offset), Python ints"""
    m = min(int(n_out), -(-int(n) // int(D)))
    out, offset = [], 0
    for b in bursts:
        lo, hi = min(b["lo"], m), min(b["hi"], m)
        out.append(dict(first_output=lo, num_outputs=hi - lo, offset=offset))
        offset += hi - lo
    return out


def total_of(table):
    return sum(b["num_outputs"] for b in table)


def rows_of(table):
    """the restatement's table as a uint64 array [B, 3]"""
    return np.array([[b[k] for k in FIELDS] for b in table], dtype=np.uint64).reshape(-1, 3)


def assert_table(got, table, what=""):
    """got: the library's dict (baseband_bursts or Receiver.baseband_info)"""
    assert got["num_bursts"] == len(table), (what, got["num_bursts"], len(table))
    assert got["total_outputs"] == total_of(table), (what, got["total_outputs"], total_of(table))
    for k in FIELDS:
        want = [b[k] for b in table]
        assert got[k].dtype == np.uint64 and got[k].tolist() == want, (what, k, got[k].tolist()[:8], want[:8])


def q16(v):
    """s of the contract: v * 2048 in float32, a NaN -> 0, clamped to [-32768, 32767], to nearest with ties to even"""
    v = np.asarray(v, dtype=np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        w = v * np.float32(2048.0)
    assert w.dtype == np.float32
    w = np.where(np.isnan(w), np.float32(0.0), w)
    w = np.clip(w, np.float32(-32768.0), np.float32(32767.0))
    return np.rint(w).astype(np.int16)


def baseband_cut_of(y, table, fmt):
    """y: float32 [n_out, 2] -> complex64 [total] (the bits of y) or int16 [total, 2]"""
    y = np.ascontiguousarray(y, dtype=np.float32).reshape(-1, 2)
    parts = [y[b["first_output"]:b["first_output"] + b["num_outputs"]] for b in table]
    for b, p in zip(table, parts):
        assert p.shape[0] == b["num_outputs"], "a burst beyond the filter's output"
    cut = np.concatenate(parts) if parts else y[:0]
    if fmt == "cf32":
        return np.ascontiguousarray(cut).view(np.complex64).reshape(-1)
    assert fmt == "sc16q11"
    return q16(cut)


def tiles_filtered_of(table, n_out, tile):
    """tiles [t tile, (t + 1) tile) with at least one output of a burst"""
    hit = np.zeros(-(-int(n_out) // tile) + 1, dtype=bool)
    for b in table:
        if b["num_outputs"]:
            a, f = b["first_output"], b["first_output"] + b["num_outputs"]
            hit[a // tile:(f - 1) // tile + 1] = True
    return int(hit.sum())


def turn_of(nu, D):
    x = float(nu) * D
    return x - float(np.rint(x))


def same_bits(got, want, fmt, what=""):
    """CF32 as uint32 views, SC16Q11 as int16: equality"""
    if fmt == "cf32":
        assert got.dtype == np.complex64 and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
        g = np.ascontiguousarray(got).view(np.uint32).reshape(-1, 2)
        w = np.ascontiguousarray(want).view(np.uint32).reshape(-1, 2)
    else:
        assert got.dtype == np.int16 and got.shape == want.shape and got.shape[1:] == (2,), (what, got.dtype, got.shape, want.shape)
        g, w = got, want
    bad = np.nonzero((g != w).any(axis=1))[0]
    assert bad.size == 0, (what, fmt, bad.size, bad[:6].tolist(), g[bad[:4]].tolist(), w[bad[:4]].tolist())
