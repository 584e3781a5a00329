"""The edge cleaning rule (include/ookiedokie_amd.h, "Edge cleaning") restated in numpy and Python integers, in both
of its forms, independent of the library: the sequential recurrence, and the parity inside maximal chains of short
runs.  Shared by tests/test_clean_host.py and tests/test_gpu_clean.py."""
import numpy as np


def short_runs(edges, min_on, min_off):
    """short(i) for the closed runs 0 <= i < E - 1: run i is "on" when i is even; the comparison is strict"""
    e = [int(x) for x in edges]
    return [e[i + 1] - e[i] < (min_on if i % 2 == 0 else min_off) for i in range(len(e) - 1)]


def deleted_sequential(edges, min_on, min_off):
    """d(-1) = 0, d(i) = short(i) and not d(i - 1), in Python integers"""
    d, before = [], False
    for s in short_runs(edges, min_on, min_off):
        before = s and not before
        d.append(before)
    return d


def _deleted_parity(edges, min_on, min_off):
    e = np.asarray(edges, dtype=np.uint64)
    if e.size < 2:
        return np.zeros(0, dtype=bool)
    length = e[1:] - e[:-1]
    i = np.arange(e.size - 1)
    minimum = np.where(i % 2 == 0, np.uint64(min_on), np.uint64(min_off))
    short = length < minimum
    # a: the start of the chain run i lies in = the last index <= i whose run is short and whose predecessor is not
    starts = short & ~np.concatenate([[False], short[:-1]])
    a = np.maximum.accumulate(np.where(starts, i, -1))
    return short & ((i - a) % 2 == 0)


def deleted_parity(edges, min_on, min_off):
    """inside a maximal chain of consecutive short runs starting at run a, d(i) = ((i - a) even), in numpy"""
    return _deleted_parity(edges, min_on, min_off).tolist()


def clean_of_long(edges, min_on, min_off):
    """clean_of for lists of millions of edges: the parity form, numpy alone"""
    e = np.asarray(edges, dtype=np.uint64)
    d = _deleted_parity(e, min_on, min_off)
    if e.size < 2:
        return e, [0, 0]
    drop = np.concatenate([d, [False]]) | np.concatenate([[False], d])
    return e[~drop], [int(d[1::2].sum()), int(d[0::2].sum())]


def clean_of(edges, min_on, min_off, form="sequential"):
    """(the cleaned list as uint64, runs deleted per level [off, on]): edge i is dropped iff d(i) or d(i - 1)"""
    e = np.asarray(edges, dtype=np.uint64)
    d = (deleted_sequential if form == "sequential" else deleted_parity)(e, min_on, min_off)
    E = int(e.size)
    keep = [not ((i < E - 1 and d[i]) or (i >= 1 and d[i - 1])) for i in range(E)]
    deleted = [sum(1 for i, x in enumerate(d) if x and i % 2 == 1), sum(1 for i, x in enumerate(d) if x and i % 2 == 0)]
    return e[np.asarray(keep, dtype=bool)] if E else e, deleted


def assert_invariants(edges, cleaned, min_on, min_off):
    """the contract's consequences: an even number of edges dropped; no closed run of the cleaned list shorter than
    the minimum of its level; the cleaned list is a fixed point"""
    e, c = np.asarray(edges, dtype=np.uint64), np.asarray(cleaned, dtype=np.uint64)
    assert (e.size - c.size) % 2 == 0 and c.size <= e.size
    assert not any(short_runs(c, min_on, min_off)), (min_on, min_off)
    again, deleted = clean_of(c, min_on, min_off)
    assert again.tolist() == c.tolist() and deleted == [0, 0]
    assert np.isin(c, e).all()


def info_of(edges, min_on, min_off):
    """what Receiver.clean_edges answers for a capture with this list"""
    c, deleted = clean_of(edges, min_on, min_off)
    return dict(edges_in=len(edges), edges_out=int(c.size), deleted=deleted, min_on=int(min_on), min_off=int(min_off))
