"""The debounced decode (include/ookiedokie_amd.h, "Debounced decode") restated: what the state machine of a debounced
context sees is the bit stream painted from the cleaned edge list, and what it answers is the CPU oracle's state machine
fed that stream buffer by buffer.  Shared by tests/test_debounce_host.py and tests/test_gpu_debounce.py."""
import numpy as np

import oracle

from tests.clean_contract import clean_of_long


def paint(edges, n_out):
    """the 0/1 stream of n_out samples with level 0 before the first edge, toggling at every edge (an edge is the
    first sample of the new level)"""
    e = np.asarray(edges, dtype=np.int64)
    assert e.size == 0 or (np.all(np.diff(e) > 0) and e[0] >= 0)
    toggles = np.zeros(int(n_out) + 1, dtype=np.int64)
    np.add.at(toggles, e[e < n_out], 1)
    return (np.cumsum(toggles[:int(n_out)]) & 1).astype(np.uint8)


def cleaned(edges, mins):
    """the cleaned list: the rule's parity form (tests/clean_contract.py; tests/test_clean_host.py holds it against the
    sequential form), which a list of any length can afford.  Minimums <= 1 give the list itself."""
    return clean_of_long(np.asarray(edges, dtype=np.uint64), int(mins[0]), int(mins[1]))[0]


def decode_cleaned(fsm, edges, n_out, mins, buf_len):
    """(message samples, payloads, error samples) of the oracle's state machine on the painted cleaned list, in buffers
    of buf_len decimated samples (samples_per_buffer / total decimation)"""
    return oracle.sm_stream(fsm, paint(cleaned(edges, mins), n_out), int(buf_len))
