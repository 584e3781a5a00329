#!/usr/bin/env python3
"""Generates tests/golden/dense_ref_recorded.json: what the REFERENCE's own state machine (oracle/_ref/libookref.so,
see oracle/Makefile) decodes from short versions of the designed streams of tests/dense_devices.py, fed in buffers of
97 and of 4096 samples.  tests/test_dense_results_host.py holds the oracle to this record (and, where oracle/_ref is
built, the record to the live reference).  Run in the build container only:

    make -C oracle && python tests/golden/make_dense_ref_recorded.py

The file holds data only: message samples, payload bytes and error samples per stream and buffer size.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.join(HERE, "..", "..")
sys.path.insert(0, ROOT)
import oracle as O  # noqa: E402
from tests import dense_devices as dd  # noqa: E402
from tests.helpers import stream_from_runs  # noqa: E402

OUT = os.path.join(HERE, "dense_ref_recorded.json")
BUFFERS = (97, 4096)


def main():
    O.build()
    if not O.have_ref():
        raise SystemExit("oracle/_ref not built: needs the reference tree")
    rec = {}
    for name, dev, runs in dd.recorded_cases():
        stream = stream_from_runs(runs)
        for buf in BUFFERS:
            ms, pay, es = O.RefSm(dd.fsm_desc(O, dev)).stream(stream, buf)
            assert len(ms) <= 200, name
            rec["%s/%d" % (name, buf)] = {"samples": int(stream.size), "msg_samples": [int(x) for x in ms],
                                          "payloads": [bytes(p).hex() for p in pay],
                                          "err_samples": [int(x) for x in es]}
    with open(OUT, "w") as f:
        json.dump(rec, f, separators=(",", ":"))
        f.write("\n")
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
