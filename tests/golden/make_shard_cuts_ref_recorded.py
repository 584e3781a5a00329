#!/usr/bin/env python3
"""Generates tests/golden/shard_cuts_ref_recorded.json: what the REFERENCE's own state machine (oracle/_ref/libookref.so,
see oracle/Makefile) decodes from every stream of tests/shard_cut_inputs.py, fed in buffers of the case's
samples_per_buffer.  tests/test_shard_cuts_host.py holds the oracle to this record (and, where oracle/_ref is built, the
record to the live reference): `gated`, the glitch streams and the error streams of case B are in no other record.  Run
in the build container only:

    make -C oracle && python tests/golden/make_shard_cuts_ref_recorded.py

The file holds data only: message samples, payload bytes and error samples per case.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.join(HERE, "..", "..")
sys.path.insert(0, ROOT)
import oracle as O  # noqa: E402
from tests import shard_cut_inputs as sci  # noqa: E402

OUT = os.path.join(HERE, "shard_cuts_ref_recorded.json")


def main():
    O.build()
    if not O.have_ref():
        raise SystemExit("oracle/_ref not built: needs the reference tree")
    rec = {}
    for name in sci.CASES:
        c = sci.case(name)
        ms, pay, es = O.RefSm(sci.oracle_device(O, c)).stream(c.stream, c.spb)
        rec[name] = {"samples": int(c.stream.size), "spb": int(c.spb), "msg_samples": [int(x) for x in ms],
                     "payloads": [bytes(p).hex() for p in pay], "err_samples": [int(x) for x in es]}
    with open(OUT, "w") as f:
        json.dump(rec, f, separators=(",", ":"))
        f.write("\n")
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
