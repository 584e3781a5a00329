#!/usr/bin/env python3
"""Generates tests/golden/ref_recorded.json: what the REFERENCE's own code
(oracle/_ref/libookref.so, see oracle/Makefile) returns for exactly the
inputs of the three differential tests that call it live:

  * tests/test_formatter.py::test_live_reference_differential  -- formatter.c
  * tests/test_host.py::test_synth_tx_walk_matches_reference_sm_generate
                                                    -- sm_generate + complexf_to_sc16q11
  * tests/test_oracle.py::test_random_devices_differential_vs_reference_fsm
                                                    -- state_machine.c

With the record those tests run where oracle/_ref cannot be built; where it
can, they also check the record against the live reference.  Run in the
build container only:

    make -C oracle && python tests/golden/make_ref_recorded.py

The file holds data only: the reference's outputs (key / value strings,
run-length coded I rails, message samples, payload bytes, error samples).
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.join(HERE, "..", "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
import oracle as O  # noqa: E402
import ookiedokie_amd as ok  # noqa: E402
import make_formatter_golden as G  # noqa: E402
from tests.helpers import golden_path, stream_from_runs  # noqa: E402
from tests.test_oracle import _random_fsm  # noqa: E402

OUT = os.path.join(HERE, "ref_recorded.json")


def rle(a):
    a = np.asarray(a)
    cut = np.flatnonzero(np.diff(a)) + 1
    starts = np.concatenate([[0], cut])
    ends = np.concatenate([cut, [a.size]])
    return [[int(a[s]), int(e - s)] for s, e in zip(starts, ends)]


def formatter_live():
    """test_live_reference_differential: per layout None (refused) or the key / value lists of its 10 payloads."""
    rng = np.random.default_rng(7)
    out = []
    for _ in range(120):
        nb = int(rng.integers(1, 257))
        fields = G.random_fields(rng, (nb + 7) // 8)
        try:
            rf = O.RefFormatter(fields, nb)
        except ValueError:
            out.append(None)
            continue
        kvs = []
        for _ in range(10):
            pay = rng.integers(0, 256, size=(nb + 7) // 8, dtype=np.uint8)
            kvs.append([list(kv) for kv in rf.data_to_keyval(pay.tobytes())])
        out.append(kvs)
    return out


SYNTH_CASES = (("p3l-nexa2012", 3000000), ("unknown-remote1", 3000000), ("p3l-nexa2012", 1000000))


def synth_tx():
    """test_synth_tx_walk_matches_reference_sm_generate: the I rail of sm_generate's waveform per message."""
    out = []
    for name, rate in SYNTH_CASES:
        dev = ok.Device.load(golden_path("devices", name), rate)
        odev, _ = O.load_device_json(golden_path("devices", name), rate)
        syn = ok.Synth(dev, 3_000_000, seed=7, sample_rate=rate, noise=0, glitch_every=0,
                       random_phase=False, gap_us=(4000, 4000))
        for i in range(min(syn.num_messages, 3)):
            _, payload = syn.message(i)
            ref_i = O.ref_pack(O.RefSm(odev).generate(payload, 0.95))[0::2]
            out.append({"device": name, "rate": rate, "message": i, "payload": payload.hex(), "i_rle": rle(ref_i)})
    return out


def random_fsm():
    """test_random_devices_differential_vs_reference_fsm: what the reference state machine decodes."""
    rng = np.random.default_rng(77)
    out = []
    for it in range(60):
        rate = int(rng.choice([3000000, 1000000, 750000, 48000]))
        dev = _random_fsm(O, rng, rate)
        scale = rate / 1e6
        runs = [max(1, int(rng.choice([30, 60, 100, 200, 250, 400, 1000])
                           * scale * rng.uniform(0.8, 1.2)))
                for _ in range(int(rng.integers(20, 200)))]
        stream = stream_from_runs(runs)
        for buf in (97, 4096):
            ms, pay, es = O.RefSm(dev).stream(stream, buf)
            out.append({"it": it, "buf": buf, "msg_samples": [int(x) for x in ms],
                        "payloads": [bytes(p).hex() for p in pay], "err_samples": [int(x) for x in es]})
    return out


def main():
    O.build()
    if not O.have_ref():
        raise SystemExit("oracle/_ref not built: needs the reference tree")
    rec = {"formatter_live": formatter_live(), "synth_tx": synth_tx(), "random_fsm": random_fsm()}
    with open(OUT, "w") as f:
        json.dump(rec, f, separators=(",", ":"))
        f.write("\n")
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
