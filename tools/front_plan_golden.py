"""Writes tests/golden/front_plan.json: what plan_front (csrc/front_plan.cpp) gives for the case list of
tests/front_plan_cases.py, through the library's test aid ookd_front_plan_digest.  No GPU needed.

    python tools/front_plan_golden.py [--check] [--cases-text FILE]

--check: compare with the file instead of writing it.  --cases-text: also write the cases in the line format
tools/front_plan_check.cpp reads.  Run with OOKD_FIR_VALU, OOKD_MFMA_G and OOKD_MFMA_XCD unset.
"""
import json
import os
import struct
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import front_plan_cases as P


def _hex32(x):
    return "%08x" % struct.unpack("<I", struct.pack("<f", x))[0]


def _hex64(x):
    return "%016x" % struct.unpack("<Q", struct.pack("<d", x))[0]


def cases_text(path):
    """one case per line: flags threshold nu K (nu thr)*K S (decimation ntaps tap*ntaps)*S, floats as bit patterns"""
    with open(path, "w") as f:
        for case in P.cases().values():
            filt = P.make_filter(case["filter"])
            car = case["carriers"] or []
            w = ["%u" % case["flags"], _hex32(case["threshold"]), _hex64(case["nu"] or 0.0), "%u" % len(car)]
            for nu, thr in car:
                w += [_hex64(nu), _hex32(thr)]
            w.append("%u" % (filt.num_stages if filt else 0))
            for s in range(filt.num_stages if filt else 0):
                d, taps = filt.stage(s)
                w += ["%u" % d, "%u" % len(taps)] + [_hex32(t) for t in taps]
            f.write(" ".join(w) + "\n")


def main():
    for v in ("OOKD_FIR_VALU", "OOKD_MFMA_G", "OOKD_MFMA_XCD"):
        assert v not in os.environ, v + " is set"
    got = {cid: P.digest_entry(P.plan_digest(case, P.make_filter(case["filter"]))) for cid, case in P.cases().items()}
    if "--cases-text" in sys.argv:
        cases_text(sys.argv[sys.argv.index("--cases-text") + 1])
    if "--check" in sys.argv:
        with open(P.GOLDEN_FILE) as f:
            want = json.load(f)
        bad = sorted(c for c in set(got) | set(want) if got.get(c) != want.get(c))
        print("%d cases, %d differ%s" % (len(got), len(bad), ": " + ", ".join(bad) if bad else ""))
        return 1 if bad else 0
    with open(P.GOLDEN_FILE, "w") as f:
        json.dump(got, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote %d cases to %s" % (len(got), P.GOLDEN_FILE))
    return 0


if __name__ == "__main__":
    sys.exit(main())
