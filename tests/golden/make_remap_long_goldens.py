#!/usr/bin/env python3
"""tests/golden/remap_long.npz: what the reference's own transducer.map_to_sequence (sloika/transducer.py:14-73 with the compiled
viterbi_helpers.pyx) returns for the long-reference reads of remap_long_cases.py, run HERE by importing the reference exactly as
make_remap_slip_goldens.py does.

    python tests/golden/make_remap_long_goldens.py

Stored per case: the sequence, the priors if any, the reference's path, its score as a float hex string, and a sha256 of the
input; the inputs themselves are regenerated from their seeds by the tests.  A case whose reference path does not show what the
case is there for (`needs`) is refused.  The archive is written with fixed member dates: the same inputs give the same file byte
for byte.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_goldens as mg                               # noqa: E402  (the reference set-up lives there)
import remap_long_cases as lc                           # noqa: E402
from make_remap_slip_goldens import write_npz           # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "remap_long.npz")


def main():
    mg._setup_reference()
    from sloika import transducer
    out = {"names": np.asarray(lc.NAMES)}
    for name in lc.NAMES:
        c = lc.build(name)
        score, path = transducer.map_to_sequence(c["ltrans"], c["seq"], slip=c["slip"], prior_initial=c["pi"],
                                                 prior_final=c["pf"], log=True)
        path = np.asarray(path, dtype=np.int32)
        assert np.asarray(score).dtype == np.float32
        miss = lc.unmet(c, path, np.float32(score))
        if miss:
            raise SystemExit("case %s does not test what it is there for: %s" % (name, "; ".join(miss)))
        out[name + "/seq"] = c["seq"]
        if c["pi"] is not None:
            out[name + "/pi"] = c["pi"]
        if c["pf"] is not None:
            out[name + "/pf"] = c["pf"]
        out[name + "/path"] = path
        out[name + "/score_hex"] = np.asarray(float(score).hex())
        out[name + "/sha256"] = np.asarray(lc.digest(c))
        d = lc.jumps_of(path)
        print("%-16s %5d x %5d  slip %-4g score %-16.6f longest jump %5d  %s" % (
            name, len(path), len(c["seq"]), c["slip"], float(score), d.max() if len(d) else 0,
            "= planted" if np.array_equal(path, c["planted"]) else ""))
    write_npz(OUT, out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
