#!/usr/bin/env python3
"""tests/golden/remap_slips.npz: what the reference's own transducer.map_to_sequence (sloika/transducer.py:14-73 with the compiled
viterbi_helpers.pyx) returns for the long-slip reads of remap_slip_cases.py, run HERE by importing the reference (stand-in
modules and the temporary Cython build as make_goldens.py).

    python tests/golden/make_remap_slip_goldens.py

Stored per case: the sequence, the priors if any, the reference's path, its score as a float hex string, and a sha256 of the
input; the inputs themselves are regenerated from their seeds by the tests.  A case whose reference path does not show what the
case is there for (`needs`) is refused, so the fixture cannot go vacuous.  The archive is written with fixed member dates: the
same inputs give the same file byte for byte.
"""
import io
import os
import sys
import zipfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_goldens as mg          # noqa: E402  (the reference set-up lives there)
import remap_slip_cases as rc      # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "remap_slips.npz")


def write_npz(path, arrays):
    """np.savez_compressed with every member dated 1980-01-01 and in the order given."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as zf:
        for name, a in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(a), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            zf.writestr(info, buf.getvalue(), compresslevel=9)


def main():
    mg._setup_reference()
    from sloika import transducer
    out = {"names": np.asarray(rc.NAMES)}
    for name in rc.NAMES:
        c = rc.build(name)
        score, path = transducer.map_to_sequence(c["ltrans"], c["seq"], slip=c["slip"], prior_initial=c["pi"],
                                                 prior_final=c["pf"], log=True)
        path = np.asarray(path, dtype=np.int32)
        assert np.asarray(score).dtype == np.float32
        miss = rc.unmet(c, path, np.float32(score))
        if miss:
            raise SystemExit("case %s does not test what it is there for: %s" % (name, "; ".join(miss)))
        out[name + "/seq"] = c["seq"]
        if c["pi"] is not None:
            out[name + "/pi"] = c["pi"]
        if c["pf"] is not None:
            out[name + "/pf"] = c["pf"]
        out[name + "/path"] = path
        out[name + "/score_hex"] = np.asarray(float(score).hex())
        out[name + "/sha256"] = np.asarray(rc.digest(c))
        d = rc.jumps_of(path)
        print("%-20s %5d x %5d  slip %-6g score %-14.6f longest jump %4d  %s" % (
            name, len(path), len(c["seq"]), c["slip"], float(score), d.max() if len(d) else 0,
            "= planted" if np.array_equal(path, c["planted"]) else ""))
    write_npz(OUT, out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
