#!/usr/bin/env python3
"""tests/golden/forward.npz: what the reference's own decode.forwards (sloika/decode.py:108-139) returns for the pairs of
forward_cases.py, run HERE by importing the reference exactly as make_goldens.py does, beside an extended-precision evaluation of
the same recursion (tests/forward_ref.py: forwards_exact, np.longdouble with exact power-of-two scaling).

    python tests/golden/make_forward_goldens.py

Stored per entry (case and mode): the reference's score as a value and as a float hex string, and the extended value as a float64
pair hi + lo (so the GPU machine needs no long double).  Stored per case: the sequence, a sha256 of the input, and the posterior
itself when it is small (forward_cases.STORE_LIMIT); larger ones are rebuilt from their recipe by the tests.  `E_ref` is the largest
|reference - extended| / max(1, |extended|) over the entries: the reference's own distance from the exact value, which the GPU test
takes as its yardstick.

Refused: a long double that is no wider than a double (eps >= 1e-18), and a `full` entry whose end state holds less than e^-600 of
the mass (too near the underflow edge, where the result depends on rounding).  The archive is written with fixed
member dates: the same inputs give the same file byte for byte.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_goldens as mg                               # noqa: E402  (the reference set-up lives there)
import forward_cases as fc                              # noqa: E402
import forward_ref                                      # noqa: E402
from make_remap_slip_goldens import write_npz           # noqa: E402

OUT = os.path.join(HERE, "forward.npz")
KNOWN = {"kat/free": -4.4275354890527474, "kat/full": -5.0702616325672301}      # test/unit/test_decode.py
FULL_FLOOR = -600.0


def main():
    if not np.finfo(np.longdouble).eps < 1e-18:
        raise SystemExit("np.longdouble is no wider than float64 here: no extended-precision truth")
    mg._setup_reference()
    from sloika import decode
    kat = dict(np.load(os.path.join(HERE, "decode.npz")))
    out = {"names": np.asarray(fc.NAMES)}
    e_ref, worst = 0.0, None
    built = {}
    for name in fc.NAMES:
        post, seq = fc.build(name, kat)
        built[name] = (post, seq)
        out[name + "/seq"] = seq
        out[name + "/sha256"] = np.asarray(fc.digest(post, seq))
        if fc.stored(fc.CASES[name]):
            out[name + "/post"] = post
    for key, name, full in fc.entries():
        post, seq = built[name]
        ref = decode.forwards(post, seq, full=full)
        assert isinstance(ref, np.float64) or isinstance(ref, float), type(ref)
        if full:
            share = float(forward_ref.forwards(post, seq, full=True, parts=True)[1])
            if not share > FULL_FLOOR:
                raise SystemExit("%s: the end state holds e^%g of the mass: too near the underflow edge" % (key, share))
        if key in KNOWN and float(ref) != KNOWN[key]:
            raise SystemExit("%s: the reference gives %r, its own test says %r" % (key, float(ref), KNOWN[key]))
        hi, lo = forward_ref.forwards_exact(post, seq, full=full)
        err = abs(float((np.longdouble(ref) - np.longdouble(hi)) - np.longdouble(lo))) / max(1.0, abs(float(hi)))
        if err > e_ref:
            e_ref, worst = err, key
        out[key + "/ref"] = np.float64(ref)
        out[key + "/ref_hex"] = np.asarray(float(ref).hex())
        out[key + "/truth"] = np.asarray([hi, lo], dtype=np.float64)
        print("%-22s %5d x %4d  L %4d  ref %-24.16g |ref - truth| / max(1, |truth|) %.2e" % (
            key, post.shape[0], post.shape[1], len(seq), float(ref), err))
    out["E_ref"] = np.float64(e_ref)
    write_npz(OUT, out)
    print("E_ref %.3e (at %s); wrote %s, %d bytes" % (e_ref, worst, OUT, os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
