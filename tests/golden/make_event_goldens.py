#!/usr/bin/env python3
"""Generate tests/golden/events.npz by IMPORTING THE REFERENCE where a checkout of it exists (never on the GPU box, never from tests):

    python tests/golden/make_event_goldens.py

The reference is put on sys.path together with throw-away stub modules for the packages it imports but that are absent here
(theano -> only `config.floatX`, h5py, Bio, fast5_research, and its own compiled viterbi_helpers); none of the stubbed functionality
is exercised.  Its features.from_events, maths.studentise and batch.chunkify are called on the seeded event tables of event_cases.py
and their outputs stored.  Only arrays the reference produced (and digests of the inputs) are written; none of its text.

What is stored, per case <c> of event_cases.CASES:
    <c>_digest                     sha256 of the generated input columns (the tests regenerate them and compare)
    <c>_fe_n<N>_k<K>               from_events(ev, tag='', normalise=N, nanonet=K)        (the biggest case: N=1, K=0 only)
    <c>_fe_scaled                  from_events(ev) with its defaults (tag='scaled_')      (small cases)
    <c>_chunks_<chunk_len>         chunkify(..., use_scaled=False, 'per-chunk')[0]        (the biggest case: chunk_len 500 only)
    <c>_labels_<chunk_len>, <c>_bad_<chunk_len>
'none' and 'per-read' chunks are the first ml * chunk_len rows of fe_n0_k0 / fe_n1_k0 reshaped -- asserted here, not stored twice.
    studentise_axis0 / _axis1 / _all   maths.studentise of event_cases.studentise_input()
    e_ref, max_abs                 the reference's largest absolute difference from the float64 evaluation of the same formulas
                                   (event_cases.features64 / studentise64) over everything studentised above, and the largest magnitude
                                   among those values
"""
import hashlib
import os
import sys
import tempfile

import numpy as np

REF = os.environ.get("SLOIKA_REFERENCE", "/root/reference")
OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, OUT)
import event_cases as ec  # noqa: E402


def _setup_reference():
    tmp = tempfile.mkdtemp(prefix="sloika_ref_stub_")
    for name, body in {
        "theano/__init__.py": "class _C:\n    floatX = 'float32'\nconfig = _C()\n",
        "h5py/__init__.py": "",
        "Bio/__init__.py": "from . import SeqIO\n",
        "Bio/SeqIO.py": "",
        "fast5_research/__init__.py": "class Fast5:\n    pass\ndef iterate_fast5(*a, **k):\n    return []\n",
        "vh/viterbi_helpers.py": "",
    }.items():
        path = os.path.join(tmp, name)
        os.makedirs(os.path.dirname(path), exist_ok=True)
        with open(path, "w") as fh:
            fh.write(body)
    sys.path.insert(0, REF)
    sys.path.insert(0, tmp)
    import sloika
    sloika.__path__.append(os.path.join(tmp, "vh"))


def digest(cols):
    h = hashlib.sha256()
    for k in sorted(cols):
        h.update(np.ascontiguousarray(cols[k]).tobytes())
    return np.frombuffer(h.digest(), dtype=np.uint8)


def main():
    _setup_reference()
    import sloika.features
    from sloika import batch, features, maths
    batch.init_chunk_identity_worker(5, b"ACGT")
    out, e_ref, max_abs = {}, 0.0, 0.0

    def measure(ref32, f64):
        nonlocal e_ref, max_abs
        if os.environ.get("EVENT_GOLDENS_VERBOSE"):
            with np.errstate(invalid="ignore"):
                print("  %-8s %-16s err %.3e  max %.4f" % (name, ref32.shape, np.nanmax(np.abs(ref32 - f64)), np.nanmax(np.abs(f64))))
        ok = np.isfinite(f64) & np.isfinite(ref32)
        if ok.any():
            e_ref = max(e_ref, float(np.abs(ref32.astype(np.float64) - f64)[ok].max()))
            max_abs = max(max_abs, float(np.abs(f64[ok]).max()))

    biggest = max(ec.CASES, key=lambda c: ec.CASES[c][0])
    for name in ec.CASES:
        cols = ec.columns(name)
        ev = ec.table(cols)
        out[name + "_digest"] = digest(cols)
        fe = {}
        with np.errstate(divide="ignore", invalid="ignore"):
            for normalise in (0, 1):
                for nanonet in (0, 1):
                    fe[normalise, nanonet] = features.from_events(ev, tag="", normalise=bool(normalise), nanonet=bool(nanonet))
                    f64 = ec.features64(ev, "", bool(normalise), bool(nanonet))
                    if normalise:
                        measure(fe[normalise, nanonet], f64)
                    elif nanonet:                               # (the other three columns are the stored values themselves)
                        measure(fe[normalise, nanonet][:, 3], f64[:, 3])
                    if name != biggest or (normalise, nanonet) == (1, 0):
                        out["%s_fe_n%d_k%d" % (name, normalise, nanonet)] = fe[normalise, nanonet]
        if name != biggest:
            out[name + "_fe_scaled"] = features.from_events(ev)
            measure(out[name + "_fe_scaled"], ec.features64(ev, "scaled_", True, False))
        for cl in ec.CHUNK_LENS:
            if len(ev) < cl:
                continue
            ml = len(ev) // cl
            res = {norm: batch.chunkify(ev, cl, 5, False, norm) for norm in ec.NORMALISATIONS}
            assert np.array_equal(res["none"][0], fe[0, 0][:ml * cl].reshape(ml, cl, 4))
            assert np.array_equal(res["per-read"][0], fe[1, 0][:ml * cl].reshape(ml, cl, 4))
            for norm in ec.NORMALISATIONS:
                assert np.array_equal(res[norm][1], res["none"][1]) and np.array_equal(res[norm][2], res["none"][2])
            measure(res["per-chunk"][0], ec.chunk_features64(ev, "", cl))
            if name == biggest and cl != max(ec.CHUNK_LENS):
                continue
            out["%s_chunks_%d" % (name, cl)] = res["per-chunk"][0]
            out["%s_labels_%d" % (name, cl)] = res["per-chunk"][1]
            out["%s_bad_%d" % (name, cl)] = res["per-chunk"][2]
            assert res["per-chunk"][1].dtype == np.int32 and res["per-chunk"][2].dtype == np.bool_
    name = "matrix"
    x = ec.studentise_input()
    for key, axis in (("axis0", 0), ("axis1", 1), ("all", None)):
        out["studentise_" + key] = maths.studentise(x, axis=axis)
        measure(out["studentise_" + key], ec.studentise64(x, axis))
    out["e_ref"] = np.float64(e_ref)
    out["max_abs"] = np.float64(max_abs)
    path = os.path.join(OUT, "events.npz")
    np.savez_compressed(path, **out)
    print("%s: %d arrays, %d bytes; e_ref = %.3e, largest studentised magnitude %.4f (one float32 ulp of it: %.3e)"
          % (path, len(out), os.path.getsize(path), e_ref, max_abs, float(np.spacing(np.float32(max_abs)))))


if __name__ == "__main__":
    main()
