#!/usr/bin/env python3
"""Generate tests/golden/olddecode.npz by IMPORTING THE REFERENCE where a checkout of it exists (never on the GPU box, never from tests):

    python tests/golden/make_olddecode_goldens.py

The reference goes on sys.path together with throw-away stub modules for the packages it imports but that are absent here (as in
make_event_goldens.py); none of the stubbed functionality is exercised.  Its basecall.decode_post(transducer=False),
decode.prepare_post, olddecode.estimate_transitions, olddecode.decode_profile and olddecode.decode_simple are called on the seeded
inputs of olddecode_cases.py and their outputs stored.  Only arrays the reference produced (and digests of the inputs) are written;
none of its text.

Per case <c> of olddecode_cases.CASES:
    <c>_digest        sha256 of the regenerated inputs (posterior, log-posteriors, log weights)
    <c>_kept          indices of the rows decode.prepare_post(drop_bad=bad) keeps (int32)
    <c>_prep_sha      sha256 of the prepared posterior's bytes;  <c>_prep_rows: its rows olddecode_cases.row_picks names, whole
    <c>_trans         olddecode.estimate_transitions(prepared, prior): float64 [kept, 3]
    <c>_post_path / _post_score     basecall.decode_post(transducer=False): states (int16) and np.float64 score
    <c>_post_score64  the same read decoded with its log-posteriors taken in float64 (the yardstick of the score allowance)
    <c>_fragile       1: the path changes when the float32 log-posteriors move by +-4 ulps (seeded): compared on score only
    <c>_prof_s<i>_path / _score, <c>_simple_s<i>_path / _score
                      decode_profile(log=True, trans=weights, slip=SLIPS[i]) and decode_simple(log=True, slip=SLIPS[i]) on
                      olddecode_cases.log_posterior(c)
(a case that loses every row -- the reference dies with IndexError there -- has digest, kept, the log=True results and no more.)
Once:
    e_ref             the reference's largest absolute difference from olddecode_cases.transitions64 (the float64 evaluation of the same
                      formulas) over all cases; rows sum to 1, so absolute is relative to 1
    score_rel_ref     the largest |post_score - post_score64| / |post_score64| over the cases
    numpy_version     of the numpy that ran the reference: its recurrence runs in float64 under numpy 2 promotion (a float32 row plus
                      an np.float64 weight) and its float32 row sum follows numpy's summation tree
"""
import os
import sys
import tempfile

import numpy as np

REF = os.environ.get("SLOIKA_REFERENCE", "/root/reference")
OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, OUT)
import olddecode_cases as oc  # noqa: E402

MAX_BYTES = 1 << 20                  # no committed file is larger than 1 MiB
MAX_FRAGILE = 0.1                    # at most one case in ten may be compared on score only


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


def main():
    _setup_reference()
    from sloika import basecall, decode, olddecode
    out, e_ref, score_rel, fragile, compared = {}, 0.0, 0.0, [], 0
    for name, (T, klen, bad, prior, seed, kind) in oc.CASES.items():
        post = oc.posterior(name)
        out[name + "_digest"] = oc.digest(name)
        prep = decode.prepare_post(post.copy(), min_prob=oc.MIN_PROB, drop_bad=bad)
        mine, rows = oc.prepare_np(post, bad)
        assert prep.dtype == np.float32 and np.array_equal(prep, mine)
        out[name + "_kept"] = rows.astype(np.int32)
        lp, w = oc.log_posterior(name)
        for i, slip in enumerate(oc.SLIPS):
            for key, (score, path) in (("prof", olddecode.decode_profile(lp, trans=w, log=True, slip=slip)),
                                       ("simple", olddecode.decode_simple(lp, log=True, slip=slip))):
                assert T == 1 or isinstance(score, np.float64), (name, type(score))   # numpy 2: the recurrence promotes to float64
                out["%s_%s_s%d_path" % (name, key, i)] = np.asarray(path, dtype=np.int16)
                out["%s_%s_s%d_score" % (name, key, i)] = np.float64(score)
        if len(rows) == 0:
            continue
        out[name + "_prep_sha"] = oc.sha256(prep)
        out[name + "_prep_rows"] = prep[oc.row_picks(len(prep))]
        trans = olddecode.estimate_transitions(prep, trans=prior)
        assert trans.dtype == np.float64
        t64 = oc.transitions64(prep, prior)
        assert np.abs(olddecode.estimate_transitions(prep.astype(np.float64), trans=prior) - t64).max() < 1e-13
        e_ref = max(e_ref, float(np.abs(trans - t64).max()))
        out[name + "_trans"] = trans
        score, path = basecall.decode_post(post.copy(), klen, False, bad, oc.MIN_PROB, trans=prior)
        s2, p2 = olddecode.decode_profile(prep, trans=np.log(oc.ETA + trans), log=False)
        assert score == s2 and np.array_equal(path, p2)
        out[name + "_post_path"] = np.asarray(path, dtype=np.int16)
        out[name + "_post_score"] = np.float64(score)
        # the same read with its log-posteriors taken in float64
        lp64 = np.log(prep.astype(np.float64) + oc.ETA)
        s64, _ = olddecode.decode_profile(lp64, trans=np.log(oc.ETA + trans), log=True)
        out[name + "_post_score64"] = np.float64(s64)
        score_rel = max(score_rel, abs(float(score) - float(s64)) / abs(float(s64)))
        # fragility: +-4 float32 ulps on the log-posteriors the reference itself forms
        lp32 = np.log(prep + np.float32(oc.ETA))
        sign = np.random.RandomState(seed + 2000).randint(0, 2, size=lp32.shape) * 2 - 1
        moved = (lp32 + sign * 4 * np.spacing(np.abs(lp32))).astype(np.float32)
        _, p3 = olddecode.decode_profile(moved, trans=np.log(oc.ETA + trans), log=True)
        frag = not np.array_equal(p3, path)
        out[name + "_fragile"] = np.int32(frag)
        compared += 1
        if frag:
            fragile.append(name)
    assert len(fragile) <= MAX_FRAGILE * compared, "too many fragile cases: %s of %d" % (fragile, compared)
    out["e_ref"] = np.float64(e_ref)
    out["score_rel_ref"] = np.float64(score_rel)
    out["numpy_version"] = np.asarray(np.__version__)
    path = os.path.join(OUT, "olddecode.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    largest = max(os.path.getsize(os.path.join(OUT, f)) for f in os.listdir(OUT) if f.endswith(".npz") and f != "olddecode.npz")
    assert size <= min(MAX_BYTES, largest), "%d bytes: larger than the cap of %d" % (size, min(MAX_BYTES, largest))
    print("%s: %d arrays, %d bytes; numpy %s; e_ref = %.3e, score_rel_ref = %.3e, fragile: %s of %d"
          % (path, len(out), size, np.__version__, e_ref, score_rel, fragile or "none", compared))


if __name__ == "__main__":
    main()
