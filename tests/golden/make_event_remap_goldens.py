#!/usr/bin/env python3
"""Generate tests/golden/event_remap.npz by IMPORTING THE REFERENCE where a checkout of it exists (never on the GPU box, never from
tests):

    python tests/golden/make_event_remap_goldens.py

The reference is set up as make_goldens.py does it (stub modules for the packages it imports but that are absent, its
viterbi_helpers built in a temporary directory).  `batch.calc_post` -- a compiled Theano function in the reference, process-global
-- is replaced by a function that returns the case's seeded posterior (event_remap_cases.build); then the reference's own
`batch.remap` and `batch.chunkify` run on the case's event table and reference.  Only what they return is stored, per case <c>:

    <c>_digest                          sha256 of reference sequence, event columns and posterior (the tests regenerate and compare)
    <c>_score, <c>_score_hex            remap's score (float32), and float.hex() of it
    <c>_path, <c>_seq                   remap's path and the states + 1 of the reference's k-mers
    <c>_seq_pos, <c>_kmer, <c>_good     the three columns remap appends (in that order, after the table's own)
    <c>_chunks, <c>_labels, <c>_bad     chunkify of the table remap returns
    <c>_strand                          the seven strand-list fields of tools/chunkify_with_remap.py:57-58, each as str() gives it
    <c>_masked                          how many entries of the returned MaskedArray are masked (0)
A case whose decoded path does not show what the case names (event_remap_cases.unmet) is refused.
"""
import os
import sys

import numpy as np

OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, OUT)
import event_remap_cases as erc  # noqa: E402
import make_goldens as mg  # noqa: E402  (the reference set-up lives there)


def main():
    mg._setup_reference()
    import sloika.features  # noqa: F401  (batch.remap reaches it through the package)
    import sloika.transducer  # noqa: F401
    from sloika import batch
    out = {}
    for name in erc.NAMES:
        c = erc.build(name)
        batch.init_chunk_identity_worker(c["k"], erc.ALPHABET)
        post = c["post"]
        batch.calc_post = lambda inMat, post=post: post[:, None, :]
        assert not set(c["ev"].dtype.names) & {"kmer", "seq_pos", "good_emission"}
        score, ev, path, seq = batch.remap(c["ref"], c["ev"], erc.MIN_PROB, c["k"], c["prior"], c["slip"])
        miss = erc.unmet(c, path)
        if miss:
            raise SystemExit("case %s is vacuous: %s" % (name, "; ".join(miss)))
        assert list(seq) == list(c["states"])
        assert ev.dtype.names == c["ev"].dtype.names + ("seq_pos", "kmer", "good_emission")
        chunks, labels, bad = batch.chunkify(ev, c["chunk_len"], c["k"], c["use_scaled"], c["normalisation"])
        assert chunks.dtype == np.float32 and labels.dtype == np.int32 and bad.dtype == np.bool_
        nev = len(ev)
        # tools/chunkify_with_remap.py:57-58
        strand = [name + ".fast5", nev, -score / nev, np.sum(np.ediff1d(path, to_begin=1) == 0), len(seq), min(path), max(path)]
        out[name + "_digest"] = np.asarray(erc.digest(c))
        out[name + "_score"] = np.asarray(score)
        out[name + "_score_hex"] = np.asarray(float(score).hex())
        out[name + "_path"] = np.asarray(path)
        out[name + "_seq"] = np.asarray(seq, dtype=np.int64)
        out[name + "_seq_pos"] = np.ma.getdata(ev["seq_pos"])
        out[name + "_kmer"] = np.ma.getdata(ev["kmer"])
        out[name + "_good"] = np.ma.getdata(ev["good_emission"])
        out[name + "_masked"] = np.asarray(sum(int(np.ma.getmaskarray(ev[f]).sum()) for f in ev.dtype.names) if
                                           isinstance(ev, np.ma.MaskedArray) else -1)
        out[name + "_chunks"] = chunks
        out[name + "_labels"] = labels
        out[name + "_bad"] = bad
        out[name + "_strand"] = np.asarray([str(x) for x in strand])
        print("%-18s %4d events, %4d positions, score %.4f, %d stays, path %d..%d, labels %s, %s of score, %s of path" % (
            name, nev, len(seq), float(score), strand[3], strand[5], strand[6], labels.shape, np.asarray(score).dtype, path.dtype))
    path = os.path.join(OUT, "event_remap.npz")
    np.savez_compressed(path, **out)
    print("%s: %d arrays, %d bytes" % (path, len(out), os.path.getsize(path)))


if __name__ == "__main__":
    main()
