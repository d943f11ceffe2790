#!/usr/bin/env python3
"""Are the per-base qualities calibrated?  A record, not a promise (design/lattice_marginals.md 6).

    python tools/quality_calibration.py [--qmax 60] [--skip 5.0] [--trim 200 10]

Calls the two real reads of tests/golden/reads.npz with the pretrained fixture weights (pipeline.Basecaller.call_reads_qual),
aligns each call to the 1D basecall ONT's software left in the same fast5 file (the yardstick of tests/test_gpu_reads.py: another
basecaller, not the truth) and prints, per Phred value the calls carry, the letters that match and that do not
(align.quality_calibration) and the empirical Phred value of the bin (align.calibration_table).
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--qmax", type=int, default=60)
    ap.add_argument("--skip", type=float, default=5.0)
    ap.add_argument("--trim", type=int, nargs=2, default=(200, 10))
    a = ap.parse_args()
    from sloika_amd import align, bio, models, pipeline
    g = np.load(os.path.join(GOLDEN, "reads.npz"))
    net = models.from_weights_npz(os.path.join(GOLDEN, "pretrained_weights.npz"))
    signals, stored = [], []
    for n in (5, 3):
        dig, off, rng, _rate = g["meta_%d" % n]
        signals.append(((g["adc_%d" % n].astype(np.float64) + off) * (rng / dig)).astype(np.float32))
        stored.append(g["called_%d" % n].tobytes().decode())
    bc = pipeline.Basecaller(net, kmer_len=5, min_prob=1e-5, skip=a.skip)
    res = bc.call_reads_qual(signals, trim=tuple(a.trim))
    calls = bio.paths_to_bases_qual(res[1], res[2], res[4], 5, qmax=a.qmax)
    results, strand, ops = align.align_batch([c[0] for c in calls], stored, ops=True)
    counts = align.quality_calibration(ops, [c[1] for c in calls], qmax=a.qmax)
    table = align.calibration_table(counts)
    for b, (seq, q) in enumerate(calls):
        r = results[b]
        print("read %d: %d letters called, %d stored; aligned letters %d .. %d, %d match, %d mismatch, %d inserted, %d deleted; "
              "log Z %.1f; mean Phred %.1f" % (b, len(seq), len(stored[b]), r[1], r[2], r[5], r[6], r[7], r[8], float(res[5][b]),
                                              float(q.mean())))
    print("Phred   right   wrong  empirical")
    for q in range(a.qmax + 1):
        if counts[q].sum():
            print("%5d %7d %7d  %9.1f" % (q, counts[q, 0], counts[q, 1], table[q]))
    right, wrong = counts[:, 0].sum(), counts[:, 1].sum()
    print("  all %7d %7d  %9.1f" % (right, wrong, -10.0 * np.log10(max(wrong, 1) / float(right + wrong))))


if __name__ == "__main__":
    main()
