"""The host side of the per-base qualities (design/lattice_marginals.md), without a GPU: the Phred threshold table and the search
that restates the device's counting rule, FASTQ text, the QUAL field of a SAM record, and the counting core of
align.quality_calibration on hand-made alignment columns."""
import numpy as np
import pytest

from sloika_amd import align, bio

M, X, I, D = align.OP_MATCH, align.OP_MISMATCH, align.OP_INSERTION, align.OP_DELETION


def test_threshold_table():
    t = bio.phred_thresholds()
    assert t.dtype == np.float64 and t.shape == (60,)
    assert t[9] == 0.1 and t[19] == 0.01 and t[0] == 10.0 ** -0.1
    assert (np.diff(t) < 0).all()
    assert bio.phred_thresholds(93).shape == (93,) and (bio.phred_thresholds(93)[:60] == t).all()
    for bad in (0, 94, -1):
        with pytest.raises(ValueError):
            bio.phred_thresholds(bad)


def test_phred_of_error_counts_thresholds():
    """The device's rule, spelled out: the number of k in 1 .. qmax with err <= 10^(-k/10)."""
    t = bio.phred_thresholds(60)
    errs = np.concatenate([[0.0, 1.0, 0.5, 0.1, np.nextafter(0.1, 1), np.nextafter(0.1, 0), 1e-6, 1e-7, 1e-300, np.nan, 2.0], t,
                           np.nextafter(t, 1), np.nextafter(t, 0)])
    want = np.array([0 if np.isnan(e) else int(sum(e <= v for v in t)) for e in errs])
    got = bio.phred_of_error(errs, 60)
    assert got.dtype == np.int64 and (got == want).all()
    assert got[0] == 60 and got[1] == 0 and got[3] == 10 and got[4] == 9 and got[5] == 10 and got[6] == 60 and got[9] == 0
    assert (bio.phred_of_error(errs, 20) == np.minimum(want, 20)).all()


def test_fastq_text():
    text = bio.fastq_text(["a", "b c"], ["ACGT", b"GG"], [np.array([0, 10, 60, 93]), [40, 41]])
    assert text == "@a\nACGT\n+\n!+]~\n@b c\nGG\n+\nIJ\n"
    assert bio.fastq_text([], [], []) == ""
    assert bio.fastq_text(["e"], [""], [np.zeros(0, np.uint8)]) == "@e\n\n+\n\n"
    with pytest.raises(ValueError):
        bio.fastq_text(["a"], ["ACGT"], [[1, 2, 3]])
    with pytest.raises(ValueError):
        bio.fastq_text(["a"], ["AC"], [[1, 94]])
    with pytest.raises(ValueError):
        bio.fastq_text(["a", "b"], ["AC"], [[1, 2]])


def test_sam_record_qual():
    row = [4, 1, 5, 10, 14, 4, 0, 0, 0]
    codes = np.array([M, M, M, M], dtype=np.uint8)
    plain = align.sam_record("r", row, '+', codes, 6, "ref", seq="AACGTA").split("\t")
    assert plain[10] == "*"
    fwd = align.sam_record("r", row, '+', codes, 6, "ref", seq="AACGTA", qual="!+5?IJ").split("\t")
    assert fwd[9] == "AACGTA" and fwd[10] == "!+5?IJ" and fwd[:9] == plain[:9] and fwd[11:] == plain[11:]
    rev = align.sam_record("r", row, '-', codes, 6, "ref", seq="AACGTA", qual="!+5?IJ").split("\t")
    assert rev[9] == "TACGTT" and rev[10] == "JI?5+!"
    un = align.sam_record("r", [0] * 9, '+', codes[:0], 6, "ref", seq="AACGTA", qual="!+5?IJ").split("\t")
    assert un[1] == "4" and un[10] == "!+5?IJ"
    with pytest.raises(ValueError):
        align.sam_record("r", row, '+', codes, 6, "ref", seq="AACGTA", qual="!!")
    with pytest.raises(ValueError):
        align.sam_record("r", row, '+', codes, 6, "ref", qual="!!!!!!")


def test_calibration_counts():
    # pair 0: letters 0-1 clipped, then = X I I D = (letters 2 .. 6), letter 7 clipped
    # pair 1: an empty alignment;  pair 2: deletions only in front of one match, from letter 0
    columns = [np.array([M, X, I, I, D, M], dtype=np.uint8), np.zeros(0, dtype=np.uint8), np.array([D, D, M], dtype=np.uint8)]
    quals = [np.array([60, 60, 10, 10, 3, 4, 10, 60]), np.array([7, 7, 7]), np.array([0, 5])]
    counts = align.calibration_counts(columns, [2, 0, 0], quals, qmax=60)
    assert counts.dtype == np.int64 and counts.shape == (61, 2)
    want = np.zeros((61, 2), dtype=np.int64)
    want[10] = [2, 1]                                       # letters 2 (=), 6 (=) right; letter 3 (X) wrong
    want[3] = [0, 1]                                        # the insertion run: letters 4 and 5
    want[4] = [0, 1]
    want[0] = [1, 0]                                        # pair 2's match is letter 0
    assert (counts == want).all()
    assert counts.sum() == 6                                # the clipped letters (Phred 60, 5) and pair 1 count nowhere
    assert (align.calibration_counts([], [], [], qmax=5) == 0).all()
    with pytest.raises(ValueError):
        align.calibration_counts([columns[0]], [4], [quals[0]])              # runs past the query's end
    with pytest.raises(ValueError):
        align.calibration_counts([columns[0]], [2], [quals[0]], qmax=9)      # a quality above qmax
    with pytest.raises(ValueError):
        align.calibration_counts(columns, [2, 0], quals)


def test_calibration_table():
    counts = np.zeros((4, 2), dtype=np.int64)
    counts[1] = [9, 1]
    counts[2] = [99, 1]
    counts[3] = [5, 0]
    t = align.calibration_table(counts)
    assert np.isnan(t[0]) and t[1] == pytest.approx(10.0) and t[2] == pytest.approx(20.0) and np.isinf(t[3])
