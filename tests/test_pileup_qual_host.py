"""The rules of design/pileup.md section 9 as the plain-loop model of tests/pileup_qual_ref.py states them: the designed case that
shows what a quality-weighted vote is for, all-ones weights against the plain model, min_qual, hand-made single positions for every
rule of the weighted call, and the FASTQ reader.  No GPU: the device is held against this same model in
tests/test_gpu_pileup_qual.py."""
import numpy as np
import pytest

from sloika_amd import bio
from tests import pileup_cases, pileup_qual_cases
from tests import pileup_qual_ref as Q
from tests import pileup_ref as R


def test_designed_case_majority_fails_weighted_recovers_the_sample():
    case, pairs = pileup_qual_cases.designed(), pileup_qual_cases.host_pairs()
    G = len(case['genome'])
    assert sorted(set(case['strands'])) == ['+', '-']
    assert all(len(q) == len(r) for q, r in zip(case['quals'], case['reads']))
    counts, ins, wcounts, wins, _ = Q.pile(pairs, 0, G, 4, Q.weights_table())
    majority = R.consensus(counts, ins, case['genome'], 0, 3)[0].decode('ascii')
    weighted, parts, _, quals, _ = Q.consensus(counts, wcounts, wins, case['genome'], 0, 3)
    assert majority != case['sample']
    assert weighted.decode('ascii') == case['sample']
    assert [len(p) for p in parts] == [len(v) for v in quals]
    # the plain tables are the plain model's
    c2, i2, _ = R.pile([p[:6] for p in pairs], 0, G, 4, True)
    assert (counts, ins) == (c2, i2)


def test_all_ones_weights_reproduce_the_plain_model():
    case, plain = pileup_cases.planted(), pileup_cases.host_pairs()
    G = len(case['genome'])
    rs = np.random.RandomState(3)
    pairs = [p + (rs.randint(0, 256, size=len(p[0])).astype(np.uint8),) for p in plain]
    assert all(int(p[2][2]) > int(p[2][1]) for p in pairs)       # every alignment has a query letter (the one exception of section 9)
    for norm in (True, False):
        counts, ins, wcounts, wins, views = Q.pile(pairs, 0, G, 4, [1] * 256, norm)
        c2, i2, v2 = R.pile(plain, 0, G, 4, norm)
        assert (counts, ins, views) == (c2, i2, v2)
        assert (wcounts, wins) == (counts, ins)
        text, parts, flags, _, _ = Q.consensus(counts, wcounts, wins, case['genome'], 0, 3)
        assert (text, parts, flags) == R.consensus(c2, i2, case['genome'], 0, 3)


def test_min_qual_zeroes_exactly_the_letters_below_it():
    assert Q.weights_table(7, 40) == [0] * 7 + list(range(7, 40)) + [40] * 216
    assert Q.weights_table() == list(range(60)) + [60] * 196
    pairs = pileup_qual_cases.host_pairs()[:12]
    G = len(pileup_qual_cases.designed()['genome'])
    _, _, w_all, i_all, _ = Q.pile(pairs, 0, G, 4, Q.weights_table(0, 60))
    _, _, w_cut, i_cut, _ = Q.pile(pairs, 0, G, 4, Q.weights_table(10, 60))
    # the same pile with the doubtful letters' qualities set to 0 by hand
    zeroed = [p[:6] + (np.where(p[6] < 10, 0, p[6]).astype(np.uint8),) for p in pairs]
    assert any((p[6] < 10).any() for p in pairs)
    _, _, w_hand, i_hand, _ = Q.pile(zeroed, 0, G, 4, Q.weights_table(0, 60))
    assert (w_cut, i_cut) == (w_hand, i_hand) and (w_cut, i_cut) != (w_all, i_all)


def test_column_weights_by_hand():
    M, X, I, D = R.MATCH, R.MISMATCH, R.INSERTION, R.DELETION
    wt = Q.weights_table()
    # forward letters ACGT with qualities 10 20 30 40; columns M D M I M against the reference AGCT
    q, r = "ACGT", "AGCT"
    row = [1, 0, 4, 0, 4, 3, 0, 1, 1]
    qual = np.array([10, 20, 30, 40], dtype=np.uint8)
    codes = [M, D, M, I, M]
    out = Q.pile([(q, r, row, codes, False, 0, qual)], 0, 4, 2, wt, normalised=False)
    wcounts, wins = out[2], out[3]
    assert [w[:6] for w in wcounts] == [[10, 0, 0, 0, 0, 0], [0, 0, 0, 0, 0, 10], [0, 20, 0, 0, 0, 0], [0, 0, 0, 40, 0, 0]]
    assert [w[6] for w in wcounts] == [0, 0, 30, 0] and [w[7] for w in wcounts] == [10, 10, 20, 0]
    assert wins[2] == [[0, 0, 30, 0, 0], [0, 0, 0, 0, 0]]
    # the same pair seen from the other strand: the qualities are read back to front with the letters
    mirror = (R.revcomp(q).decode(), R.revcomp(r).decode(), row, codes[::-1], True, 0, qual[::-1].copy())
    assert Q.pile([mirror], 0, 4, 2, wt, normalised=False)[:4] == out[:4]
    # a deletion as the first or the last column has one neighbour; an alignment without a query letter has none
    assert Q.deletion_weight([7, 9], 0) == 7 and Q.deletion_weight([7, 9], 2) == 9 and Q.deletion_weight([7, 9], 1) == 7
    assert Q.deletion_weight([], 0) == 0


def test_weighted_call_rules():
    z = [[0] * 5 for _ in range(2)]
    call = lambda cn, wn, wip, ref, **kw: Q.call_full(cn, wn, wip, ord(ref), **kw)[:2] + Q.call_full(cn, wn, wip, ord(ref), **kw)[4:]  # noqa: E731
    d6 = [6, 0, 0, 0, 0, 0, 0, 6]
    # the greatest WEIGHT wins, whatever the heads say; posq is the lead over the runner-up
    assert call([5, 1, 0, 0, 0, 0, 0, 6], [15, 30, 0, 0, 0, 0, 0, 45], z, 'A') == (b"C", R.CHANGED, [15], 15)
    # depth is the unweighted one
    assert call([1, 1, 0, 0, 0, 0, 0, 2], [40, 0, 0, 0, 0, 0, 0, 40], z, 'N') == (b"N", R.LOW, [0], 0)
    assert call([1, 1, 0, 0, 0, 0, 0, 2], [40, 0, 0, 0, 0, 0, 0, 40], z, 'G', min_depth=2) == (b"A", R.CHANGED, [40], 40)
    # zero weights under sufficient depth: LOW, the reference byte, quality 0
    assert call(d6, [0, 0, 0, 0, 9, 0, 0, 9], z, 'C') == (b"C", R.LOW, [0], 0)
    assert call(d6, [0] * 8, [[5, 0, 0, 0, 0], [0] * 5], 'T') == (b"T", R.LOW, [0], 0)
    # a tie goes to the reference letter's class if it is among the tied: posq 0
    assert call(d6, [20, 0, 0, 20, 0, 20, 0, 60], z, 'T') == (b"T", 0, [0], 0)
    # ... else to the first of A C G T deletion
    assert call(d6, [0, 20, 0, 20, 0, 20, 0, 60], z, 'A') == (b"C", R.CHANGED, [0], 0)
    assert call(d6, [0, 0, 20, 0, 0, 20, 0, 60], z, 'G') == (b"G", 0, [0], 0)
    assert call(d6, [0, 0, 20, 0, 0, 20, 0, 60], z, 'A') == (b"G", R.CHANGED, [0], 0)
    # a reference letter that is none of A C G T takes part in no tie
    assert call(d6, [7, 7, 0, 0, 0, 7, 0, 21], z, 'N') == (b"A", R.CHANGED, [0], 0)
    # the deletion wins: nothing is emitted, posq is written all the same
    assert call(d6, [0, 0, 0, 5, 0, 30, 0, 35], z, 'T') == (b"", R.CHANGED, [], 25)
    assert call(d6, [0, 0, 0, 0, 0, 30, 0, 30], z, 'N') == (b"", R.CHANGED, [], 30)
    # posq is capped at qmax
    assert call(d6, [200, 10, 0, 0, 0, 0, 0, 210], z, 'A') == (b"A", 0, [60], 60)
    assert call(d6, [200, 10, 0, 0, 0, 0, 0, 210], z, 'A', qmax=93) == (b"A", 0, [93], 93)
    assert call(d6, [200, 10, 0, 0, 0, 0, 0, 210], z, 'A', qmax=1) == (b"A", 0, [1], 1)
    # W_next comes from entry 4 when `other` is the runner-up; `other` never wins, and a lead below 0 is written as 0
    assert call(d6, [50, 10, 0, 0, 35, 0, 0, 95], z, 'A') == (b"A", 0, [15], 15)
    assert call(d6, [50, 10, 0, 0, 80, 0, 0, 140], z, 'A') == (b"A", 0, [0], 0)
    # an insertion at exactly half the span's weight is not emitted, one above it is
    assert call(d6, [100, 0, 0, 0, 0, 0, 50, 100], [[0, 0, 50, 0, 0], [0] * 5], 'A') == (b"A", 0, [60], 60)
    assert call(d6, [100, 0, 0, 0, 0, 0, 51, 100], [[0, 0, 51, 0, 0], [0] * 5], 'A') == (b"AG", R.INSERTED, [60, 2], 60)
    # its quality is 2 mx - span, clamped at 0 (a split insertion that `other` helps over the line) and at qmax
    assert call(d6, [100, 0, 0, 0, 0, 0, 70, 100], [[0, 30, 30, 0, 10], [0] * 5], 'A') == (b"AC", R.INSERTED, [60, 0], 60)
    assert call(d6, [100, 0, 0, 0, 0, 0, 90, 100], [[0, 0, 0, 90, 0], [0] * 5], 'A') == (b"AT", R.INSERTED, [60, 60], 60)
    # the stop at the first failing k: the third letter would pass, and is not reached
    three = [[0, 0, 0, 90, 0], [0, 40, 0, 0, 0], [90, 0, 0, 0, 0]]
    assert call(d6, [100, 0, 0, 0, 0, 0, 90, 100], three, 'A') == (b"AT", R.INSERTED, [60, 60], 60)
    # nothing but `other` letters at k = 0: no maximum above 0, nothing emitted
    assert call(d6, [100, 0, 0, 0, 0, 0, 90, 100], [[0, 0, 0, 0, 90], [0, 0, 0, 90, 0]], 'A') == (b"A", 0, [60], 60)
    # behind a deletion the insertion's letters are the position's only letters
    assert call(d6, [0, 0, 0, 0, 0, 100, 80, 100], [[0, 80, 0, 0, 0], [0] * 5], 'A') == (b"C", R.CHANGED | R.INSERTED, [60], 60)
    # sums near 2^30: 2 Wn and 2 mx are formed without wrapping
    big = 1 << 30
    assert call(d6, [big, 0, 0, 0, 0, 0, big, big + 5], [[big, 0, 0, 0, 0], [0] * 5], 'A') == (b"AA", R.INSERTED, [60, 60], 60)


def test_variants_with_quality():
    genome = "ACGT"
    counts = [[6, 0, 0, 0, 0, 0, 0, 6], [1, 5, 0, 0, 0, 0, 4, 6], [0, 0, 2, 0, 0, 4, 0, 6], [0, 0, 0, 6, 0, 0, 0, 0]]
    wcounts = [[90, 0, 0, 0, 0, 0, 0, 90], [30, 10, 0, 0, 0, 0, 70, 40], [0, 0, 5, 0, 0, 50, 0, 55], [0, 0, 0, 90, 0, 0, 0, 0]]
    wins = [[[0] * 5] * 2, [[0, 0, 0, 25, 0], [0, 0, 45, 0, 0]], [[0] * 5] * 2, [[0] * 5] * 2]
    got = Q.variants(counts, wcounts, wins, genome, 0, [0, 4], ["c"])
    assert got == [("c", 1, 'sub', 'C', 'A', 6, 1, 20), ("c", 1, 'ins', '', 'TG', 6, 4, 10), ("c", 2, 'del', 'G', '', 6, 4, 45)]


def test_fastq_records_round_trip_and_refusals():
    rs = np.random.RandomState(4)
    names = ["read_%d extra words" % k for k in range(5)]
    bases = [''.join("ACGTN"[v] for v in rs.randint(0, 5, size=n)) for n in (1, 0, 17, 64, 200)]
    quals = [rs.randint(0, 94, size=len(b)).astype(np.uint8) for b in bases]
    quals[2][:3] = (0, 93, 31)                                   # '!' , '~' and '@' among the quality characters
    text = bio.fastq_text(names, bases, quals)
    got = bio.fastq_records(text)
    assert [g[0] for g in got] == names and [g[1] for g in got] == bases
    assert all(g[2].dtype == np.uint8 and np.array_equal(g[2], q) for g, q in zip(got, quals))
    assert bio.fastq_text(*zip(*got)) == text
    assert bio.fastq_records("") == []
    repeated = bio.fastq_records("@r\nAC\n+r\n!5\n")             # the '+' line may repeat the name
    assert repeated[0][:2] == ("r", "AC") and repeated[0][2].tolist() == [0, 20]
    with pytest.raises(ValueError, match="record 2 "):
        bio.fastq_records("@a\nAC\n+\n!!\n@b\nACG\n+\n!!\n")
    with pytest.raises(ValueError, match="record 2 "):
        bio.fastq_records("@a\nAC\n+\n!!\nb\nAC\n+\n!!\n")
    with pytest.raises(ValueError, match="record 1 "):
        bio.fastq_records("@a\nAC\n-\n!!\n")
    with pytest.raises(ValueError, match="record 1 "):
        bio.fastq_records("@a\nAC\n+\n! \n")
    with pytest.raises(ValueError, match="record 2 "):
        bio.fastq_records("@a\nAC\n+\n!!\n@b\nAC\n")
