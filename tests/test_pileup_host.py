"""The rules of design/pileup.md section 1 as the plain-loop model of tests/pileup_ref.py states them: hand cases with the expected
codes written out, properties over random alignments, strand symmetry, the call rules, and the planted-variant case that shows
what gap normalisation is for.  No GPU: the device is held against this same model in tests/test_gpu_pileup.py."""
import numpy as np
import pytest

from tests import align_ops_ref, pileup_cases
from tests import pileup_ref as R

M, X, I, D = R.MATCH, R.MISMATCH, R.INSERTION, R.DELETION


def _norm(q, r, codes):
    row = [1, 0, len(q), 0, len(r)] + [sum(1 for c in codes if c == k) for k in range(4)]
    f, _, _ = R.forward_view(q, r, row, codes, False)
    return R.normalise(f, *R.forward_bytes(q, r, row, False))


def test_deletion_in_homopolymer_ends_at_its_first_letter():
    assert _norm("CAAAAAG", "CAAAAAAG", [M, M, M, M, D, M, M, M]) == [M, D, M, M, M, M, M, M]


def test_two_letter_insertion_in_repeat_rotates():
    q, r = "GCACACAT", "GCACAT"
    got = _norm(q, r, [M, M, I, I, M, M, M, M])                  # the inserted letters are AC ...
    assert got == [M, I, I, M, M, M, M, M]                       # ... and CA once the run stands behind the G
    counts, ins = R.tables(len(r), 2)
    R.count(counts, ins, got, [R.letter_class(c) for c in q.encode()], 0, 0, len(r))
    assert ins[0] == [[0, 1, 0, 0, 0], [1, 0, 0, 0, 0]] and counts[0][R.INS_READS] == 1
    assert _norm(q, r, [M, M, M, M, M, I, I, M]) == [M, I, I, M, M, M, M, M]


def test_run_stops_at_the_alignments_start():
    assert _norm("AAT", "AAAT", [M, M, D, M]) == [D, M, M, M]


def test_run_stops_at_a_mismatch_that_breaks_the_letter_test():
    assert _norm("TAGAAC", "TAAAC", [M, M, X, M, I, M]) == [M, M, X, I, M, M]
    # a mismatch whose letters pass the test moves like a match, and stays a mismatch
    assert _norm("TAGAC", "TAAAAC", [M, M, X, M, D, M]) == [M, D, M, X, M, M]


def test_run_stops_against_an_earlier_gap():
    assert _norm("CGAAT", "CAAAT", [M, I, M, M, D, M]) == [M, I, D, M, M, M]


def _mutate(rs, s, rate):
    out = []
    for c in s:
        u = rs.random_sample()
        if u < rate / 3:
            out.append("ACGT"[rs.randint(0, 4)])
        elif u < 2 * rate / 3:
            out.append(c + "ACGT"[rs.randint(0, 4)])
        elif u >= rate:
            out.append(c)
    return ''.join(out)


def _random_pairs(seed, n):
    rs = np.random.RandomState(seed)
    for _ in range(n):
        # few letters and short repeats: many gaps have somewhere to go
        ref = ''.join(rs.choice(list("AC"), p=[0.6, 0.4]) if rs.random_sample() < 0.7 else "ACGT"[rs.randint(0, 4)]
                      for _ in range(int(rs.randint(30, 90))))
        q = _mutate(rs, ref[int(rs.randint(0, 8)):len(ref) - int(rs.randint(0, 8))], 0.25)
        row, codes = align_ops_ref.ops(q, ref)
        if row[0] > 0:
            yield q, ref, row, codes


def test_normalised_columns_still_align_the_same_letters():
    moved = 0
    for q, r, row, codes in _random_pairs(11, 60):
        for minus in (False, True):
            if minus:                                            # aligned on the other strand: the aligner's gaps sit at the other end
                q2, r2 = R.revcomp(q).decode(), R.revcomp(r).decode()
                row2, codes2 = align_ops_ref.ops(q2, r2)
            else:
                q2, r2, row2, codes2 = q, r, row, codes
            f, _, _ = R.forward_view(q2, r2, row2, codes2, minus)
            Q, Rb = R.forward_bytes(q2, r2, row2, minus)
            g = R.normalise(f, Q, Rb)
            assert [g.count(k) for k in range(4)] == [f.count(k) for k in range(4)]
            i = j = 0
            for c in g:
                if c in (M, X):
                    assert (Q[i] == Rb[j]) == (c == M)
                i += c != D
                j += c != I
            assert (i, j) == (len(Q), len(Rb))
            moved += g != f
    assert moved > 20                                            # the cases do exercise the pass


def test_strand_symmetry():
    """A pair and its mirror image give identical tables."""
    G, S = 120, 3
    for q, r, row, codes in _random_pairs(12, 40):
        t0 = 7 + row[3]
        mirror = (R.revcomp(q).decode(), R.revcomp(r).decode(),
                  [row[0], len(q) - row[2], len(q) - row[1], len(r) - row[4], len(r) - row[3]] + list(row[5:]), codes[::-1], True, t0)
        a = R.pile([(q, r, row, codes, False, t0)], 0, G, S)
        b = R.pile([mirror], 0, G, S)
        assert a == b


def test_call_rules():
    z = [[0] * 5 for _ in range(2)]
    # the greatest count wins; LOW below min_depth keeps the reference letter, whatever it is
    assert R.call([1, 5, 0, 0, 0, 0, 0, 5], z, ord('A')) == (b"C", R.CHANGED)
    assert R.call([1, 1, 0, 0, 0, 0, 0, 1], z, ord('N')) == (b"N", R.LOW)
    assert R.call([1, 1, 0, 0, 0, 0, 0, 1], z, ord('G'), min_depth=2) == (b"A", R.CHANGED)
    # a tie goes to the reference letter's class if it is among the tied ...
    assert R.call([2, 0, 0, 2, 0, 2, 0, 5], z, ord('T')) == (b"T", 0)
    # ... else to the first of A C G T deletion
    assert R.call([0, 2, 0, 2, 0, 2, 0, 5], z, ord('A')) == (b"C", R.CHANGED)
    assert R.call([0, 0, 0, 1, 0, 3, 0, 3], z, ord('T')) == (b"", R.CHANGED)
    assert R.call([0, 0, 2, 0, 0, 2, 0, 3], z, ord('G'), min_depth=1) == (b"G", 0)
    # a reference letter that is none of A C G T takes part in no tie, and is not the deletion
    assert R.call([1, 1, 0, 0, 0, 1, 0, 3], z, ord('N')) == (b"A", R.CHANGED)
    assert R.call([0, 0, 0, 0, 0, 3, 0, 3], z, ord('N')) == (b"", R.CHANGED)
    # nothing but other letters: nothing to call
    assert R.call([0, 0, 0, 0, 6, 0, 0, 6], z, ord('C')) == (b"C", R.LOW)
    # an insertion at exactly half the span is not emitted, one above it is; the second letter needs its own majority
    assert R.call([6, 0, 0, 0, 0, 0, 3, 6], [[0, 0, 3, 0, 0], [0, 0, 3, 0, 0]], ord('A')) == (b"A", 0)
    assert R.call([6, 0, 0, 0, 0, 0, 4, 6], [[0, 0, 3, 0, 1], [0, 0, 3, 0, 0]], ord('A')) == (b"AG", R.INSERTED)
    assert R.call([6, 0, 0, 0, 0, 0, 4, 6], [[0, 2, 2, 0, 0], [0, 0, 0, 4, 0]], ord('A')) == (b"ACT", R.INSERTED)
    assert R.call([6, 0, 0, 0, 0, 0, 4, 6], [[0, 0, 0, 0, 4], [0, 0, 0, 4, 0]], ord('A')) == (b"A", 0)
    # no insertion is emitted at a LOW position
    assert R.call([1, 0, 0, 0, 0, 0, 1, 1], [[0, 0, 1, 0, 0], [0, 0, 0, 0, 0]], ord('A')) == (b"A", R.LOW)


def test_insertion_in_front_of_the_first_reference_letter_is_counted_nowhere():
    counts, ins = R.tables(4, 2)
    R.count(counts, ins, [I, M, M, I, I, I, M], [0, 1, 2, 3, 3, 3, 0], 1, 0, 4)
    assert [c[R.INS_READS] for c in counts] == [0, 0, 1, 0] and ins[2] == [[0, 0, 0, 1, 0], [0, 0, 0, 1, 0]]
    assert [c[R.SPAN] for c in counts] == [0, 1, 1, 0] and [sum(c[:6]) for c in counts] == [0, 1, 1, 1]


@pytest.fixture(scope="module")
def planted_tables():
    case, pairs = pileup_cases.planted(), pileup_cases.host_pairs()
    G = len(case['genome'])
    return {norm: R.pile(pairs, 0, G, 4, norm) for norm in (True, False)}


def test_planted_variants_need_normalisation(planted_tables):
    case = pileup_cases.planted()
    G = len(case['genome'])
    assert sorted(set(case['strands'])) == ['+', '-']
    counts, ins, views = planted_tables[True]
    cons, _, flags = R.consensus(counts, ins, case['genome'], 0, 3)
    assert cons.decode('ascii') == case['sample']
    assert [v[:5] for v in R.variants(counts, ins, case['genome'], 0, [0, G], [pileup_cases.CONTIG])] == case['variants']
    assert any(f & R.LOW for f in flags) or min(sum(c[:6]) for c in counts) >= 3
    counts, ins, raw = planted_tables[False]
    assert R.consensus(counts, ins, case['genome'], 0, 3)[0].decode('ascii') != case['sample']
    assert raw != views
