"""Read accuracy, host side: the alignment oracle (tests/align_ref.py) on hand-worked cases and against a carried-count pass,
sloika_amd.align's accuracy rows and summary on hand-computed numbers, and its argument refusals (no GPU needed)."""
import numpy as np
import pytest

from tests import align_ref as ref


# ---- the oracle on hand-worked cases ------------------------------------------------------------------------------------

def test_identical_strings():
    assert ref.align("ACGTACGTAC", "ACGTACGTAC") == [10, 0, 10, 0, 10, 10, 0, 0, 0]
    assert ref.align("acgtacgtac", b"ACGTACGTAC")[0] == 10            # str input is upper-cased


def test_one_planted_mismatch():
    #          ACGTACGT A CGTACGTA   8 matches, 1 mismatch (-2), 8 matches
    assert ref.align("ACGTACGTACGTACGTA", "ACGTACGTTCGTACGTA") == [14, 0, 17, 0, 17, 16, 1, 0, 0]


def test_one_planted_insertion():
    # the query holds one letter (G) the reference lacks: 16 matches - (2 + 1)
    q = "ACCATGTCA" + "G" + "TTCAGCA"
    r = "ACCATGTCA" + "TTCAGCA"
    assert ref.align(q, r) == [13, 0, 17, 0, 16, 16, 0, 1, 0]


def test_one_planted_deletion():
    # the reference holds two letters the query lacks: 16 matches - (2 + 2)
    q = "ACCATGTCA" + "TTCAGCA"
    r = "ACCATGTCA" + "GG" + "TTCAGCA"
    assert ref.align(q, r) == [12, 0, 16, 0, 18, 16, 0, 0, 2]


def test_no_common_letter_is_the_empty_alignment():
    assert ref.align("AAAA", "CCCCCC") == [0] * 9
    assert ref.align("", "ACGT") == [0] * 9
    assert ref.align("ACGT", "") == [0] * 9


def test_homopolymer_pair_by_the_tie_rules():
    """q = AAA, r = AAAAA: with no mismatch anywhere H[i][j] = min(i, j) (a gap never pays: it costs 3 to save nothing).  The
    maximum 3 fills row 3 from column 3 on; smallest i, then smallest j ends the alignment in (3, 3), and on the way back the
    diagonal attains every value, so it wins over the gaps that do not: start (0, 0), three matches."""
    assert ref.align("AAA", "AAAAA") == [3, 0, 3, 0, 3, 3, 0, 0, 0]
    # the other way round the 3 fills COLUMN 3 from row 3 on: smallest i picks (3, 3) again, not a later row
    assert ref.align("AAAAA", "AAA") == [3, 0, 3, 0, 3, 3, 0, 0, 0]


def test_dinucleotide_repeat_pair_by_the_tie_rules():
    """q = ACACAC, r = ACA|ACAC (an A too many after three letters).  Bridging the extra A costs O + E = 3 and joins ACA (3) to
    what follows: never more than the 4 of ACAC alone, which sits in r[3:7].  H reaches 4 first in row 4, column 7 (q[0:4]
    against r[3:7]); rows 5 and 6 reach 4 again at (6, 7) but smallest i decides.  Four matches, no gap."""
    assert ref.align("ACACAC", "ACAACAC") == [4, 0, 4, 3, 7, 4, 0, 0, 0]
    # with (AC)x6 against (AC)x3 A (AC)x3 the gap pays: 12 matches - 3 = 9 in the last cell (12, 13), the only 9.  Walking back,
    # six letters match diagonally down to (7, 8) = 4, whose diagonal predecessor is (6, 7) = 3.  There q[5] = C meets the extra
    # A: the diagonal offers H[5][6] - 2 = 0, E offers H[6][6] - 3 = 3, so the A is deleted, and (6, 6) = 6 is six more matches.
    assert ref.align("AC" * 6, "AC" * 3 + "A" + "AC" * 3) == [9, 0, 12, 0, 13, 12, 0, 0, 1]


# ---- traceback against carried counts -----------------------------------------------------------------------------------

def carried(q, r, A=1, B=2, O=2, X=1):
    """The same optimum with NO matrices kept: every value carries (q_start, r_start, mismatches, insertions) from the predecessor
    the tie rules pick; matches and deletions follow from where the alignment ends."""
    q, r = ref.as_bytes(q), ref.as_bytes(r)
    n, m = len(q), len(r)
    oe = O + X
    Hrow = [(0, (0, j, 0, 0)) for j in range(m + 1)]
    Frow = [(ref.NEG, (0, 0, 0, 0))] * (m + 1)
    best = (0, 0, 0, (0, 0, 0, 0))
    for i in range(1, n + 1):
        newH = [(0, (i, 0, 0, 0))]
        e = (ref.NEG, (0, 0, 0, 0))
        for j in range(1, m + 1):
            left = newH[j - 1]
            e = (left[0] - oe, left[1]) if left[0] - oe >= e[0] - X else (e[0] - X, e[1])
            up, f = Hrow[j], Frow[j]
            f = (up[0] - oe, up[1]) if up[0] - oe >= f[0] - X else (f[0] - X, f[1])
            f = (f[0], (f[1][0], f[1][1], f[1][2], f[1][3] + 1))
            Frow[j] = f
            dg = Hrow[j - 1]
            same = q[i - 1] == r[j - 1]
            h = (dg[0] + (A if same else -B), (dg[1][0], dg[1][1], dg[1][2] + (0 if same else 1), dg[1][3]))
            if e[0] > h[0]:
                h = e
            if f[0] > h[0]:
                h = f
            if h[0] <= 0:
                h = (0, (i, j, 0, 0))
            newH.append(h)
            if h[0] > best[0]:
                best = (h[0], i, j, h[1])
        Hrow = newH
    score, qe, re, (qs, rs, mm, ins) = best
    if score == 0:
        return [0] * 9
    match = qe - qs - mm - ins
    return [score, qs, qe, rs, re, match, mm, ins, re - rs - match - mm]


def test_traceback_agrees_with_carried_counts_on_random_pairs():
    rs = np.random.RandomState(5)
    gaps = 0
    for k in range(200):
        n, m = rs.randint(0, 41), rs.randint(0, 61)
        nletters = 2 if k % 3 == 0 else 4                     # two letters: many ties
        q = bytes(bytearray(b"ACGT"[c] for c in rs.randint(0, nletters, size=n)))
        r = bytes(bytearray(b"ACGT"[c] for c in rs.randint(0, nletters, size=m)))
        scores = (1, 2, 2, 1) if k % 2 == 0 else ((3, 1, 5, 2) if k % 4 == 1 else (2, 3, 0, 1))
        want = ref.align(q, r, *scores)
        assert carried(q, r, *scores) == want, (q, r, scores)
        assert want[0] == ref.score_only(q, r, *scores)
        if want[0]:
            assert want[2] - want[1] == want[5] + want[6] + want[7] and want[4] - want[3] == want[5] + want[6] + want[8]
            assert want[0] <= scores[0] * want[5]
        gaps += want[7] + want[8]
    assert gaps > 50                                          # the pairs exercise E and F, not only the diagonal


# ---- accuracy rows and summary ------------------------------------------------------------------------------------------

def test_samacc_rows_by_hand():
    from sloika_amd import align
    res = np.array([
        [80, 0, 100, 5, 103, 90, 4, 6, 4],        # a usual row
        [50, 0, 50, 0, 50, 50, 0, 0, 0],          # perfect: NM = 0, no log of 0
        [2, 0, 10, 0, 40, 2, 6, 2, 30],           # NM / readlen = 38 / 10 -> capped at 0.75
        [30, 10, 40, 0, 30, 30, 0, 0, 0],         # coverage 30 / 100 = 0.3: dropped
        [0, 0, 0, 0, 0, 0, 0, 0, 0],              # empty: dropped
        [0, 0, 0, 0, 0, 0, 0, 0, 0],              # a read of no letters: dropped
        [9, 0, 10, 0, 10, 9, 0, 1, 1],            # mismatch == 0 but NM = 2: the second entropy term applies
    ], dtype=np.int32)
    rows = align.samacc_rows(res, ['+', '-', '+', '+', '+', '+', '-'], [100, 50, 10, 100, 20, 0, 10], names=list("abcdefg"))
    assert [r['query'] for r in rows] == ['a', 'b', 'c', 'g']
    a, b, c, g = rows
    assert a['strand'] == '+' and b['strand'] == '-'
    assert (a['reference_start'], a['reference_end']) == (5, 103)
    assert (a['match'], a['mismatch'], a['insertion'], a['deletion']) == (90, 4, 6, 4)
    assert a['coverage'] == 1.0 and a['id'] == 90 / 94 and a['accuracy'] == 90 / 104
    perr = 14 / 100
    assert a['information'] == pytest.approx(94 * (2 + (1 - perr) * np.log2(1 - perr) + perr * np.log2(perr / 3)), rel=1e-12)
    assert b['id'] == 1.0 and b['accuracy'] == 1.0 and b['information'] == 100.0      # 50 * (2 + 1 * log2 1)
    assert c['accuracy'] == 2 / 40 and c['id'] == 0.25
    assert c['information'] == pytest.approx(8 * (2 + 0.25 * np.log2(0.25) + 0.75 * np.log2(0.25)), rel=1e-12)   # = 0 bits
    perr = 2 / 10
    assert g['information'] == pytest.approx(9 * (2 + 0.8 * np.log2(0.8) + 0.2 * np.log2(0.2 / 3)), rel=1e-12)
    assert g['accuracy'] == 9 / 11
    assert len(align.samacc_rows(res, ['+'] * 7, [100, 50, 10, 100, 20, 0, 10], min_coverage=0.0)) == 5
    assert [r['query'] for r in align.samacc_rows(res[:1], ['+'], [100])] == [0]


def test_summary_by_hand():
    from sloika_amd import align
    assert align.summary([]) == {'mapped': 0}
    accs = [0.80, 0.85, 0.91, 0.95, 0.99]
    rows = [{'query': k, 'accuracy': a, 'information': 1e5 * (k + 1)} for k, a in enumerate(accs)]
    s = align.summary(rows)
    assert s['mapped'] == 5 and s['mean'] == pytest.approx(0.9)
    assert s['quantiles'][50] == 0.91 and s['quantiles'][25] == 0.85 and s['quantiles'][75] == 0.95
    assert s['quantiles'][5] == pytest.approx(0.81) and s['quantiles'][95] == pytest.approx(0.982)
    assert s['proportion_gt_90'] == 0.6 and s['count_gt_90'] == 3
    assert s['ciscore_mbits'] == pytest.approx(1.5)


# ---- refusals -----------------------------------------------------------------------------------------------------------

def test_argument_refusals():
    from sloika_amd import align
    with pytest.raises(ValueError, match="65535"):
        align.align_batch(["A" * 65536], ["ACGT"])
    with pytest.raises(ValueError, match="65535"):
        align.align_batch(["ACGT"], [np.zeros(65536, dtype=np.uint8)])
    for kw in ({"match": 0}, {"match": -1}, {"gap_extend": 0}, {"gap_extend": -2}, {"mismatch": -1}, {"gap_open": -1},
               {"match": 16385}):
        with pytest.raises(ValueError):
            align.align_batch(["ACGT"], ["ACGT"], **kw)
    with pytest.raises(ValueError, match="2 queries but 1 references"):
        align.align_batch(["ACGT", "AC"], ["ACGT"])
    with pytest.raises(ValueError):
        align.align_batch([np.zeros(4, dtype=np.int32)], ["ACGT"])


def test_c_entry_refuses_by_code_not_by_truncation():
    """The C entry checks its host arguments before it touches a pointer or the device, so this runs without a GPU."""
    from sloika_amd import _lib, build
    build.build()
    L = _lib.lib()
    P = L.slk_align_pass_width()
    assert P >= 64 and P % 64 == 0
    bad = _lib.SLK_ERR_INVALID_ARG
    assert L.slk_align_local_batch_u8(None, 0, None, None, None, 1, 65536, 10, 1, 2, 2, 1, None, None, 0, None) == bad
    assert L.slk_align_local_batch_u8(None, 0, None, None, None, 1, 10, 65536, 1, 2, 2, 1, None, None, 0, None) == bad
    assert L.slk_align_local_batch_u8(None, 0, None, None, None, 1, 10, 10, 0, 2, 2, 1, None, None, 0, None) == bad
    assert L.slk_align_local_batch_u8(None, 0, None, None, None, 1, 10, 10, 1, 2, 2, 0, None, None, 0, None) == bad
    assert L.slk_align_local_batch_u8(None, 0, None, None, None, 1, 10, 10, 1, 2, 2, 1, None, None, 0, None) == bad   # null pointers
    assert L.slk_align_local_workspace_bytes(7, 1000, P) == 0
    assert L.slk_align_local_workspace_bytes(7, 1000, P + 1) == 7 * 1000 * 24
    assert L.slk_align_local_workspace_bytes(7, 65536, P + 1) == 0
    assert L.slk_revcomp_u8(None, None, -1, 4, None, None) == bad


def test_align_batch_needs_a_gpu():
    import torch
    from sloika_amd import _lib, align, build
    build.build()
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    with pytest.raises(_lib.SloikaAmdError):
        align.align_batch(["ACGT"], ["ACGT"])
