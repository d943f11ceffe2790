"""The alignments' columns, host side (no GPU needed): the column oracle (tests/align_ops_ref.py) against the counting oracle,
the band argument of design/align_traceback.md on the planted and the tie-ridden pairs, sloika_amd.align's CIGAR / SAM / summary
code on hand-written cases, a SAM record parsed back over its reference, and the new entry points' argument refusals."""
import ctypes

import numpy as np
import pytest

from tests import align_cases, align_ops_cases as cases, align_ops_ref as ref, align_ref


def _some_pairs():
    rs = np.random.RandomState(5)
    out = [("ACGTACGTAC", "ACGTACGTAC"), ("AAAA", "CCCCCC"), ("", "ACGT"), ("AAA", "AAAAA"), ("AC" * 6, "AC" * 3 + "A" + "AC" * 3)]
    for _ in range(12):
        r = align_cases.random_seq(rs, rs.randint(20, 120))
        out.append((align_cases.query_of(rs, r, rs.randint(1, 100)), r))
    return out + list(cases.edge_pairs()) + cases.tie_pairs(6)


def test_oracle_columns_count_to_the_nine_integers():
    for scores in ((1, 2, 2, 1), (3, 1, 5, 2)) + cases.TIE_SCORES:
        for q, r in _some_pairs():
            row, codes = ref.ops(q, r, *scores)
            assert row == align_ref.align(q, r, *scores), (q, r, scores)
            assert len(codes) == sum(row[5:9]) and codes.dtype == np.uint8


def test_band_restricted_dp_walks_the_same_columns():
    """The claim the device traceback rests on: the DP over the diagonals [-D, +I] of the aligned rectangle, anchored at the start
    cell, ends on the reported score and walks back the full traceback's columns -- also where ties decide the path."""
    todo = [(q, r, (1, 2, 2, 1)) for q, r in _some_pairs()] + [cases.width_pair(W) + ((1, 2, 2, 1),) for W in (1, 2, 63)]
    todo += [(q, r, s) for s in cases.TIE_SCORES + ((2, 3, 4, 1),) for q, r in cases.tie_pairs(12, seed=78)]
    todo.append(cases.wide_pair(257) + (cases.WIDE_SCORES,))
    live = 0
    for q, r, scores in todo:
        row, codes = ref.ops(q, r, *scores)
        if row[0] > 0:
            live += 1
            score, banded = ref.banded_ops(q, r, row, *scores)
            assert score == row[0] and np.array_equal(banded, codes), (q, r, scores)
    assert live > 50


def test_planted_pairs_have_their_width_and_touch_their_edges():
    for W in (1, 2, 63):
        row, _ = ref.ops(*cases.width_pair(W))
        assert row[7] + row[8] + 1 == W
    row, codes = ref.ops(*cases.wide_pair(257), *cases.WIDE_SCORES)
    assert row[7] + row[8] + 1 == 257 and ref.diagonal_range(codes)[1] == row[7]
    (q1, r1), (q2, r2) = cases.edge_pairs()
    row, codes = ref.ops(q1, r1)
    assert row[7] > 3 and row[8] > 3 and ref.diagonal_range(codes)[1] == row[7]
    row, codes = ref.ops(q2, r2)
    assert row[7] > 3 and row[8] > 3 and ref.diagonal_range(codes)[0] == -row[8]


def test_cigar_run_lengths_clips_and_reversal():
    from sloika_amd import align
    codes = np.array([0, 0, 1, 0, 2, 2, 0, 3, 0, 0], dtype=np.uint8)
    assert align.cigar_string(codes) == "2=1X1=2I1=1D2="
    assert align.cigar_string(codes, extended=False) == "4M2I1M1D2M"
    assert align.cigar_string(codes, False, 3, 0) == "3S4M2I1M1D2M"
    assert align.cigar_string(codes, False, 0, 5) == "4M2I1M1D2M5S"
    assert align.cigar_string(codes[::-1], False, 5, 3) == "5S2M1D1M2I4M3S"
    assert align.cigar_string(np.zeros(0, dtype=np.uint8)) == ""
    assert align.cigar_string([3]) == "1D" and align.cigar_string([1, 1], extended=False) == "2M"
    rs = np.random.RandomState(2)
    for _ in range(20):
        c = rs.randint(0, 4, size=rs.randint(1, 40)).astype(np.uint8)
        for ext in (True, False):
            assert align.cigar_string(c, ext, 2, 0) == ref.cigar(c, ext, 2, 0)


def test_profile_fields_and_error_summary():
    from sloika_amd import align
    assert len(align.PROFILE_FIELDS) == 68 and len(set(align.PROFILE_FIELDS)) == 68
    assert align.PROFILE_FIELDS[0] == "A/A" and align.PROFILE_FIELDS[1 * 6 + 3] == "C/T" and align.PROFILE_FIELDS[5] == "A/gap"
    assert align.PROFILE_FIELDS[36] == "insertion_run_1" and align.PROFILE_FIELDS[51] == "insertion_run_16+"
    assert align.PROFILE_FIELDS[52] == "deletion_run_1" and align.PROFILE_FIELDS[67] == "deletion_run_16+"
    q, r = "ACGTTACGNAC", "ACCTACGGGAC"
    #       ACGTTACG--NAC
    #       ACCT-ACGGG-AC   written by hand: columns = X= I === DD I ==
    codes = np.array([0, 0, 1, 0, 2, 0, 0, 0, 3, 3, 2, 0, 0], dtype=np.uint8)
    row = [0, 0, 11, 0, 11, 8, 1, 2, 2]
    p = ref.profile(q, r, row, codes)
    assert p[:36].sum() == len(codes) and p[0] == 3 and p[2 * 6 + 1] == 1 and p[3 * 6 + 5] == 1 and p[4 * 6 + 5] == 1
    assert p[5 * 6 + 2] == 2 and p[36] == 2 and p[52 + 1] == 1 and p[35] == 0
    s = align.error_summary(np.stack([p, p]))
    assert s['substitutions'].shape == (4, 4) and s['substitutions'].trace() == 16 and s['substitutions'][2, 1] == 2
    assert s['insertions'].tolist() == [0, 0, 0, 2, 2] and s['deletions'].tolist() == [0, 0, 4, 0, 0]
    assert s['insertion_runs'][0] == 4 and s['deletion_runs'][1] == 2 and s['reference_letters'] == 22
    assert s['mismatch_rate'] == 2 / 22.0 and s['insertion_rate'] == 4 / 22.0 and s['deletion_rate'] == 4 / 22.0
    assert align.error_summary(np.zeros((0, 68)))['reference_letters'] == 0


def test_sam_record_parses_back_on_both_strands():
    from sloika_amd import align
    rs = np.random.RandomState(9)
    contig = align_cases.random_seq(rs, 400)
    for strand in '+-':
        read = "GATTACA" + align_cases.mutate(rs, contig[120:300]) + "TTT"
        if strand == '-':
            read = ref.revcomp(read)
        against = contig if strand == '+' else ref.revcomp(contig)
        row, codes = ref.ops(read, against)
        assert row[0] > 100 and row[7] and row[8] and row[6] and row[1] > 0 and row[2] < len(read)
        fwd = list(row)
        if strand == '-':
            fwd[3], fwd[4] = len(contig) - row[4], len(contig) - row[3]
        line = align.sam_record("read1", fwd, strand, codes, len(read), "chr", read)
        assert line.split("\t") == ref.sam_fields("read1", fwd, strand, codes, read, "chr")
        got = ref.parse_sam_line(line, contig)
        assert got["flag"] == (16 if strand == '-' else 0) and got["pos"] == fwd[3] + 1
        assert (got["M"], got["I"], got["D"], got["mismatch"]) == (row[5] + row[6], row[7], row[8], row[6])
        assert got["nm"] == got["tags"]["NM"] == row[6] + row[7] + row[8] and got["tags"]["AS"] == row[0]
        assert (got["r_start"], got["r_end"]) == (fwd[3], fwd[4])
        clips = (row[1], len(read) - row[2])
        assert (got["front"], got["back"]) == (clips if strand == '+' else clips[::-1])
        assert line.split("\t")[4] == "255"
        assert align.sam_record("read1", fwd, strand, codes, len(read), "chr").split("\t")[9] == "*"
    un = align.sam_record("r2", [0] * 9, '+', np.zeros(0, dtype=np.uint8), 4, "chr", "ACGT").split("\t")
    assert un[1] == "4" and un[2] == "*" and un[3] == "0" and un[5] == "*" and un[9] == "ACGT"
    text = align.sam_text([("chr", 400), ("chr2", 7)], [line, "\t".join(un)])
    lines = text.splitlines()
    assert lines[0].startswith("@HD\tVN:") and lines[1] == "@SQ\tSN:chr\tLN:400" and lines[2] == "@SQ\tSN:chr2\tLN:7"
    assert lines[3] == line and len(lines) == 5 and text.endswith("\n")


def test_traceback_runs_split_at_the_limit():
    from sloika_amd import align
    need = [100, 0, 50, 300, 20, 20]
    assert align._traceback_runs(need, None) == [(0, 6)]
    assert align._traceback_runs(need, 150) == [(0, 3), (3, 4), (4, 6)]
    assert align._traceback_runs(need, 10) == [(b, b + 1) for b in range(6)]     # a pair above the limit is a run of its own
    assert align._traceback_runs([], 10) == [(0, 0)]


@pytest.fixture(scope="module")
def L():
    from sloika_amd import build, _lib
    build.build()
    return _lib.lib()


def test_max_band_and_workspace_formula(L):
    W = L.slk_align_traceback_max_band()
    assert W >= 1024                                   # 8000 letters with 12 % planted errors: about 650 diagonals
    f = L.slk_align_traceback_workspace_bytes
    assert f(0, 0, 0, 0) == 16                         # one iteration, one diagonal rounded up to four dwords
    assert f(10, 10, 0, 0) == 2 * 16                   # 11 iterations: two blocks of eight
    n, m, I, D = 8000, 8010, 315, 325
    iters = ((n + m + D - (D & ~1)) >> 1) + 1
    assert f(n, m, I, D) == ((iters + 7) // 8) * ((I + D + 1 + 3) // 4 * 4) * 4
    assert f(n, m, I, D) <= (n + D + 8) * (I + D + 4) // 2 + 16      # 4 bits per band cell, never n' x m'
    assert f(n, m, I, D) % 16 == 0
    assert f(10, 10, 1, 0) == 0 and f(-1, 0, 0, 0) == 0 and f(10, 12, 0, 1) == 0 and f(70000, 70000, 0, 0) == 0
    assert f(2000, 2000, W - 1, W - 1) == 0 and f(2000, 1999, W // 2, W - 1 - W // 2) > 0 and f(2000, 1999, W // 2 + 1, W - W // 2) == 0


def test_entry_points_refuse_bad_arguments(L):
    from sloika_amd import _lib
    buf = (ctypes.c_uint8 * 256)()
    p = ctypes.addressof(buf) & ~15
    p = p if p == ctypes.addressof(buf) else p + 16
    tb = lambda args, B=1, scores=(1, 2, 2, 1): L.slk_align_traceback_batch_u8(
        args[0], 8, args[1], args[2], args[3], B, scores[0], scores[1], scores[2], scores[3], args[4], args[5], args[6], 8, args[7],
        args[8], 64, args[9], None)
    full = [p] * 10
    for k in range(10):                                # every pointer in turn
        args = list(full)
        args[k] = None
        assert tb(args) == _lib.SLK_ERR_INVALID_ARG, k
    assert tb(full, B=-1) == _lib.SLK_ERR_INVALID_ARG
    for scores in ((0, 2, 2, 1), (1, -1, 2, 1), (1, 2, -1, 1), (1, 2, 2, 0), (16385, 2, 2, 1), (1, 2, 2, 16385)):
        assert tb(full, scores=scores) == _lib.SLK_ERR_INVALID_ARG, scores
    args = list(full)
    args[7] = p + 4                                    # a workspace that is not 16-byte aligned
    assert tb(args) == _lib.SLK_ERR_WORKSPACE
    assert tb([None] * 10, B=0) == _lib.SLK_OK          # nothing to do: nothing is looked at
    pr = lambda args, B=1: L.slk_align_error_profile_u8(args[0], 8, args[1], args[2], args[3], args[4], args[5], args[6], B, args[7],
                                                        None)
    for k in range(8):
        args = [p] * 8
        args[k] = None
        assert pr(args) == _lib.SLK_ERR_INVALID_ARG, k
    assert pr([p] * 8, B=-1) == _lib.SLK_ERR_INVALID_ARG and pr([None] * 8, B=0) == _lib.SLK_OK
