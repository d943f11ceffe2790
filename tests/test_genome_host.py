"""The host side of sloika_amd.genome and the model of tests/genome_ref.py, without a GPU: the model against hand-worked cases,
the window and get_refs arithmetic, FASTA text and its reader, and every refusal that is raised before anything is launched."""
import numpy as np
import pytest

from tests import align_cases, genome_ref

TINY = [("a", "ACGTACGTAC"), ("b", "ACG"), ("c", "nACGTACGTN")]


def test_codes_and_keys_by_hand():
    assert genome_ref.kmer_code("ACGTACGT") == 0x1B1B and genome_ref.kmer_code("AAAAAAAC") == 1
    assert genome_ref.kmer_code("T" * 15) == 4 ** 15 - 1 < genome_ref.INVALID
    assert genome_ref.kmer_code("ACGNACGT") is None
    keys, valid = genome_ref.genome_keys(TINY, 8)
    want = [genome_ref.INVALID] * 23
    want[0], want[1], want[2], want[14] = 0x1B1B, 0x6C6C, 0xB1B1, 0x1B1B      # a: the three k-mers that end inside it; c: the one between its Ns
    assert valid == 4 and keys.dtype == np.int64
    assert keys.tolist() == [(c << 32) | p for p, c in enumerate(want)]
    # sorted, invalid keys lie behind every real one and positions ascend within a code
    assert [k & 0xFFFFFFFF for k in sorted(keys.tolist())[:4]] == [0, 14, 1, 2]
    assert genome_ref.occurrences(TINY, 8) == {0x1B1B: [0, 14], 0x6C6C: [1], 0xB1B1: [2]}


def test_vote_by_hand():
    table = genome_ref.occurrences(TINY, 8)
    # ACGTACGT occurs at 0 and 14: diagonals 65536 and 65550, at width 4 the bins 16384, 16383 and 16387, 16386, one vote each
    assert genome_ref.vote(table, "ACGTACGT", 8, 4, 64) == (16383, 1, 1, 1)
    assert genome_ref.vote(table, "ACGTACGT", 8, 8, 64) == (8192, 2, 0, 1)            # bins 8192, 8191 and 8193, 8192: the two loci share one
    assert genome_ref.vote(table, "ACGTACGT", 8, 4, 2) == (16383, 1, 1, 1)            # exactly max_occ occurrences still vote
    assert genome_ref.vote(table, "ACGTACGT", 8, 4, 1) == (0, 0, 0, 0)                # one more than max_occ: skipped, not a seed
    assert genome_ref.vote(table, "ACGTACG", 8, 4, 64) == (0, 0, 0, 0)                # shorter than k
    assert genome_ref.vote(table, "TTTTTTTTTT", 8, 4, 64) == (0, 0, 0, 3)             # valid k-mers that occur nowhere are seeds without votes
    # position 2 of the query on genome position 1: diagonal 65535, bins 16383 and 16382
    assert genome_ref.vote(table, "NNCGTACGTA", 8, 4, 64) == (16382, 1, 0, 1)
    # the '-' strand is the vote of the reverse complement; ACGTACGT is its own
    assert genome_ref.revcomp("AACGTN") == "NACGTT"
    assert genome_ref.seed(table, "acgtacgt", 8, 4, 64) == [[16383, 1, 1, 1], [16383, 1, 1, 1]]
    assert genome_ref.seed(table, "GTACGTAC", 8, 4, 64)[0] == [16383, 1, 0, 1]
    assert genome_ref.seed(table, "GTACGTAC", 8, 4, 64)[1] == [16383, 1, 0, 1]        # its reverse complement GTACGTAC: itself


def test_vote_of_an_exact_copy():
    rs = np.random.RandomState(5)
    contigs = [("x", align_cases.random_seq(rs, 400)), ("y", align_cases.random_seq(rs, 300))]
    table = genome_ref.occurrences(contigs, 8)
    q = contigs[1][1][100:160]                                    # packed position 500: diagonal 66036 = 4127 * 16 + 4
    rows = genome_ref.seed(table, q, 8, 16, 64)
    assert rows[0][0] == 4126 and rows[0][1] >= 53 and rows[0][3] == 53 and rows[0][2] < 5      # bins 4126 and 4127 tie: the smaller
    assert rows[1][1] < 5
    assert genome_ref.choose_strand(rows, 3) == ('+', rows[0])
    back = genome_ref.seed(table, genome_ref.revcomp(q), 8, 16, 64)
    assert back == [rows[1], rows[0]] and genome_ref.choose_strand(back, 3)[0] == '-'
    assert genome_ref.choose_strand([[7, 2, 0, 9], [9, 2, 0, 9]], 3) is None
    assert genome_ref.choose_strand([[7, 3, 0, 9], [9, 3, 0, 9]], 3) == ('+', [7, 3, 0, 9])      # a tie goes to '+'
    # the window: slack = 16 + ceil(60 / 16) = 20; [4126 * 16 - 65536 - 20, 4128 * 16 - 65536 + 60 + 20), inside contig y
    assert genome_ref.window(4126, 60, 16, 1.0 / 16, [0, 400, 700]) == (460, 592, 1)
    assert genome_ref.window(4126, 60, 16, 0.0, [0, 400, 700]) == (464, 588, 1)
    assert genome_ref.window(4126, 60, 16, 1.0 / 16, [0, 400, 520]) == (460, 520, 1)             # clipped to its contig's end
    assert genome_ref.window(4126, 60, 16, 1.0 / 16, [0, 500, 700]) == (500, 592, 1)             # ... and start
    assert genome_ref.window(4090, 60, 16, 1.0 / 16, [0, 400, 700]) == (0, 16, 0)                # overhangs the genome's start


def test_window_of_and_runs_agree_with_the_model():
    from sloika_amd import genome
    for b, n, w, drift in ((4126, 60, 16, 1.0 / 16), (300, 8000, 256, 1.0 / 16), (257, 1, 64, 0.0), (1000, 999, 256, 0.3)):
        lo, hi = genome.window_of(b, n, w, drift)
        assert (max(lo, -10 ** 9), min(hi, 10 ** 9), 0) == genome_ref.window(b, n, w, drift, [-10 ** 9, 10 ** 9])
    assert genome.align_runs([100, 100, 100], [600, 600, 600], None) == [(0, 3)]


def test_reference_span_arithmetic():
    from sloika_amd import genome
    row = [70, 5, 90, 200, 290, 80, 3, 2, 7]
    # '+': 5 letters in front of the alignment, 10 behind it
    assert genome.reference_span(row, '+', 100, 1000, pad=50) == (145, 350)
    # '-': the record holds the reverse complement, whose first 10 letters and last 5 are unaligned
    assert genome.reference_span(row, '-', 100, 1000, pad=50) == (140, 345)
    assert genome.reference_span(row, '+', 100, 1000, pad=0) == (195, 300)
    assert genome.reference_span(row, '-', 100, 1000, pad=0) == (190, 295)
    assert genome.reference_span([70, 5, 90, 20, 110, 80, 3, 2, 7], '+', 100, 1000, pad=50) == (0, 170)        # the contig's start
    assert genome.reference_span([70, 5, 90, 900, 990, 80, 3, 2, 7], '-', 100, 1000, pad=50) == (840, 1000)    # ... and end
    for r in (row, [70, 5, 90, 20, 110, 80, 3, 2, 7], [70, 0, 100, 900, 1000, 80, 3, 2, 7]):
        for s in '+-':
            for pad in (0, 50):
                assert genome.reference_span(r, s, 100, 1000, pad=pad) == genome_ref.reference_span(r[1], r[2], r[3], r[4], s, 100, 1000, pad)
    contig = align_cases.random_seq(np.random.RandomState(2), 1000)
    assert genome_ref.read_reference(contig, 5, 90, 200, 290, '+', 100, 50) == contig[145:350]
    assert genome_ref.read_reference(contig, 5, 90, 200, 290, '-', 100, 50) == align_cases.revcomp(contig[140:345])


def test_reference_spans_filter_and_offsets():
    from sloika_amd import genome
    lengths, offsets = np.array([1000, 500]), np.array([0, 1000, 1500])
    res = np.array([[70, 5, 90, 200, 290, 80, 3, 2, 7],           # coverage 0.85
                    [0, 0, 0, 0, 0, 0, 0, 0, 0],                  # unmapped
                    [40, 10, 69, 100, 160, 55, 2, 2, 3],          # coverage 0.59: under the bound
                    [40, 10, 70, 100, 160, 56, 2, 2, 2],          # coverage 0.60: kept
                    [70, 5, 90, 200, 290, 80, 3, 2, 7]], dtype=np.int32)
    strand = np.array(['+', '+', '+', '-', '-'])
    contig = np.array([0, -1, 1, 1, 0], dtype=np.int32)
    keep, start, end = genome.reference_spans(lengths, offsets, res, strand, contig, [100] * 5, min_coverage=0.6, pad=50)
    assert keep == [0, 3, 4]
    assert (start[0], end[0]) == (145, 350) and (start[2], end[2]) == (140, 345)
    assert (start[1], end[1]) == (1000 + 100 - 30 - 50, 1000 + 160 + 10 + 50)
    keep, _, _ = genome.reference_spans(lengths, offsets, res, strand, contig, [100] * 5, min_coverage=0.0, pad=50)
    assert keep == [0, 2, 3, 4]
    keep, _, _ = genome.reference_spans(lengths, offsets, res, strand, contig, [100, 100, 100, 100, 0], min_coverage=0.9, pad=0)
    assert keep == []


def test_fasta_text_and_reader(tmp_path):
    from sloika_amd import genome, util
    records = [("chr1", "ACGTTGCA" * 20), ("two", "acgtnACGT"), ("three", "GGGTTTAAACCC")]
    assert genome.fasta([("r", "ACGT"), ("s", b"TT")]) == ">r\nACGT\n>s\nTT\n"
    path = tmp_path / "g.fa"
    path.write_text(genome.fasta(records))
    assert util.fasta_records(str(path)) == records
    # wrapped lines, a description behind the id, blank lines, a record without letters
    path.write_text(";comment\n>chr1 first contig\n" + "\n".join(records[0][1][j:j + 60] for j in range(0, 160, 60))
                    + "\n\n>two\nacgtn\nACGT\n>empty\n>three\tx\nGGGTTTAAACCC")
    got = util.fasta_records(str(path))
    assert got == records[:2] + [("empty", "")] + records[2:]
    # the reference's loader leaves out records with an N (of that case) and empty ones, and gives bytes
    assert util.fasta_file_to_dict(str(path)) == {"chr1": records[0][1].encode(), "two": b"acgtnACGT", "three": b"GGGTTTAAACCC"}
    path.write_text(">two\nACGTNACGT\n>three\nGG\n")
    assert util.fasta_file_to_dict(str(path)) == {"three": b"GG"}
    assert genome.trim_fast5_extension("read7.fast5") == "read7" and genome.trim_fast5_extension("read7.txt") == "read7.txt"


def test_refusals_before_any_launch():
    from sloika_amd import genome
    good = [("c", "ACGT" * 10)]
    for kw in (dict(k=7), dict(k=16), dict(k=10.5), dict(bin_width=100), dict(bin_width=0), dict(bin_width=1), dict(bin_width=65536),
               dict(max_occ=0), dict(max_occ=5000)):
        with pytest.raises(ValueError, match="genome: (k|bin_width|max_occ) ="):
            genome.Index(good, **kw)
    with pytest.raises(ValueError, match="empty"):
        genome.Index([])
    with pytest.raises(ValueError, match="empty"):
        genome.Index({"a": "", "b": b""})
    half = np.zeros(1 << 30, dtype=np.uint8)                       # (never touched: the length alone is refused)
    with pytest.raises(ValueError, match="2\\^31"):
        genome.Index([("a", half), ("b", half)])
    with pytest.raises(ValueError):
        genome.Index([("a", np.zeros(4, dtype=np.int32))])          # a sequence is a str, bytes or uint8
