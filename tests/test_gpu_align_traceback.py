"""The alignments' columns on the device: csrc/align_traceback.hip through sloika_amd.align / genome against the column oracle
of tests/align_ops_ref.py.  Every comparison is an integer equality.  Pairs are a few hundred letters (the oracle is plain loops)
except one of 1500 x 1500."""
import numpy as np
import pytest

from tests import align_cases, align_ops_cases as cases, align_ops_ref as ref, align_ref
from tests.gpu_util import need_gpu, dev

pytestmark = pytest.mark.gpu

DEFAULT = (1, 2, 2, 1)


def _kw(scores):
    return dict(match=scores[0], mismatch=scores[1], gap_open=scores[2], gap_extend=scores[3])


def _check(pairs, scores, res, ops, want=None, profile=True):
    """Rows, columns, CIGAR and profile of a batch against the oracle's; -> the oracle's (row, codes) list."""
    want = want or [ref.ops(q, r, *scores) for q, r in pairs]
    assert len(ops) == len(pairs) and ops.status.dtype == np.int32
    bad = []
    for b, ((q, r), (row, codes)) in enumerate(zip(pairs, want)):
        assert res[b].tolist() == row, b
        assert ops.status[b] == (0 if row[0] > 0 else 1), (b, ops.status[b])
        got = ops.codes(b)
        assert got.dtype == np.uint8
        if not np.array_equal(got, codes):
            bad.append((b, len(q), len(r), row))
    assert not bad, bad[:5]
    assert ops.offsets.tolist() == np.concatenate(([0], np.cumsum([len(c) for _, c in want]))).tolist()
    if profile:
        prof = ops.profile()
        assert prof.dtype == np.int32 and prof.shape == (len(pairs), 68)
        for b, ((q, r), (row, codes)) in enumerate(zip(pairs, want)):
            assert prof[b].tolist() == ref.profile(q, r, row, codes).tolist(), b
            assert prof[b, :36].sum() == len(codes) and prof[b, 35] == 0
    return want


@pytest.fixture(scope="module")
def ragged():
    need_gpu()
    from sloika_amd import align
    pairs = [(q, r) for _, q, r in align_cases.batch(align.PASS_WIDTH)]
    return pairs, [ref.ops(q, r) for q, r in pairs]


def test_ragged_batch_equals_the_column_oracle(ragged):
    from sloika_amd import align
    pairs, want = ragged
    res, strand, ops = align.align_batch([q for q, _ in pairs], [r for _, r in pairs], ops=True)
    _check(pairs, DEFAULT, res, ops, want)
    rows = np.array([w[0] for w in want])
    assert (rows[:, 0] == 0).sum() >= 5 and rows[:, 7].sum() > 20 and rows[:, 8].sum() > 20
    assert {len(q) for q, _ in pairs} >= {0, 1, 2, 63, 64, 65, 203}
    for b in (0, len(pairs) // 2, len(pairs) - 1):
        assert ops.cigar(b) == (ref.cigar(want[b][1]) if rows[b, 0] > 0 else "*")
        if rows[b, 0] > 0:
            n = len(pairs[b][0])
            assert ops.cigar(b, extended=False, clip=n) == ref.cigar(want[b][1], False, rows[b, 1], n - rows[b, 2])
            assert ops.cigar(b, False, n, reverse=True) == ref.cigar(want[b][1][::-1], False, n - rows[b, 2], rows[b, 1])
    prof = ops.profile()
    assert np.trace(prof[:, :36].sum(axis=0).reshape(6, 6)[:4, :4]) == rows[:, 5].sum()       # only A C G T occur here


def test_both_strands_columns_index_the_chosen_buffer():
    need_gpu()
    from sloika_amd import align
    planted = align_cases.strand_batch(align.PASS_WIDTH)
    qs, rs_, strands = [p[0] for p in planted], [p[1] for p in planted], [p[2] for p in planted]
    res, strand, ops = align.align_batch(qs, rs_, both_strands=True, ops=True)
    assert strand.tolist() == strands and '-' in strands and '+' in strands
    prof = ops.profile()
    for b, (q, r, s) in enumerate(planted):
        against = r if s == '+' else align_cases.revcomp(r)
        row, codes = ref.ops(q, against)
        assert ops.rows[b].tolist() == row                               # the coordinates of the buffer the columns index
        fwd = list(row)
        if s == '-':
            fwd[3], fwd[4] = len(r) - row[4], len(r) - row[3]
        assert res[b].tolist() == fwd and ops.status[b] == 0
        assert np.array_equal(ops.codes(b), codes), b
        assert prof[b].tolist() == ref.profile(q, against, row, codes).tolist(), b
    # SAM records, parsed back over the forward reference
    names = ["read%d" % b for b in range(len(qs))]
    lines = align.sam_records(res, strand, ops, names, ["ref%d" % b for b in range(len(qs))], [len(r) for r in rs_], queries=qs)
    for b, line in enumerate(lines):
        got = ref.parse_sam_line(line, rs_[b])
        assert got["flag"] == (16 if strands[b] == '-' else 0) and line.split("\t")[2] == "ref%d" % b
        assert (got["r_start"], got["r_end"]) == (res[b, 3], res[b, 4])
        assert (got["M"], got["I"], got["D"], got["mismatch"]) == (res[b, 5] + res[b, 6], res[b, 7], res[b, 8], res[b, 6])
        assert got["nm"] == got["tags"]["NM"] and got["tags"]["AS"] == res[b, 0]
    assert align.sam_records(res, strand, ops, names, names, [len(r) for r in rs_])[0].split("\t")[9] == "*"
    assert ops.queries() == [q.encode() for q in qs]
    same = align.align_batch(qs, rs_, both_strands=True)
    assert len(same) == 2 and np.array_equal(same[0], res) and same[1].tolist() == strand.tolist()


@pytest.mark.parametrize("W", cases.WIDTHS)
def test_planted_band_widths(W):
    need_gpu()
    from sloika_amd import align
    pairs = [cases.width_pair(W), ("ACGT" * 5, "ACGT" * 5)]
    res, _, ops = align.align_batch([q for q, _ in pairs], [r for _, r in pairs], ops=True)
    want = _check(pairs, DEFAULT, res, ops)
    assert want[0][0][7] + want[0][0][8] + 1 == W


@pytest.mark.parametrize("W", cases.WIDE_WIDTHS)
def test_wide_bands_on_both_sides_of_the_layout_switches(W):
    """W = 256 runs four diagonals per lane, 257 eight, 513 twelve, 769 sixteen; 1024 is the widest band.  Gap-cheap scores keep
    the pairs short; the runs are 'N' / 'K' letters, which the profile files under class 4."""
    need_gpu()
    from sloika_amd import _lib, align
    assert _lib.lib().slk_align_traceback_max_band() == 1024
    pairs = [cases.wide_pair(W), ("ACGT" * 5, "ACGT" * 5)]
    res, _, ops = align.align_batch([q for q, _ in pairs], [r for _, r in pairs], ops=True, **_kw(cases.WIDE_SCORES))
    want = _check(pairs, cases.WIDE_SCORES, res, ops)
    row, codes = want[0]
    assert row[7] + row[8] + 1 == W and ref.diagonal_range(codes)[1] > W // 3
    prof = ops.profile()[0].reshape(-1)
    assert prof[4 * 6 + 5] == row[7] and prof[5 * 6 + 4] == row[8] and prof[36 + 15] > 0 and prof[52 + 15] > 0


def test_band_wider_than_the_kernel_accepts_is_refused_by_name():
    need_gpu()
    from sloika_amd import align
    q, r = cases.wide_pair(1025)
    res, _, ops = align.align_batch([q, "ACGTACGT"], [r, "ACGTACGT"], ops=True, **_kw(cases.WIDE_SCORES))
    assert res[0, 7] + res[0, 8] + 1 == 1025 and ops.status.tolist() == [-4, 0]
    with pytest.raises(ValueError, match="pair 0.*widest band"):
        ops.codes(0)
    with pytest.raises(ValueError, match="pair 0"):
        ops.profile()
    assert ops.cigar(1) == "8="


def test_paths_that_touch_the_edges_of_their_band():
    need_gpu()
    from sloika_amd import align
    pairs = list(cases.edge_pairs())
    res, _, ops = align.align_batch([q for q, _ in pairs], [r for _, r in pairs], ops=True)
    want = _check(pairs, DEFAULT, res, ops)
    assert ref.diagonal_range(want[0][1])[1] == want[0][0][7] > 3 and ref.diagonal_range(want[1][1])[0] == -want[1][0][8] < -3


@pytest.mark.parametrize("scores", cases.TIE_SCORES)
def test_two_letter_pairs_where_ties_decide_the_path(scores):
    need_gpu()
    from sloika_amd import align
    pairs = cases.tie_pairs()
    res, _, ops = align.align_batch([q for q, _ in pairs], [r for _, r in pairs], ops=True, **_kw(scores))
    want = _check(pairs, scores, res, ops)
    assert sum(1 for row, _ in want if row[0] > 0) >= 0.9 * len(pairs)


def test_long_pair_with_the_inter_pass_workspace():
    """1500 x 1500: the forward pass walks three passes.  The score against the score-only DP, the columns against the oracle on
    the aligned rectangle alone (anchored there, the oracle finds the same alignment: every prefix of it scores above 0)."""
    need_gpu()
    from sloika_amd import align
    rs = np.random.RandomState(31)
    r = align_cases.random_seq(rs, 1500)
    q = (align_cases.mutate(rs, r) + align_cases.random_seq(rs, 200))[:1500]
    assert len(q) == 1500 and len(r) > 2 * align.PASS_WIDTH
    res, _, ops = align.align_batch([q], [r], ops=True)
    row = res[0].tolist()
    assert row[0] == align_ref.score_only(q, r) and ops.status[0] == 0 and row[7] + row[8] + 1 > 64
    sub_row, codes = ref.ops(q[row[1]:row[2]], r[row[3]:row[4]])
    assert sub_row == [row[0], 0, row[2] - row[1], 0, row[4] - row[3]] + row[5:]
    assert np.array_equal(ops.codes(0), codes)
    assert ops.profile()[0].tolist() == ref.profile(q, r, row, codes).tolist()


def test_same_bits_alone_reversed_and_in_split_launches(ragged):
    from sloika_amd import align
    pairs, want = ragged
    pairs, want = pairs[::2] + list(cases.edge_pairs()), want[::2] + [ref.ops(q, r) for q, r in cases.edge_pairs()]
    qs, rs_ = [q for q, _ in pairs], [r for _, r in pairs]
    _, _, whole = align.align_batch(qs, rs_, ops=True)
    _check(pairs, DEFAULT, whole.rows, whole, want, profile=False)
    from sloika_amd import _lib
    per = [_lib.lib().slk_align_traceback_workspace_bytes(row[2] - row[1], row[4] - row[3], row[7], row[8]) if row[0] > 0 else 0
           for row, _ in want]
    limit = sum(per) // 4
    assert len(align._traceback_runs(per, limit)) >= 3 and whole.workspace_bytes == sum(per)        # three launches or more
    _, _, split = align.align_batch(qs, rs_, ops=True, workspace_limit=limit)
    _, _, rev = align.align_batch(qs[::-1], rs_[::-1], ops=True)
    B = len(pairs)
    for b in range(B):
        assert np.array_equal(split.codes(b), want[b][1]) and np.array_equal(rev.codes(B - 1 - b), want[b][1]), b
    assert split.status.tolist() == whole.status.tolist() == rev.status[::-1].tolist()
    for b in (3, B - 1):
        _, _, alone = align.align_batch([qs[b]], [rs_[b]], ops=True)
        assert np.array_equal(alone.codes(0), want[b][1]) and alone.status[0] == whole.status[b]


# ---- the C entry itself: canaries around every slice, doctored rows ------------------------------------------------------------

CANARY = 0xA5
STATUS_CANARY = 0x5A5A5A5A


class Raw(object):
    """One batch driven through the C ABI in one launch, with 64 canary bytes before and after ops and the workspace and a canary
    word on either side of status.  The LAST pair is the one the tests doctor: a workspace slice that is one byte short then
    moves no other pair's offset."""

    def __init__(self, pairs, scores=DEFAULT):
        torch = need_gpu()
        from sloika_amd import _lib, align
        self.torch, self.L, self.scores, self.pairs = torch, _lib.lib(), scores, pairs
        qs, rs_ = [q for q, _ in pairs], [r for _, r in pairs]
        self.rows, _ = align.align_batch(qs, rs_, **_kw(scores))
        B = self.B = len(pairs)
        self.ldq = max(max(len(q) for q in qs), 1)
        qh = np.zeros((B, self.ldq), dtype=np.uint8)
        for b, q in enumerate(qs):
            qh[b, :len(q)] = np.frombuffer(q.encode(), dtype=np.uint8)
        self.q, self.qlen = dev(qh), dev(np.array([len(q) for q in qs], dtype=np.int32))
        self.r = dev(np.frombuffer("".join(rs_).encode() + b"\0" * 8, dtype=np.uint8).copy())
        self.roff = dev(np.concatenate(([0], np.cumsum([len(r) for r in rs_]))).astype(np.int64))
        self.ncol = np.where(self.rows[:, 0] > 0, self.rows[:, 5:9].sum(axis=1), 0).astype(np.int64)
        self.need = np.array([self.L.slk_align_traceback_workspace_bytes(int(w[2] - w[1]), int(w[4] - w[3]), int(w[7]), int(w[8]))
                              if w[0] > 0 else 0 for w in self.rows], dtype=np.int64)
        assert (self.need % 16 == 0).all()

    def run(self, rows=None, ws_short=0, ops_extra=0):
        """rows: the rows the kernel is given; ws_short / ops_extra: bytes taken from the last pair's workspace slice / added to
        its ops slice.  -> (status with its canaries, ops bytes, ops offsets, workspace bytes, workspace offsets)."""
        torch = self.torch
        rows = self.rows if rows is None else rows
        ncol, need = self.ncol.copy(), self.need.copy()
        ncol[-1] += ops_extra
        need[-1] -= ws_short
        ooff = 64 + np.concatenate(([0], np.cumsum(ncol))).astype(np.int64)
        woff = 64 + np.concatenate(([0], np.cumsum(need))).astype(np.int64)
        ops = torch.full((int(ooff[-1]) + 64,), CANARY, dtype=torch.uint8, device=self.q.device)
        ws = torch.full((int(woff[-1]) + 64,), CANARY, dtype=torch.uint8, device=self.q.device)
        status = torch.full((self.B + 2,), STATUS_CANARY, dtype=torch.int32, device=self.q.device)
        rows_d, ooff_d, woff_d = dev(np.ascontiguousarray(rows, dtype=np.int32)), dev(ooff), dev(woff)
        rc = self.L.slk_align_traceback_batch_u8(self.q.data_ptr(), self.ldq, self.qlen.data_ptr(), self.r.data_ptr(),
                                                 self.roff.data_ptr(), self.B, *self.scores, rows_d.data_ptr(), ops.data_ptr(),
                                                 ooff_d.data_ptr(), ops.numel(), ws.data_ptr(), woff_d.data_ptr(), ws.numel(),
                                                 status[1:].data_ptr(), None)
        assert rc == 0
        torch.cuda.synchronize()
        return status.cpu().numpy(), ops.cpu().numpy(), ooff, ws.cpu().numpy(), woff


def _canaries_intact(status, ops, ooff, ws, woff, untouched=()):
    assert status[0] == STATUS_CANARY and status[-1] == STATUS_CANARY
    assert (ops[:64] == CANARY).all() and (ops[ooff[-1]:] == CANARY).all() and len(ops) == ooff[-1] + 64
    assert (ws[:64] == CANARY).all() and (ws[woff[-1]:] == CANARY).all() and len(ws) == woff[-1] + 64
    for b in untouched:
        assert (ops[ooff[b]:ooff[b + 1]] == CANARY).all() and (ws[woff[b]:woff[b + 1]] == CANARY).all(), b


@pytest.fixture(scope="module")
def raw():
    long_one = align_cases.random_seq(np.random.RandomState(4), 1200)
    pairs = [cases.edge_pairs()[0], ("AAAA", "CCCCCC"), ("", "ACGT"), ("ACGT", ""), ("ACGTACGTAC", "ACGTACGTAC"),
             (long_one, long_one), cases.width_pair(63)]
    return Raw(pairs)


def test_canaries_and_empty_alignments(raw):
    """An empty alignment, a query of no letters and a reference of no letters: status 1 and not a byte."""
    status, ops, ooff, ws, woff = raw.run()
    assert status[1:-1].tolist() == [0, 1, 1, 1, 0, 0, 0]
    _canaries_intact(status, ops, ooff, ws, woff, untouched=(1, 2, 3))
    assert ooff[1] == ooff[2] == ooff[3] == ooff[4] and woff[1] == woff[4]
    for b in (0, 4, 6):
        row, codes = ref.ops(*raw.pairs[b])
        assert raw.rows[b].tolist() == row and np.array_equal(ops[ooff[b]:ooff[b + 1]], codes), b
    assert (ops[ooff[5]:ooff[6]] == 0).all() and ooff[6] - ooff[5] == 1200


@pytest.mark.parametrize("what,code", [("span_past_qlen", -1), ("span_past_rlen", -1), ("negative_count", -2),
                                       ("counts_do_not_add_up", -3), ("band_above_max_band", -4), ("workspace_one_byte_short", -5),
                                       ("ops_slice_one_byte_long", -6), ("score_of_another_pair", -7)])
def test_doctored_rows_are_refused_and_nothing_is_touched(raw, what, code):
    """Inconsistent DATA, which the kernel must reject: for every case but the last the refusal is a comparison of the row with
    qlen / roff / ws_off / ops_off at the top of align_traceback_kernel, before anything of the pair is read or written.  The
    last is found after the fill (the band's DP ends on another value): the pair's workspace is used, its ops are not."""
    rows = raw.rows.copy()
    b = raw.B - 1
    n, m = len(raw.pairs[b][0]), len(raw.pairs[b][1])
    kw = {}
    if what == "span_past_qlen":
        rows[b, 1], rows[b, 2] = rows[b, 1] + n, rows[b, 2] + n
    elif what == "span_past_rlen":                                       # (the sums still hold: only the span check can refuse it)
        rows[b, 3], rows[b, 4] = 0, m + 1
        rows[b, 5:9] = [rows[b, 2] - rows[b, 1], 0, 0, m + 1 - (rows[b, 2] - rows[b, 1])]
    elif what == "negative_count":
        rows[b, 5], rows[b, 6] = rows[b, 5] + rows[b, 6] + 2, -2
    elif what == "counts_do_not_add_up":
        rows[b, 7] += 1
    elif what == "band_above_max_band":                                  # consistent in itself, inside both sequences, W = 1101
        b = 5
        rows[b] = [50, 0, 600, 0, 600, 50, 0, 550, 550]
    elif what == "workspace_one_byte_short":
        kw = dict(ws_short=1)
    elif what == "ops_slice_one_byte_long":
        kw = dict(ops_extra=1)
    else:
        rows[b, 0] += 1
    status, ops, ooff, ws, woff = raw.run(rows, **kw)
    assert status[1 + b] == code
    others = [k for k in range(raw.B) if k != b]
    assert status[1:-1][others].tolist() == [[0, 1, 1, 1, 0, 0, 0][k] for k in others]
    _canaries_intact(status, ops, ooff, ws, woff, untouched=(1, 2, 3))
    assert (ops[ooff[b]:ooff[b + 1]] == CANARY).all()
    if code != -7:
        assert (ws[woff[b]:woff[b + 1]] == CANARY).all()
    row, codes = ref.ops(*raw.pairs[0])
    assert np.array_equal(ops[ooff[0]:ooff[1]], codes)


# ---- through the other public entries -------------------------------------------------------------------------------------------

def test_accuracy_of_paths_columns_decode_against_the_called_bases():
    need_gpu()
    from sloika_amd import align, bio
    klen, rs = 5, np.random.RandomState(8)
    nst = 4 ** klen
    lens = [0, 1, 40, 300, 120, 77]
    paths = np.zeros((len(lens), max(lens) + 2), dtype=np.int32)
    for b, n in enumerate(lens):
        s = rs.randint(0, nst)
        for t in range(n):
            s = (s * 4) % nst + rs.randint(0, 4) if rs.uniform() < 0.9 else rs.randint(0, nst)
            paths[b, t] = s
    pd, ld = dev(paths), dev(np.asarray(lens, dtype=np.int32))
    called = bio.paths_to_bases(pd, ld, klen, "ACGT", always_move=True)
    refs = [align_cases.mutate(rs, c) if c else "ACGT" for c in called]
    refs[2] = align_cases.revcomp(refs[2])
    res, strand, nbases, ops = align.accuracy_of_paths(pd, ld, refs, klen, both_strands=True, ops=True)
    plain = align.accuracy_of_paths(pd, ld, refs, klen, both_strands=True)
    assert len(plain) == 3 and np.array_equal(plain[0], res) and plain[1].tolist() == strand.tolist()
    assert np.array_equal(plain[2], nbases) and strand[2] == '-' and nbases.tolist() == [len(c) for c in called]
    for b, c in enumerate(called):
        against = refs[b] if strand[b] == '+' else align_cases.revcomp(refs[b])
        row, codes = ref.ops(c, against)
        assert ops.rows[b].tolist() == row and np.array_equal(ops.codes(b), codes), b
    assert [x.decode() for x in ops.queries()] == list(called)
    _, _, _, split = align.accuracy_of_paths(pd, ld, refs, klen, both_strands=True, ops=True, workspace_limit=1)
    assert all(np.array_equal(split.codes(b), ops.codes(b)) for b in range(len(lens)))


def test_index_map_columns_and_sam_records():
    need_gpu()
    from sloika_amd import align, genome
    rs = np.random.RandomState(40)
    contigs = [("c%d" % k, align_cases.random_seq(rs, n)) for k, n in enumerate((900, 1500, 700))]
    idx = genome.Index(contigs, k=11, bin_width=64)
    reads, truth = [], []
    for k, (c, lo, hi, minus) in enumerate(((0, 100, 400, False), (1, 900, 1300, True), (2, 50, 350, False), (1, 100, 420, True),
                                           (0, 500, 880, False))):
        read = "GGATC" + align_cases.mutate(rs, contigs[c][1][lo:hi]) + "CA"
        reads.append(align_cases.revcomp(read) if minus else read)
        truth.append((c, '-' if minus else '+'))
    reads.append(align_cases.random_seq(rs, 150))                        # lies nowhere
    names = ["read%d" % k for k in range(len(reads))]
    res, strand, info, ops = idx.map(reads, ops=True)
    plain = idx.map(reads)
    assert len(plain) == 3 and np.array_equal(plain[0], res) and plain[1].tolist() == strand.tolist()
    assert info['contig'].tolist() == [c for c, _ in truth] + [-1] and strand.tolist() == [s for _, s in truth] + ['+']
    assert ops.status.tolist() == [0] * 5 + [1]
    lines = genome.sam_records(idx, res, strand, info, ops, names, queries=reads)
    for b, (c, s) in enumerate(truth):
        got = ref.parse_sam_line(lines[b], contigs[c][1])
        assert lines[b].split("\t")[2] == "c%d" % c and got["flag"] == (16 if s == '-' else 0)
        assert (got["r_start"], got["r_end"]) == (res[b, 3], res[b, 4])
        assert (got["M"], got["I"], got["D"], got["mismatch"]) == (res[b, 5] + res[b, 6], res[b, 7], res[b, 8], res[b, 6])
        assert got["nm"] == got["tags"]["NM"] and got["tags"]["AS"] == res[b, 0]
        n = len(reads[b])
        clips = (res[b, 1], n - res[b, 2])
        assert (got["front"], got["back"]) == (clips if s == '+' else clips[::-1])
    assert lines[5].split("\t")[1:6] == ["4", "*", "0", "0", "*"]
    text = align.sam_text(zip(idx.names, idx.lengths), lines)
    assert text.count("@SQ") == 3 and text.splitlines()[1] == "@SQ\tSN:c0\tLN:900"
    split = idx.map(reads, ops=True, workspace_limit=1)
    assert all(np.array_equal(split[3].codes(b), ops.codes(b)) for b in range(len(reads)))
    prof = ops.profile()
    assert prof[:, :36].sum(axis=1).tolist() == [int(res[b, 5:9].sum()) for b in range(len(reads))]


def test_defaults_return_what_they_returned():
    need_gpu()
    from sloika_amd import align
    got = align.align_batch(["ACGTACGT", ""], ["ACGTTCGT", "AC"])
    assert len(got) == 2 and got[0].dtype == np.int32 and got[0].shape == (2, 9) and got[1].dtype.kind == 'U'
    assert got[0][0].tolist() == align_ref.align("ACGTACGT", "ACGTTCGT") and got[0][1].tolist() == [0] * 9
    empty = align.align_batch([], [], ops=True)
    assert len(empty) == 3 and len(empty[2]) == 0 and empty[2].profile().shape == (0, 68)
    assert len(align.align_batch([], [])) == 2
