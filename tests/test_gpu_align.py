"""Read accuracy on the device: csrc/align.hip through sloika_amd.align against the traceback oracle of tests/align_ref.py.
The nine integers per pair must be EQUAL: there is no tolerance.  The batch (tests/align_cases.py) takes its edge lengths from
align.PASS_WIDTH and is ragged, with a size that is no multiple of the waves per workgroup."""
import numpy as np
import pytest

from tests import align_cases, align_ref
from tests.gpu_util import need_gpu, dev

pytestmark = pytest.mark.gpu

SCORES2 = (3, 1, 5, 2)


@pytest.fixture(scope="module")
def cases():
    need_gpu()
    from sloika_amd import align
    P = align.PASS_WIDTH
    batch = align_cases.batch(P)
    assert len(batch) % 4 != 0
    want = np.array([align_ref.align(q, r) for _, q, r in batch], dtype=np.int32)
    return P, batch, want


def _compare(got, want, batch):
    bad = [(batch[b][0], got[b].tolist(), want[b].tolist()) for b in range(len(batch)) if not np.array_equal(got[b], want[b])]
    assert not bad, bad[:5]


def test_ragged_batch_equals_traceback_oracle(cases):
    from sloika_amd import align
    P, batch, want = cases
    got, strand = align.align_batch([q for _, q, _ in batch], [r for _, _, r in batch])
    assert got.dtype == np.int32 and got.shape == (len(batch), 9) and (strand == '+').all()
    _compare(got, want, batch)
    # the batch holds what it claims: both kinds of gap, alignments on both sides of and across the column between passes
    assert want[:, 7].sum() > 20 and want[:, 8].sum() > 20 and (want[:, 0] == 0).sum() >= 5
    assert ((want[:, 3] < P) & (want[:, 4] > P)).sum() >= 5 and (want[:, 3] >= P).any() and (want[:, 4] == P).any()


def test_single_pairs_and_input_kinds(cases):
    """One pair per launch (a workgroup with one live wave), given as bytes and as uint8 arrays; lower case is upper-cased."""
    from sloika_amd import align
    P, batch, want = cases
    for b in (0, len(batch) - 1, len(batch) // 2):
        _, q, r = batch[b]
        got, _ = align.align_batch([q.encode()], [np.frombuffer(r.encode(), dtype=np.uint8)])
        assert got[0].tolist() == want[b].tolist()
        got, _ = align.align_batch([q.lower()], [r])
        assert got[0].tolist() == want[b].tolist()
    got, strand = align.align_batch([], [])
    assert got.shape == (0, 9) and len(strand) == 0


def test_second_score_set(cases):
    from sloika_amd import align
    P, batch, _ = cases
    sub = batch[::3] + [c for c in batch if c[0].startswith(("del_", "ins_", "homo_", "dinuc_"))]
    want = np.array([align_ref.align(q, r, *SCORES2) for _, q, r in sub], dtype=np.int32)
    got, _ = align.align_batch([q for _, q, _ in sub], [r for _, _, r in sub], match=SCORES2[0], mismatch=SCORES2[1],
                               gap_open=SCORES2[2], gap_extend=SCORES2[3])
    _compare(got, want, sub)


def test_revcomp_against_numpy():
    need_gpu()
    import torch
    from sloika_amd import align
    rs = np.random.RandomState(3)
    lens = [0, 1, 2, 255, 256, 257, 5000, 0, 70000]
    seqs = [rs.randint(0, 256, size=n).astype(np.uint8) for n in lens]           # every byte value: only ACGT may change
    seqs[3][:8] = np.frombuffer(b"ACGTNacg", dtype=np.uint8)
    off = np.concatenate(([0], np.cumsum(lens))).astype(np.int64)
    table = np.arange(256, dtype=np.uint8)
    table[np.frombuffer(b"ACGT", dtype=np.uint8)] = np.frombuffer(b"TGCA", dtype=np.uint8)
    want = np.concatenate([table[s[::-1]] for s in seqs])
    got = align.revcomp_packed(dev(np.concatenate(seqs)), dev(off), max(lens))
    torch.cuda.synchronize()
    assert np.array_equal(got.cpu().numpy(), want)


def test_both_strands_finds_planted_reverse_complements():
    need_gpu()
    from sloika_amd import align
    P = align.PASS_WIDTH
    planted = align_cases.strand_batch(P)
    qs, rs_, strands = [p[0] for p in planted], [p[1] for p in planted], [p[2] for p in planted]
    got, strand = align.align_batch(qs, rs_, both_strands=True)
    assert strand.tolist() == strands
    for b, (q, r, s) in enumerate(planted):
        if s == '+':
            want = align_ref.align(q, r)
        else:                                        # the alignment against the reverse complement, in forward coordinates
            want = align_ref.align(q, align_cases.revcomp(r))
            want[3], want[4] = len(r) - want[4], len(r) - want[3]
        assert got[b].tolist() == want, b
        assert got[b, 0] >= max(align_ref.score_only(q, r), align_ref.score_only(q, align_cases.revcomp(r)))
    one, plus = align.align_batch(qs, rs_)
    assert (plus == '+').all() and (one[:, 0] <= got[:, 0]).all()


def test_accuracy_of_paths_equals_align_batch_on_the_called_strings():
    need_gpu()
    from sloika_amd import align, bio
    P = align.PASS_WIDTH
    klen, rs = 5, np.random.RandomState(8)
    nst = 4 ** klen
    lens = [0, 1, 40, 300, P + 30, 120, 77]
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
    for both in (False, True):
        res, strand, nbases = align.accuracy_of_paths(pd, ld, refs, klen, both_strands=both)
        want, wstrand = align.align_batch(called, refs, both_strands=both)
        assert np.array_equal(res, want) and strand.tolist() == wstrand.tolist()
        assert nbases.tolist() == [len(c) for c in called]
    assert strand[2] == '-'
    res, strand, nbases = align.accuracy_of_paths(pd, ld, refs, klen)
    assert [r.tolist() for r in res] == [align_ref.align(c, r) for c, r in zip(called, refs)]
    rows = align.samacc_rows(res, strand, nbases)
    assert 3 <= len(rows) <= 5 and all(0.7 < r['accuracy'] <= 1.0 for r in rows)


def test_long_pair_score_and_consistency():
    """About 3000 x 3100: six passes, 47 refills of lane 0's input.  Score against the score-only DP; the counts must add up to
    the spans they were derived with."""
    need_gpu()
    from sloika_amd import align
    rs = np.random.RandomState(12)
    ref = align_cases.random_seq(rs, 3100)
    q = align_cases.mutate(rs, ref[40:3060])
    assert 2900 < len(q) < 3100
    got, _ = align.align_batch([q, 'A' * 10], [ref, 'A' * 10])
    score, qs, qe, rs_, re, match, mism, ins, dele = got[0].tolist()
    assert score == align_ref.score_only(q, ref)
    assert qe - qs == match + mism + ins and re - rs_ == match + mism + dele
    assert min(match, mism, ins, dele) > 0 and 0 <= qs < qe <= len(q) and 0 <= rs_ < re <= len(ref)
    assert match > 0.85 * len(q)
    assert got[1].tolist() == [10, 0, 10, 0, 10, 10, 0, 0, 0]


def test_device_side_length_beyond_its_bound_is_refused_not_truncated():
    """The C entry trusts max_qlen / max_rlen for its workspace and limits; a pair whose device-side length exceeds them gets the
    row (-1, 0, ...) and Python raises."""
    torch = need_gpu()
    from sloika_amd import _lib, align
    q = dev(np.frombuffer(b"ACGTACGTAC", dtype=np.uint8).reshape(1, 10).copy())
    qlen = dev(np.array([10], dtype=np.int32))
    r = dev(np.frombuffer(b"ACGTACGTAC", dtype=np.uint8).copy())
    roff = dev(np.array([0, 10], dtype=np.int64))
    out = torch.zeros((1, 9), dtype=torch.int32, device=q.device)
    L = _lib.lib()
    for mq, mr in ((9, 10), (10, 9)):
        assert L.slk_align_local_batch_u8(q.data_ptr(), 10, qlen.data_ptr(), r.data_ptr(), roff.data_ptr(), 1, mq, mr, 1, 2, 2, 1,
                                          out.data_ptr(), None, 0, None) == 0
        torch.cuda.synchronize()
        assert out.cpu().numpy()[0].tolist() == [-1, 0, 0, 0, 0, 0, 0, 0, 0]
    with pytest.raises(ValueError):
        align._align_device(q, 10, qlen, 9, r, roff, np.array([10]), (1, 2, 2, 1), False)
