"""The rescoring identity of design/rescore_edits.md on the CPU: tests/rescore_ref.py (the stored lattices and the cut sum, plain float64
loops) against the forward score of the spelled-out sequence (tests/forward_ref.py), bio.edit_states, and the planted polish case.

E_ref = 3.219e-15 is design/forward_score.md 5: the reference recursion's own distance from the exact value.  E_cut, the model's
largest distance from the extended-precision value over rescore_ref.wide_cases, is 1.6e-16 (0.05 E_ref)."""
import math

import numpy as np
import pytest

from tests import forward_ref as fr
from tests import rescore_ref as rr

E_REF = 3.219e-15


def test_identity_tiny():
    """Every (a, d) and m in {0, 1, 2, 8} on T in {1, 2, 3, 5, 9}, L in {0, 1, 2, 4}: the cut sum is the forward score of the
    spelled-out sequence within 4 E_ref, and -inf in exactly the same cases."""
    n = ninf = 0
    for post, seq, edits in rr.tiny_cases():
        score, ll = rr.rescore(post, seq, edits)
        want = fr.forwards(post, seq, full=True)
        assert score == want or abs(score - want) <= 4 * E_REF * max(1.0, abs(want))
        for e, got in zip(edits, ll):
            want = float(fr.forwards(post, np.array(rr.spell(seq, e), dtype=np.int64), full=True))
            n += 1
            if math.isinf(want):
                ninf += 1
                assert got == want, (post.shape, list(seq), e)
                assert len(seq) - e[1] + len(e[2]) > post.shape[0]
            else:
                assert abs(got - want) <= 4 * E_REF * max(1.0, abs(want)), (post.shape, list(seq), e, got, want)
    assert n >= 500 and 0 < ninf < n


def test_cut_error_wide():
    """E_cut: the model's largest relative distance from the extended-precision forward score of the spelled-out sequence."""
    if np.finfo(np.longdouble).eps > 1e-18:
        pytest.skip("needs an extended long double")
    e_cut = 0.0
    for post, seq, edits in rr.wide_cases():
        score, ll = rr.rescore(post, seq, edits)
        for e, got in zip(edits, ll):
            hi, lo = fr.forwards_exact(post, np.array(rr.spell(seq, e), dtype=np.int64), full=True)
            assert math.isfinite(hi) and math.isfinite(got)
            err = abs(float((np.longdouble(got) - np.longdouble(hi)) - np.longdouble(lo))) / max(1.0, abs(hi))
            e_cut = max(e_cut, err)
        assert abs(ll[-1] - score) <= 4 * E_REF * max(1.0, abs(score))
    print("E_cut = %.3e (%.3f E_ref)" % (e_cut, e_cut / E_REF))
    assert 0.0 < e_cut <= 4 * E_REF


@pytest.mark.parametrize("k", [1, 3, 5])
def test_edit_states_of_every_single_letter_edit(k):
    from sloika_amd import bio
    rng = np.random.default_rng(5)
    text = ''.join('ACGT'[i] for i in rng.integers(0, 4, size=23)) + 'AAAAAAAA' + 'ACACACAC'
    old = bio.seq_to_states(text, k)
    assert list(old) == rr.states_of(text, k) == [bio.kmer_mapping(k)[x] for x in bio.seq_to_kmers(text, k)]
    rows = bio.single_letter_edits(text)
    assert [r[:3] for r in rows] == [r[:3] for r in rr.letter_edits(text)] and [r[3] for r in rows] == [r[3] for r in rr.letter_edits(text)]
    assert len(rows) == 8 * len(text) + 4
    most = 0
    for kind, pos, letter, edited in rows:
        assert bio.apply_letter_edits(text, [(kind, pos, letter)]) == edited
        new = bio.seq_to_states(edited, k)
        a, d, ins = bio.edit_states(old, new)
        assert 0 <= a and 0 <= d and a + d <= len(old)
        assert np.array_equal(np.concatenate([old[:a], ins, old[a + d:]]), new)
        assert (a, d, list(ins)) == tuple(rr.strip_common(list(old), list(new)))
        most = max(most, len(ins))
    assert most <= k + 1 <= rr.MAX_NEW
    assert bio.edit_states(old, old) == (len(old), 0, pytest.approx(np.zeros(0)))
    only = bio.single_letter_edits(text, kinds=('del',))
    assert len(only) == len(text) and all(r[0] == 'del' for r in only)
    with pytest.raises(ValueError):
        bio.single_letter_edits(text, kinds=('swap',))


@pytest.fixture(scope="module")
def planted():
    return rr.planted_case()


def test_planted_polish(planted):
    """The three planted errors lie 10 letters apart: one round takes all three, the next accepts nothing."""
    truth, draft, posts = planted
    assert draft != truth and len(draft) == len(truth)
    text, applied, rounds, total = rr.polish(posts, draft, 3)
    print("applied:", applied, "score", total)
    assert text == truth and rounds == 1
    assert sorted(a[1] for a in applied) == ['del', 'ins', 'sub'] and applied[0][1:3] == ('sub', 10)
    rows, gain, again = rr.gains(posts, truth, 3)
    assert again == total and not (gain > 0.0).any()
    assert min(a[4] for a in applied) > 10.0


def test_planted_polish_one_by_one(planted):
    """With one edit per round the truth comes back in three rounds, gains descending."""
    truth, draft, posts = planted
    text, applied, rounds, total = rr.polish(posts, draft, 3, most=1)
    print("applied:", applied)
    assert text == truth and rounds == 3 and len(applied) == 3
