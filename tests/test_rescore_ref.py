"""The rescoring identity of design/rescore_edits.md on the CPU: tests/rescore_ref.py (the stored lattices and the cut sum, plain float64
loops) against the forward score of the spelled-out sequence (tests/forward_ref.py), bio.edit_states, and the planted polish case.

E_ref = 3.219e-15 is design/forward_score.md 5: the reference recursion's own distance from the exact value.  E_cut, the model's
largest distance from the extended-precision value over rescore_ref.wide_cases, is 1.5e-16 (0.05 E_ref)."""
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


# ---- the cases of tests/test_gpu_rescore_edges.py: each lies in the tier it is meant for, and the model agrees with the truth on it ----

def exact(post, seq):
    hi, lo = fr.forwards_exact(post, np.asarray(seq, dtype=np.int64), full=True)
    return np.longdouble(hi) + np.longdouble(lo)


def model_against_truth(post, seq, edits):
    """rescore_ref.rescore within 4 E_ref of the extended-precision score of every spelled-out edit, -inf in exactly the same places:
    -> (score, [ll], the largest ratio)."""
    score, ll = rr.rescore(post, seq, edits)
    worst = 0.0
    for got, truth in [(score, exact(post, seq))] + [(g, exact(post, rr.spell(seq, e))) for e, g in zip(edits, ll)]:
        if not np.isfinite(truth):
            assert got == float(truth)
            continue
        assert math.isfinite(got)
        worst = max(worst, float(abs(np.longdouble(got) - truth)) / (E_REF * max(1.0, abs(float(truth)))))
    assert worst <= 4.0
    return score, ll, worst


def test_ownership_tiers_of_the_generated_cases():
    """States per thread by L + 1, the lattice kernel by the longest pair of a launch, rows against the fetch depth."""
    assert [rr.ppt_of(L) for L in (0, 255, 256, 511, 512, 1023, 1024, 2047, 2048, 4095, 4096, 8191)] == [1, 1, 2, 2, 4, 4, 8, 8, 16, 16, 32, 32]
    assert [rr.ppt_of(L) for L in rr.TIER_L] == [1, 2, 2, 4, 4, 8, 8, 16, 16, 32, 32]
    assert [rr.budget_of(L) for L in rr.TIER_L] == [2, 2, 2, 8, 8, 8, 8, 32, 32, 32, 32]
    for L in rr.TIER_L[:-1]:                                       # L + 1 on both sides of every boundary: 256 ppt states, and one more
        assert (L + 1) % 256 in (0, 1)
    assert {(L + 1) // 256 for L in rr.TIER_L if (L + 1) % 256 == 0} == {1, 2, 4, 8, 16, 32}
    assert {L // 256 for L in rr.TIER_L if (L + 1) % 256 == 1} == {1, 2, 4, 8, 16}
    assert [rr.ahead_of(p) for p in (1, 2, 4, 8, 16, 32)] == [4, 4, 4, 2, 1, 1]
    # few rows: 2 to 32 states per thread, each with fewer rows than it fetches ahead, as many, and more
    assert sorted({rr.ppt_of(L) for L in rr.FEW_L}) == [2, 4, 8, 16, 32]
    assert {rr.budget_of(L) for L in rr.FEW_L} == {2, 8, 32}
    for L in rr.FEW_L:
        d = rr.ahead_of(rr.ppt_of(L))
        assert min(rr.FEW_T) < d and d in rr.FEW_T and max(rr.FEW_T) > d and 0 in rr.FEW_T
    # the diagonal pairs
    for ppt, T, L in rr.DIAGONAL:
        assert rr.ppt_of(L) == ppt and T >= L + rr.MAX_NEW
    assert [rr.budget_of(L) for _, _, L in rr.DIAGONAL] == [8, 32, 32]


def test_deletion_edits_by_their_shapes():
    """Every tier's edits: inside the sequence, at most T positions left (finite), the first and the last column of both lattices
    among the columns read, all four values of a, of L - a - d and of m present."""
    rng = np.random.default_rng(1)
    for L in rr.TIER_L:
        edits = rr.deletion_edits(L, rr.TIER_T, rng)
        assert len(edits) >= 48
        for a, d, new in edits:
            assert 0 <= a and 0 <= d and a + d <= L and len(new) <= rr.MAX_NEW and L - d + len(new) <= rr.TIER_T < L
        assert {e[0] for e in edits} == {0, 1, 10, 30} and {L - e[0] - e[1] for e in edits} == {0, 1, 5, 20}
        assert {len(e[2]) for e in edits} == {0, 1, 3, 8}
        ppt = rr.ppt_of(L)
        assert {e[0] // ppt for e in edits} >= {0} and {(e[0] + e[1] + 1) // ppt for e in edits if e[0] + e[1] < L} == {L // ppt, (L - 4) // ppt, (L - 19) // ppt}


def test_model_on_the_deletion_cases():
    worst = 0.0
    for post, seq, edits in rr.deletion_cases(lengths=[L for L in rr.TIER_L if L <= 2048]):
        score, ll, w = model_against_truth(post, seq, edits)
        assert score == -math.inf and all(math.isfinite(v) for v in ll)
        worst = max(worst, w)
    print("deletions: the model's largest ratio %.3f E_ref" % worst)


def test_diagonal_edits_lie_on_thread_boundaries():
    for ppt, T, L in rr.DIAGONAL:
        post, seq, edits, named = rr.diagonal_case(T, L, full=ppt < 32)
        assert post.dtype == np.float32 and post.shape == (T, 65) and len(seq) == L and 12 <= len(edits) <= 20
        threads = rr.boundary_threads(L)
        last = L // ppt
        assert threads[0] == 1 and threads[-1] == last and len(threads) == 3
        assert threads[0] // 64 == 0 and 0 < threads[1] // 64 < last // 64 and threads[1] % 64 == 0
        for tid, spans in zip(threads, named):
            j0 = tid * ppt
            edge = {j0 - 1, j0, min(j0 + ppt - 1, L), min(j0 + ppt, L)}
            n = 3 if min(j0 + ppt - 1, L) < min(j0 + ppt, L) else 2
            assert {a for a, _ in spans[:n]} | {b for _, b in spans[:n]} == edge
            for a, b in spans:
                assert (a, b - 1 - a) in [(e[0], e[1]) for e in edits] and 0 <= a < b <= L
        for a, d, new in edits:
            assert 0 <= a and 0 <= d and a + d <= L and L - d + len(new) <= T and len(new) - d <= 2
        assert {len(e[2]) for e in edits} == {0, 1, 8}
        assert any(e[0] == 0 for e in edits) and any(e[0] + e[1] == L for e in edits)
        a, d, new = edits[-1]
        assert d == 1 and list(new) == [seq[a]]                    # the identity edit
        assert np.isfinite(float(exact(post, seq)))                 # the planted path: the pair's own score is finite


def test_staging_tiers_of_the_generated_cases():
    """Granules, registers per thread and LDS by S, and the planted columns against every alignment the rows of a run have."""
    want = {"float32": [2, 5, 5, 17, 17, 17, 17], "float64": [2, 5, 5, 17, 17, 17]}
    for name, tiers in want.items():
        dt = np.dtype(name)
        sizes = rr.STAGE_S[dt]
        grans = [rr.gran_of(S, dt.itemsize) for S in sizes]
        assert [rr.nch_of(g) for g in grans] == tiers
        assert {512, 513, 1280, 1281} <= set(grans)                # both sides of 2 -> 5 -> 17
        assert max(sizes) == 8192 and rr.lds_of(max(grans)) == 2 * 16 * (8192 * dt.itemsize // 16 + 1)
        assert any(rr.lds_of(g) > 64 * 1024 for g in grans) and any(rr.lds_of(g) <= 64 * 1024 and rr.nch_of(g) == 17 for g in grans)
        for S, g in zip(sizes, grans):
            assert g <= 17 * 256
            post, seq, edits = rr.stage_case(S, dt)
            assert post.dtype == dt and post.shape == (rr.STAGE_T, S) and len(seq) == rr.STAGE_L
            used = {int(c) for c in seq} | {int(c) for e in edits for c in e[2]} | {S - 1}
            assert used >= set(rr.planted_columns(S, dt.itemsize))
            per = 16 // dt.itemsize
            seen = set()
            for lead in range(per):
                for t in range(rr.STAGE_T):
                    ms = rr.row_mis(t, S, dt.itemsize, lead)
                    seen.add(ms)
                    edge = rr.edge_columns(S, dt.itemsize, ms)
                    ngran = (ms + S + per - 1) // per
                    assert ngran <= g and {0, S - 1} <= set(edge) <= used
                    # value c of the row sits in slot c + ms of the staged row: the named columns are granule edges
                    assert (per - 1) in {c + ms for c in edge} and (ngran - 1) * per in {c + ms for c in edge}
                    for k in range(1, 17):
                        if 256 * k < ngran:
                            assert {256 * k * per - 1 - ms, 256 * k * per - ms} <= set(edge), (S, ms, k)
            assert seen == set(range(per))                          # rows begin at every offset of a granule
            for a, d, new in edits:
                assert 0 <= a and 0 <= d and a + d <= rr.STAGE_L and rr.STAGE_L - d + len(new) <= rr.STAGE_T
            # distinct values: a neighbouring column cannot pass for the right one
            cols = np.array(sorted(used))
            for c in (cols - 1, cols + 1):
                ok = (c >= 0) & (c < S)
                assert (post[:, cols[ok]] != post[:, c[ok]]).all()
    # the float32 threshold of the raised limit lies between 8188 and 8189 columns
    assert rr.lds_of(rr.gran_of(8188, 4)) == 64 * 1024 and rr.lds_of(rr.gran_of(8189, 4)) > 64 * 1024
    assert rr.lds_of(rr.gran_of(4094, 8)) == 64 * 1024 and rr.lds_of(rr.gran_of(4095, 8)) > 64 * 1024
    # the network-layout cases: rows ld = S + 1 .. S + 3 apart begin at every offset, too
    for S in (65, 2045):
        assert {rr.row_mis(t * 3 + b, ld, 4) for ld in (S + 1, S + 2, S + 3) for t in range(rr.STAGE_T) for b in range(3)} == {0, 1, 2, 3}
        assert rr.nch_of(rr.gran_of(S, 4)) == (2 if S == 65 else 5)


def test_model_on_few_rows():
    """T = 0 .. 5 under up to 2048 positions: -inf where more positions are left than there are rows, and nowhere else."""
    cases = rr.few_rows_cases(lengths=[L for L in rr.FEW_L if L <= 2048])
    ninf = nfin = 0
    for post, seq, edits in cases:
        T, L = post.shape[0], len(seq)
        score, ll, _ = model_against_truth(post, seq, edits)
        for (a, d, new), got in zip(edits, ll):
            assert 0 <= a and 0 <= d and a + d <= L and len(new) <= rr.MAX_NEW and L - d + len(new) <= T + 1
            assert (got == -math.inf) == (L - d + len(new) > T) and not math.isnan(got)
            ninf += got == -math.inf
            nfin += math.isfinite(got)
        if L:
            assert score == -math.inf and [(e[0], e[1], len(e[2])) for e in edits[:3]] == [(0, L, 0), (0, L, T), (0, L, T + 1)]
            assert any(e[0] > 0 for e in edits) and any(0 < e[0] + e[1] < L for e in edits)
    post, seq, edits = cases[-1]
    assert post.shape[0] == 0 and len(seq) == 0 and [(e[0], e[1], len(e[2])) for e in edits] == [(0, 0, 0)]
    assert rr.rescore(post, seq, edits) == (0.0, [0.0])
    assert ninf > 50 and nfin > 50


@pytest.mark.parametrize("variant", ["random", "alternate"])
def test_model_on_rows_of_unequal_scale(variant):
    """Row t times 2^-k_t is exact: the truth moves by ln 2 times the sum of k and nothing else, and the model stays within its bound
    although neighbouring rows, and with them the stored lattice rows, lie up to 600 binary places apart."""
    ld = np.longdouble
    for post, seq, edits, plain, k in rr.scaled_cases(variant):
        assert np.array_equal(np.ldexp(post, k[:, None]), plain) and post.min() > 0.0
        assert (k.max() == 600 and set(k[::2]) == {0} and set(k[1::2]) == {600}) if variant == "alternate" else (150 < k.max() <= 200 and k.min() < 50)
        model_against_truth(post, seq, edits)
        shift = ld(int(k.sum())) * np.log(ld(2))
        for e in edits[::7]:
            s = rr.spell(seq, e)
            a, b = exact(post, s), exact(plain, s)
            assert abs((b - a) - shift) <= 8 * np.finfo(ld).eps * abs(a)
        # the exponents the candidates add: their steps from row to row are what the (mantissa, exponent) sum has to follow
        F, B, EF, EB = rr.lattice(post, seq)
        e = np.array([EF[t + 1] + EB[t] for t in range(post.shape[0])])
        assert np.abs(np.diff(e)).max() >= (500 if variant == "alternate" else 100) and (np.diff(e) > 0).any() and (np.diff(e) < 0).any()
        assert np.abs(np.diff(EF)).max() <= 1088


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
