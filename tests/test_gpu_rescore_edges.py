"""Rescoring at every tier of its two kernels (csrc/rescore_edits.hip; design/rescore_edits.md 3, 4 and 6): every number of states per
thread of the lattice kernel under each of its three register budgets, every staging tier of the candidate kernel up to the widest
table and the raised LDS limit, rows at every offset of a granule, pairs of fewer rows than the emissions are fetched ahead, and rows
whose scales lie hundreds of binary places apart.

The truth and the bound are those of tests/test_gpu_rescore.py: tests/forward_ref.forwards_exact (np.longdouble) of the spelled-out
sequence, |device - truth| <= 4 E_ref max(1, |truth|) with E_ref = 3.219e-15, -inf met exactly, no NaN.  The cases come from
tests/rescore_ref.py, and tests/test_rescore_ref.py shows without a GPU that each one lies in the tier it is meant for.

Measured on an MI355X, the largest ratio per group (in E_ref; 4 allowed): deletions over all ownership tiers 0.056 (float64) and
0.050 (float32 with min_prob), the diagonal pairs at 8 / 16 / 32 states per thread 0.039 / 0.046 / 0.058, the staging tiers 0.057,
few rows 0.052, rows of unequal scale 0.053 (random) and 0.040 (alternating).  Before the cut term was freed of its rows' scales
(design/rescore_edits.md 5, step 1) the alternating case gave -inf for 76 of the 86 candidates of either pair."""
import numpy as np
import pytest

from tests.gpu_util import need_gpu, dev
from tests import rescore_ref as rr
from tests.rescore_gpu import E_REF, run, same, exact, ratio

pytestmark = pytest.mark.gpu

MIN_PROB = 1e-5
VARIANTS = ["float64", "float32_min_prob"]


def fed_of(post, variant):
    """(what to hand to the entry, the values it then computes on: decode.prepare_post's, float32 arithmetic, decode.py:36)"""
    if variant == "float64":
        return post, post
    post = post.astype(np.float32)
    return post, (np.float32(MIN_PROB) + np.float32(1.0 - MIN_PROB) * post).astype(np.float32)


def kw_of(variant):
    return {} if variant == "float64" else {"min_prob": MIN_PROB}


def worst_ratio(fed, seq, edits, ll, blank=-1):
    worst = 0.0
    for i, e in enumerate(edits):
        assert not np.isnan(ll[i]), e
        worst = max(worst, ratio(ll[i], exact(fed, rr.spell(seq, e), blank=blank)))
    return worst


def by_budget(cases):
    """The batches that reach rescore_lattice_kernel<T, 2>, <T, 8> and <T, 32> by their longest pair: pair indices per budget."""
    out = {}
    for budget, below in ((2, 512), (8, 2048), (32, 8192)):
        out[budget] = [b for b, c in enumerate(cases) if len(c[1]) < below]
        assert rr.budget_of(max(len(cases[b][1]) for b in out[budget])) == budget
    return out


def run_some(cases, fed, idx, **kw):
    score, ll = run([fed[b] for b in idx], [cases[b][1] for b in idx], [cases[b][2] for b in idx], **kw)
    return {b: (score[i:i + 1], ll[i]) for i, b in enumerate(idx)}


# ---- 1: every ownership tier ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("variant", VARIANTS)
def test_every_ownership_tier_by_long_deletions(variant):
    """T = 40 rows under L = 255 .. 8191 positions, 1 to 32 states per thread: edits that delete all but a few positions read column a
    of F beside thread 0 and column a + d + 1 of B beside the last owning thread.  Every pair alone (max_npos = L: each lattice kernel
    with its own longest pair) and in the three mixed batches that reach <T, 2>, <T, 8> and <T, 32>: the same bits."""
    need_gpu()
    cases = rr.deletion_cases(dtype=np.float64 if variant == "float64" else np.float32)
    given, fed = zip(*[fed_of(c[0], variant) for c in cases])
    assert sorted({rr.ppt_of(len(c[1])) for c in cases}) == [1, 2, 4, 8, 16, 32]
    alone = {}
    for b in range(len(cases)):
        alone.update(run_some(cases, given, [b], **kw_of(variant)))
    assert {rr.budget_of(len(c[1])) for c in cases} == {2, 8, 32}
    for budget, idx in by_budget(cases).items():
        got = run_some(cases, given, idx, **kw_of(variant))
        for b in idx:
            assert same(got[b][0], alone[b][0]) and same(got[b][1], alone[b][1]), (budget, len(cases[b][1]))
    worst = 0.0
    for b, (post, seq, edits) in enumerate(cases):
        score, ll = alone[b]
        assert score[0] == -np.inf and len(ll) == len(edits) and np.isfinite(ll).all(), len(seq)
        w = worst_ratio(fed[b], seq, edits, ll)
        print("deletions %s L = %d (%d states per thread): %d edits, largest ratio %.3f E_ref" % (variant, len(seq), rr.ppt_of(len(seq)), len(edits), w))
        worst = max(worst, w)
    assert worst <= 4.0


@pytest.fixture(scope="module")
def diagonal():
    """Per tier the case and its truths, made once for both entries: the float64 entry gets the float32 entry's prepared values."""
    made = {}

    def get(ppt):
        if ppt not in made:
            T, L = {p: (t, n) for p, t, n in rr.DIAGONAL}[ppt]
            post, seq, edits, _ = rr.diagonal_case(T, L, full=ppt < 32)
            fed = fed_of(post, "float32_min_prob")[1]
            made[ppt] = (post, fed, seq, edits, exact(fed, seq), [exact(fed, rr.spell(seq, e)) for e in edits])
        return made[ppt]
    return get


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("ppt", [8, 16, 32])
def test_diagonal_pair_of_an_upper_tier(diagonal, ppt, variant):
    """(T, L) = (1100, 1030), (2100, 2050), (4200, 4100) on a posterior that follows the sequence: edits whose columns of F and B lie
    on both sides of thread boundaries in the first, a middle and the last owning wave, and at both ends."""
    need_gpu()
    post, fed, seq, edits, t_score, t_edits = diagonal(ppt)
    assert rr.ppt_of(len(seq)) == ppt and np.isfinite(float(t_score))
    if variant == "float64":
        score, ll = run([fed.astype(np.float64)], [seq], [edits], workspace_limit=320 << 20)
    else:
        score, ll = run([post], [seq], [edits], min_prob=MIN_PROB, workspace_limit=320 << 20)
    worst = ratio(score[0], t_score)
    for i, e in enumerate(edits):
        assert np.isfinite(ll[0][i]), e
        worst = max(worst, ratio(ll[0][i], t_edits[i]))
    print("diagonal %s, %d states per thread: score %.3f, %d edits, largest ratio %.3f E_ref" % (variant, ppt, score[0], len(edits), worst))
    assert worst <= 4.0
    assert abs(ll[0][-1] - score[0]) <= 4 * E_REF * max(1.0, abs(score[0]))            # the identity edit


# ---- 2: every staging tier and the widest table -------------------------------------------------------------------------------------

STAGE = [(dt, S) for dt in ("float32", "float64") for S in rr.STAGE_S[np.dtype(dt)]]


@pytest.mark.parametrize("dtype,S", STAGE)
def test_every_staging_tier(dtype, S):
    """T = 12, L = 6 on rows of S columns, on both sides of 2 -> 5 -> 17 granules per thread and of 64 KB of LDS, up to 8192 columns;
    the blank, the sequence and the new symbols sit where staging changes hands (rescore_ref.edge_columns).  Rows that begin 1, 2
    and 3 values (float64: 1) behind an aligned address give the same bits, and the float32 entry those of the float64 entry on the
    widened rows."""
    need_gpu()
    post, seq, edits = rr.stage_case(S, dtype)
    score, ll = run([post], [seq], [edits])
    worst = max(ratio(score[0], exact(post, seq)), worst_ratio(post, seq, edits, ll[0]))
    assert np.isfinite(score[0]) and np.isfinite(ll[0]).all()
    print("staging %s S = %d (%d granules, %d per thread, %d bytes of LDS): largest ratio %.3f E_ref"
          % (dtype, S, rr.gran_of(S, post.itemsize), rr.nch_of(rr.gran_of(S, post.itemsize)), rr.lds_of(rr.gran_of(S, post.itemsize)), worst))
    assert worst <= 4.0
    for lead in range(1, 16 // post.itemsize):
        s2, l2 = run([post], [seq], [edits], lead=lead)
        assert same(s2, score) and same(l2[0], ll[0]), lead
    if dtype == "float32":
        s2, l2 = run([post.astype(np.float64)], [seq], [edits])
        assert same(s2, score) and same(l2[0], ll[0])


@pytest.mark.parametrize("S", [65, 2045])
def test_staging_in_the_network_layout_float32(S):
    """[T, B = 3, ld] float32 with ld = S + 1, S + 2 and S + 3, NaN between the rows: the bits of the packed run."""
    need_gpu()
    from sloika_amd import decode
    cases = [rr.stage_case(S, np.float32, seed=80 + b) for b in range(3)]
    score, ll = run([c[0] for c in cases], [c[1] for c in cases], [c[2] for c in cases])
    assert np.isfinite(score).all() and all(np.isfinite(v).all() for v in ll)
    for ld in (S + 1, S + 2, S + 3):
        post = np.full((rr.STAGE_T, 3, ld), np.nan, dtype=np.float32)
        for b, c in enumerate(cases):
            post[:, b, :S] = c[0]
        s2, l2 = decode.rescore_edits_batch(dev(post)[:, :, :S], [c[1] for c in cases], [c[2] for c in cases])
        assert same(s2.cpu().numpy(), score), ld
        for b in range(3):
            assert same(l2[b].cpu().numpy(), ll[b]), (ld, b)


# ---- 3: few rows ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("variant", VARIANTS)
def test_few_rows_in_every_tier(variant):
    """T = 0 .. 5 rows (below, at and above the 1, 2 and 4 rows that emissions are fetched ahead) under 2 to 32 states per thread, and
    the pair without rows and without positions, whose empty edit scores 0.0 exactly.  decode.rescore_edits_batch takes a pair
    without rows among others (only a batch without any row has no posterior to point at), so nothing here needs the bare entry.
    The three batches that reach <T, 2>, <T, 8> and <T, 32> give the same bits."""
    need_gpu()
    cases = rr.few_rows_cases(dtype=np.float64 if variant == "float64" else np.float32)
    given, fed = zip(*[fed_of(c[0], variant) for c in cases])
    groups = by_budget(cases)
    got = {budget: run_some(cases, given, idx, **kw_of(variant)) for budget, idx in groups.items()}
    worst, ninf, nfin = 0.0, 0, 0
    for b, (post, seq, edits) in enumerate(cases):
        score, ll = got[32][b]
        for budget in (2, 8):
            if b in got[budget]:
                assert same(got[budget][b][0], score) and same(got[budget][b][1], ll), (budget, post.shape[0], len(seq))
        worst = max(worst, ratio(score[0], exact(fed[b], seq)), worst_ratio(fed[b], seq, edits, ll))
        ninf += int(np.isinf(ll).sum())
        nfin += int(np.isfinite(ll).sum())
        if len(seq):
            assert score[0] == -np.inf and ll[0] != -np.inf and ll[2] == -np.inf, (post.shape[0], len(seq))
    assert len(cases[-1][1]) == 0 and cases[-1][0].shape[0] == 0
    assert got[32][len(cases) - 1][0][0] == 0.0 and got[32][len(cases) - 1][1][0] == 0.0
    print("few rows %s: %d finite and %d -inf edits, largest ratio %.3f E_ref" % (variant, nfin, ninf, worst))
    assert ninf > 0 and nfin > 0 and worst <= 4.0


# ---- 4: the exponent sum --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("variant", ["random", "alternate"])
def test_rows_of_unequal_scale(variant):
    """Row t times 2^-k_t, k_t random in 0 .. 200, or 0 and 600 on neighbouring rows: the running exponents of the lattices and the
    (mantissa, exponent) sum of the cut terms move by hundreds of places from row to row, in both directions.  The scaling is exact,
    so the truth is that of the unscaled rows less ln 2 times the sum of k (tests/test_rescore_ref.py); it is computed on the scaled
    rows all the same.
    No case has neighbouring exponents more than 4096 apart: a finite float64 row total moves a running exponent by 1088 at the most
    (1075 places of the format and 13 of the 8192 columns), and the shifts that re_clamp_shift limits never point upwards past t = 0,
    where the sum is still 0; a finite double that goes down by 2098 places or more is 0 whatever the shift, so the clamp at 4096
    keeps the conversion to int defined and cannot change a result."""
    need_gpu()
    worst = 0.0
    for post, seq, edits, _, k in rr.scaled_cases(variant):
        score, ll = run([post], [seq], [edits])
        assert np.isfinite(score[0]) and np.isfinite(ll[0]).all()
        w = max(ratio(score[0], exact(post, seq)), worst_ratio(post, seq, edits, ll[0]))
        print("scaled rows, %s, T = %d: sum of k %d, score %.3f, largest ratio %.3f E_ref" % (variant, post.shape[0], int(k.sum()), score[0], w))
        worst = max(worst, w)
    assert worst <= 4.0
