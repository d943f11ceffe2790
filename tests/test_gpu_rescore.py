"""Rescoring of edited sequences on the device (csrc/rescore_edits.hip through decode.rescore_edits_batch, polish and
pipeline.Basecaller.rescore_chunks / polish_chunks; design/rescore_edits.md).

The truth is tests/forward_ref.forwards_exact (np.longdouble) of the spelled-out sequence, full length; the bound is
|device - truth| <= 4 E_ref max(1, |truth|) with E_ref = 3.219e-15 (design/forward_score.md 5), for ll_edit and for score alike.  The
model of tests/rescore_ref.py says where -inf and NaN stand.  Everything else is bit equality or exact structure.
Measured on an MI355X: the largest ratio is 0.058 E_ref on the tiny exhaustive set, 0.050 on S = 65 and 1025, 0.049 for the float32
entry with min_prob, and 0.051 (of the 8 allowed) between the chunk-sized pair and decode.forwards_batch."""
import ctypes
import math

import numpy as np
import pytest

from tests.gpu_util import need_gpu, dev
from tests import rescore_ref as rr

pytestmark = pytest.mark.gpu

from tests.rescore_gpu import E_REF, SENTINEL, run, same, exact, ratio, raw_call                  # noqa: F401


# ---- 1: accuracy ---------------------------------------------------------------------------------------------------------------

def test_tiny_exhaustive():
    """T in {1, 2, 3, 5, 9} x L in {0, 1, 2, 4}, every (a, d), m in {0, 1, 2, 8}: one launch of 20 pairs and 500 candidates."""
    need_gpu()
    cases = rr.tiny_cases()
    score, ll = run([c[0] for c in cases], [c[1] for c in cases], [c[2] for c in cases])
    worst = n = ninf = 0
    for b, (post, seq, edits) in enumerate(cases):
        worst = max(worst, ratio(score[b], exact(post, seq)))
        model = rr.rescore(post, seq, edits)[1]
        for i, e in enumerate(edits):
            n += 1
            ninf += math.isinf(model[i])
            assert math.isinf(model[i]) == math.isinf(ll[b][i]) and not math.isnan(ll[b][i])
            worst = max(worst, ratio(ll[b][i], exact(post, rr.spell(seq, e))))
    print("tiny: %d candidates, %d of them -inf, largest ratio %.3f E_ref" % (n, ninf, worst))
    assert n == 500 and ninf > 0 and worst <= 4.0


@pytest.fixture(scope="module")
def wide():
    return rr.wide_cases()


@pytest.mark.parametrize("variant", ["float64", "float32_min_prob"])
def test_wide(wide, variant):
    """S = 65 and 1025, edits at both ends and inside, m up to 8, an identity edit; the float32 entry with min_prob against the exact
    value on decode.prepare_post's values."""
    need_gpu()
    mp = 1e-5 if variant == "float32_min_prob" else None
    worst = 0.0
    for post, seq, edits in wide:
        if mp:
            post = post.astype(np.float32)
            fed = (np.float32(mp) + np.float32(1.0 - mp) * post).astype(np.float32)      # decode.py:36, float32 arithmetic
        else:
            fed = post
        score, ll = run([post], [seq], [edits], min_prob=mp)
        worst = max(worst, ratio(score[0], exact(fed, seq)))
        model = rr.rescore(fed, seq, edits)[1]
        for i, e in enumerate(edits):
            truth = exact(fed, rr.spell(seq, e))
            worst = max(worst, ratio(ll[0][i], truth))
            assert abs(ll[0][i] - model[i]) <= 4 * E_REF * max(1.0, abs(model[i]))
        assert abs(ll[0][-1] - score[0]) <= 4 * E_REF * max(1.0, abs(score[0]))            # the identity edit
    print("wide %s: largest ratio %.3f E_ref" % (variant, worst))
    assert worst <= 4.0


def test_symbol_on_the_blank_column():
    need_gpu()
    post, seq, edits = rr.wide_cases(((65, 40, 12),))[0]
    seq = seq.copy()
    seq[::4] = 64
    edits = [(a, d, np.where(np.arange(len(n)) % 2 == 0, 64, n)) for a, d, n in edits]
    score, ll = run([post], [seq], [edits])
    worst = ratio(score[0], exact(post, seq))
    for i, e in enumerate(edits):
        worst = max(worst, ratio(ll[0][i], exact(post, rr.spell(seq, e))))
    assert worst <= 4.0


def test_chunk_sized_pair_against_forwards_batch():
    """800 x 1025 float32 rows, 400 positions, every single-letter edit of a 404-letter draft at kmer_len = 5 (3236 candidates, 13
    workgroups); 64 of them against decode.forwards_batch on the spelled-out sequences, within 8 E_ref: both sides are allowed 4."""
    need_gpu()
    import sys
    from tests.conftest import GOLDEN
    sys.path.insert(0, GOLDEN)
    import forward_cases as fc
    from sloika_amd import bio, decode, polish
    rng = np.random.default_rng(31)
    post = np.roll(fc.make_post(77, 800, 1025, "float32"), 1, axis=1)        # (the generator's blank is the last column: here column 0)
    draft = ''.join('ACGT'[i] for i in rng.integers(0, 4, size=404))
    cols, rows, eset = polish.draft_edits(draft, 5, bio.EDIT_KINDS, 'ACGT', 0, 1025)
    assert len(cols) == 400 and len(rows) == 8 * 404 + 4
    pd = dev(post)
    score, ll = decode.rescore_edits_batch(pd, [cols], [eset], blank=0, min_prob=1e-5, row_off=[0, 800])
    score, ll = score.cpu().numpy(), ll[0].cpu().numpy()
    pick = rng.choice(len(rows), size=64, replace=False)
    spelled = [polish.state_columns(bio.seq_to_states(rows[i][3], 5), 0, 1025) for i in pick]
    rows_d = pd.repeat(64, 1)
    want = decode.forwards_batch(rows_d, spelled, full=True, blank=0, min_prob=1e-5, row_off=800 * np.arange(65)).cpu().numpy()
    own = decode.forwards_batch(pd, [cols], full=True, blank=0, min_prob=1e-5, row_off=[0, 800]).cpu().numpy()
    assert np.isfinite(want).all() and np.isfinite(ll).all()
    worst = max(abs(ll[i] - w) / (E_REF * max(1.0, abs(w))) for i, w in zip(pick, want))
    print("chunk-sized pair: largest distance from forwards_batch %.3f E_ref; score %.3f" % (worst, score[0]))
    assert worst <= 8.0
    assert abs(score[0] - own[0]) <= 8 * E_REF * max(1.0, abs(own[0]))


# ---- 2: bits -------------------------------------------------------------------------------------------------------------------

def many_edits(rng, L, S, n):
    out = []
    for _ in range(n):
        a = int(rng.integers(0, L + 1))
        d = int(rng.integers(0, min(3, L - a) + 1))
        out.append((a, d, rng.integers(0, S - 1, size=int(rng.integers(0, 9)))))
    return out


@pytest.fixture(scope="module")
def mixed():
    """7 pairs of mixed lengths, 1, 2 and 4 states per thread among them, one with L = 0 and one without candidates."""
    rng = np.random.default_rng(41)
    out = []
    for b, (T, L) in enumerate(((40, 12), (9, 0), (600, 300), (7, 5), (64, 40), (1200, 600), (5, 3))):
        post = rng.uniform(size=(T, 65)) * rng.uniform(size=(T, 65))
        post[:, -1] += 0.3
        seq = rng.integers(0, 64, size=L)
        if L >= 300:                                              # a likely path along the diagonal: the scores stay finite
            post[np.arange(0, T, 2), seq] += 1.0
        post /= post.sum(axis=1, keepdims=True)
        out.append((post, seq, many_edits(rng, L, 65, 0 if b == 4 else (300 if b == 0 else 70))))
    return out


@pytest.fixture(scope="module")
def mixed_alone(mixed):
    need_gpu()
    return [run([p], [s], [e]) for p, s, e in mixed]


def test_bits_among_other_candidates(mixed):
    need_gpu()
    post, seq, edits = mixed[0]
    score, ll = run([post], [seq], [edits[:257]])
    for n in (1, 63, 64, 65, 255, 256):
        s2, l2 = run([post], [seq], [edits[:n]])
        assert same(s2, score) and same(l2[0], ll[0][:n]), n
    s2, l2 = run([post], [seq], [edits[:257][::-1]])
    assert same(l2[0], ll[0][::-1])
    # the entry itself, which does not sort: every candidate in another lane and another workgroup
    rc, s3, l3, _ = raw_call([post], [seq], [(0,) + e for e in edits[:257][::-1]])
    assert rc == 0 and same(l3, ll[0][::-1]) and same(s3, score)


def test_bits_in_a_batch(mixed, mixed_alone):
    need_gpu()
    score, ll = run([m[0] for m in mixed], [m[1] for m in mixed], [m[2] for m in mixed])
    assert len(ll[4]) == 0
    for b in range(len(mixed)):
        assert same(score[b:b + 1], mixed_alone[b][0]) and same(ll[b], mixed_alone[b][1][0]), b
    assert np.isfinite(score).all() and all(np.isfinite(v).any() for b, v in enumerate(ll) if b != 4)


def test_bits_under_a_workspace_limit(mixed, mixed_alone):
    need_gpu()
    from sloika_amd import _lib, transducer
    L = _lib.lib()
    alone = []
    for post, seq, _ in mixed:
        nrow, pos = np.array([post.shape[0]], dtype=np.int32), np.array([0, len(seq)], dtype=np.int64)
        alone.append(int(L.slk_rescore_edits_workspace_bytes(1, nrow.ctypes.data_as(ctypes.c_void_p), pos.ctypes.data_as(ctypes.c_void_p))))
    limit = max(alone) + 512
    assert len(transducer.workspace_runs([n - 256 + 16 for n in alone], limit - 512)) == 3
    score, ll = run([m[0] for m in mixed], [m[1] for m in mixed], [m[2] for m in mixed], workspace_limit=limit)
    for b in range(len(mixed)):
        assert same(score[b:b + 1], mixed_alone[b][0]) and same(ll[b], mixed_alone[b][1][0]), b
    with pytest.raises(ValueError):
        run([m[0] for m in mixed], [m[1] for m in mixed], [m[2] for m in mixed], workspace_limit=max(alone) - 1)


def test_bits_in_the_network_layout(mixed, mixed_alone):
    need_gpu()
    from sloika_amd import decode
    T = max(m[0].shape[0] for m in mixed)
    post = np.full((T, len(mixed), 67), np.nan)                  # (rows a pair does not own, and two columns past the states)
    for b, m in enumerate(mixed):
        post[:m[0].shape[0], b, :65] = m[0]
    score, ll = decode.rescore_edits_batch(dev(post)[:, :, :65], [m[1] for m in mixed], [m[2] for m in mixed],
                                           lengths=[m[0].shape[0] for m in mixed])
    for b in range(len(mixed)):
        assert same(score[b:b + 1].cpu().numpy(), mixed_alone[b][0]) and same(ll[b].cpu().numpy(), mixed_alone[b][1][0]), b


def test_float32_entry_is_the_float64_entry_on_widened_rows(mixed):
    need_gpu()
    for post, seq, edits in (mixed[0], mixed[2]):
        p32 = post.astype(np.float32)
        a, b = run([p32], [seq], [edits]), run([p32.astype(np.float64)], [seq], [edits])
        assert same(a[0], b[0]) and same(a[1][0], b[1][0])
    # 1025 columns: rows of float32 that begin at every 4-byte offset of a 16-byte granule
    post, seq, edits = rr.wide_cases(((1025, 64, 30),))[0]
    p32 = post.astype(np.float32)
    a, b = run([p32], [seq], [edits]), run([p32.astype(np.float64)], [seq], [edits])
    assert same(a[0], b[0]) and same(a[1][0], b[1][0])


# ---- 3: refusals ---------------------------------------------------------------------------------------------------------------

def test_refused_candidates(mixed):
    need_gpu()
    post, seq, edits = mixed[0]
    L = len(seq)
    good = [(0,) + e for e in edits[:5]]
    bad = [(0, -1, 0, [1]), (0, 0, -1, [1]), (0, L, 1, [1]), (0, 2, L, []), (0, 1, 1, [1] * 9), (0, 1, 1, [2, 65]), (0, 1, 1, [-1])]
    cands = []
    for g, x in zip(good + good, bad):
        cands += [g, x]
    rc, score, ll, _ = raw_call([post], [seq], cands)
    assert rc == 0
    want = run([post], [seq], [edits[:5]])
    assert same(score, want[0])
    for i, c in enumerate(cands):
        if i % 2:
            assert math.isnan(ll[i]), c
        else:
            assert ll[i] == want[1][0][(i // 2) % 5]


def test_refused_pairs(mixed):
    need_gpu()
    (p0, s0, e0), (p3, s3, e3), (p5, s5, e5) = mixed[0], mixed[3], mixed[5]
    broken = s3.copy()
    broken[2] = 65                                                # no column
    cands = [(0,) + e for e in e0[:4]] + [(1,) + e for e in e3[:4]] + [(2,) + e for e in e5[:4]]
    # pair 1 has a symbol that is no column; pair 2 is longer than max_npos says (600 positions in the budget of 511)
    rc, score, ll, _ = raw_call([p0, p3, p5], [s0, broken, s5], cands, max_npos=20)
    assert rc == 0
    want = run([p0], [s0], [e0[:4]])
    assert same(score[:1], want[0]) and same(ll[:4], want[1][0])
    assert np.isnan(score[1:]).all() and np.isnan(ll[4:]).all()


def test_entry_refusals(mixed):
    need_gpu()
    from sloika_amd import _lib, decode
    post, seq, edits = mixed[0]
    cands = [(0,) + e for e in edits[:3]]
    rc, score, ll, need = raw_call([post], [seq], cands)
    assert rc == 0 and need == 256 + 16 * (post.shape[0] + 1) * (len(seq) + 2 + 1)
    rc, score, ll, _ = raw_call([post], [seq], cands, ws_bytes=need - 1)
    assert rc == _lib.SLK_ERR_WORKSPACE and (score == SENTINEL).all() and (ll == SENTINEL).all()
    rc, score, ll, _ = raw_call([post, post], [seq, seq], [(1,) + edits[0], (0,) + edits[1]])      # pairs out of order
    assert rc == _lib.SLK_ERR_INVALID_ARG and (score == SENTINEL).all() and (ll == SENTINEL).all()
    assert decode.rescore_max_new() == 8
    for e in ((1, 1, [1] * 9), (len(seq), 1, [1]), (-1, 0, [1]), (1, 1, [65])):
        with pytest.raises(ValueError):
            run([post], [seq], [[e]])


# ---- 4: end to end -------------------------------------------------------------------------------------------------------------

def test_polish_planted_case():
    """The device takes the model's edits round for round: the gains stand 10 and more apart from every runner-up."""
    need_gpu()
    from sloika_amd import polish
    truth, draft, posts = rr.planted_case()
    want = rr.polish(posts, draft, 3)
    post = dev(np.stack(posts, axis=1))                          # [T, 3, 65]
    got = polish.polish(post, [draft] * 3, 3, group=["g"] * 3, blank=0)
    assert len(got) == 1 and got[0].name == "g"
    assert got[0].sequence == truth == want[0] and got[0].rounds == want[2] == 1
    assert [a[:4] for a in got[0].applied] == [a[:4] for a in want[1]]
    assert np.allclose([a[4] for a in got[0].applied], [a[4] for a in want[1]], rtol=0, atol=1e-9)
    assert abs(got[0].score - want[3]) <= 1e-9
    res = polish.rescore_drafts(post, [truth] * 3, 3, group=[0, 0, 0], blank=0)
    assert not bool((res[0].gain > 0).any())


def test_basecaller_rescore_and_polish_chunks():
    """32 chunks in two groups through a small random network: rescore_chunks' gains are rescore_edits_batch's on posteriors(), and the
    summed score does not decrease from round to round."""
    need_gpu()
    import torch
    from sloika_amd import bio, decode, models, pipeline, polish
    net = models.build_model("raw_0.98_rgrgr", klen=5, sd=0.5, seed=11)
    bc = pipeline.Basecaller(net, kmer_len=5, skip=0.0)
    chunks = torch.from_numpy(pipeline.synthetic_chunks(32, chunk_len=500, seed=7)).cuda()
    rng = np.random.default_rng(3)
    text = [''.join('ACGT'[i] for i in rng.integers(0, 4, size=n)) for n in (30, 41)]
    group = [b % 2 for b in range(32)]
    drafts = [text[g] for g in group]
    res = bc.rescore_chunks(chunks, drafts, group=group)
    assert [r.name for r in res] == [0, 1] and [r.draft for r in res] == text
    post = bc.posteriors(chunks)
    for r in res:
        assert r.pairs == list(range(r.name, 32, 2)) and [e[:3] for e in r.edits] == [e[:3] for e in bio.single_letter_edits(r.draft)]
        cols, rows, eset = polish.draft_edits(r.draft, 5, bio.EDIT_KINDS, 'ACGT', 0, 1025)
        sub = post[:, r.pairs, :]
        score, ll = decode.rescore_edits_batch(sub, [cols] * 16, [eset] * 16, blank=0, min_prob=bc.min_prob)
        want = (torch.stack(ll) - score[:, None]).sum(0)
        assert torch.equal(want, r.gain) and torch.equal(score.sum(), r.score)
        assert same(score.cpu().numpy(), bc.score_chunks(chunks[r.pairs], [r.draft] * 16).cpu().numpy()) or \
            torch.allclose(score, bc.score_chunks(chunks[r.pairs], [r.draft] * 16), rtol=4 * E_REF, atol=0)
    # polishing: every round's string scores at least what the round before scored
    out = bc.polish_chunks(chunks, drafts, group=group, max_rounds=3)
    for g, (r, p) in enumerate(zip(res, out)):
        assert p.name == g and p.rounds <= 3
        now, seq = float(r.score.item()), r.draft
        for rnd in range(p.rounds):
            seq = bio.apply_letter_edits(seq, [a[1:4] for a in p.applied if a[0] == rnd])
            nxt = float(bc.score_chunks(chunks[r.pairs], [seq] * 16).sum().item())
            print("group %d round %d: %.6f -> %.6f" % (g, rnd, now, nxt))
            assert nxt >= now
            now = nxt
        assert seq == p.sequence and abs(now - p.score) <= 1e-9 * max(1.0, abs(now))
    with pytest.raises(NotImplementedError):
        bc2 = pipeline.Basecaller(net, kmer_len=5, skip=0.0)
        bc2.transducer = False
        bc2.rescore_chunks(chunks, drafts, group=group)
