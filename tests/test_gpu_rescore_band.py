"""Banded rescoring of edited sequences on the device (csrc/rescore_band.hip through decode.rescore_edits_banded_batch, the C entry,
polish(band=); design/rescore_band.md).

The truth is tests/rescore_band_ref.truth: the banded identity in np.longdouble with exact scaling, one vector operation per row.  The
bound is the project's, |device - truth| <= 4 E_ref max(1, |truth|) with E_ref = 3.219e-15 (design/forward_score.md 5), for ll_edit
and for score alike; the float64 model of the same file says where -inf and NaN stand.  Everything else is bit equality or exact
structure: with lo all 0 and a width that holds every state the banded entry has the dense entry's bits.
Measured on an MI355X, largest |device - truth| / (E_ref max(1, |truth|)): 0.055 on the ring steps (0.039 / 0.055 / 0.046 at W = 256 /
512 / 2048), 0.035 on the diagonal pairs whose mass goes round the ring (float32 rows with min_prob), 0.034 with 1 .. 5 rows, 0.043 on
the whole read of 20 000 rows x 9 000 positions; the polish gains have the CPU model's bits.  No ratio is near the bound of 4."""
import ctypes
import math

import numpy as np
import pytest

from tests.gpu_util import need_gpu, dev, stream
from tests import rescore_ref as rr
from tests import rescore_band_ref as rb
from tests.rescore_gpu import E_REF, SENTINEL, packed, run, same, ratio

pytestmark = pytest.mark.gpu


def run_band(posts, seqs, edits, los, width, **kw):
    """decode.rescore_edits_banded_batch on packed rows -> (score numpy [B], [ll numpy])."""
    from sloika_amd import decode
    rows, off = packed(posts)
    score, ll = decode.rescore_edits_banded_batch(dev(rows), seqs, edits, los, width, row_off=off, **kw)
    return score.cpu().numpy(), [v.cpu().numpy() for v in ll]


def raw_band(posts, seqs, cands, los, width, ws_bytes=None, min_prob=None, band_off=None, fill=SENTINEL):
    """The C entry itself, nothing checked on the host: cands = [(pair, start, ndel, new)] -> (rc, score, ll, need)."""
    import torch
    from sloika_amd import _lib
    L = _lib.lib()
    rows, off = packed(posts)
    nread = len(posts)
    nrow = np.array([p.shape[0] for p in posts], dtype=np.int32)
    pos = np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).astype(np.int64)
    seq = np.concatenate([np.asarray(s, dtype=np.int32) for s in seqs] + [np.zeros(1, np.int32)])
    noff = np.concatenate([[0], np.cumsum([len(c[3]) for c in cands])]).astype(np.int64)
    new = np.concatenate([np.asarray(c[3], dtype=np.int32) for c in cands] + [np.zeros(1, np.int32)])
    lo = np.concatenate([np.asarray(v, dtype=np.int32) for v in los])
    boff = np.concatenate([[0], np.cumsum([len(v) for v in los])]).astype(np.int64) if band_off is None else np.asarray(band_off, np.int64)
    need = L.slk_rescore_edits_banded_workspace_bytes(nread, nrow.ctypes.data_as(ctypes.c_void_p), width)
    size = max(need, 16 * int(nrow.sum() + nread) * 257 + 4096)                  # (an entry that is refused must find room all the same)
    d = dict(rows=dev(rows), off=dev(off[:nread].copy()), nrow=dev(nrow), seq=dev(seq), pos=dev(pos), lo=dev(lo), boff=dev(boff),
             pair=dev(np.array([c[0] for c in cands] + [0], dtype=np.int32)), start=dev(np.array([c[1] for c in cands] + [0], dtype=np.int32)),
             ndel=dev(np.array([c[2] for c in cands] + [0], dtype=np.int32)), noff=dev(noff), new=dev(new))
    score = torch.full((nread,), fill, dtype=torch.float64, device="cuda")
    ll = torch.full((max(len(cands), 1),), fill, dtype=torch.float64, device="cuda")
    ws = torch.zeros(size, dtype=torch.uint8, device="cuda")
    head = (d["rows"].data_ptr(), rows.shape[1], d["off"].data_ptr(), 1, d["nrow"].data_ptr(), rows.shape[1], d["seq"].data_ptr(),
            d["pos"].data_ptr(), nread, rows.shape[1] - 1)
    tail = (d["lo"].data_ptr(), d["boff"].data_ptr(), width, d["pair"].data_ptr(), d["start"].data_ptr(), d["ndel"].data_ptr(),
            d["noff"].data_ptr(), d["new"].data_ptr(), len(cands), score.data_ptr(), ll.data_ptr(), ws.data_ptr(),
            (need or size) if ws_bytes is None else ws_bytes, stream())
    if rows.dtype == np.float32:
        rc = L.slk_rescore_edits_banded_batch_f32(*head, float(min_prob or 0.0), *tail)
    else:
        rc = L.slk_rescore_edits_banded_batch_f64(*head, *tail)
    torch.cuda.synchronize()
    return rc, score.cpu().numpy(), ll.cpu().numpy()[:len(cands)], need


def against_truth(post, seq, edits, lo, width, score, ll, model=None):
    """-> (largest ratio, finite candidates, -inf candidates); NaN and -inf where the float64 model has them."""
    if model is None:
        ms, ml = rb.evaluate(post, seq, edits, lo, width, -1, np.float64)
        model = (float(ms), [float(v) for v in ml])
    ts, tl = rb.truth(post, seq, edits, lo, width)
    worst, fin, ninf = 0.0, 0, 0
    for got, mod, tru in zip([score] + list(ll), [model[0]] + list(model[1]), [ts] + list(tl)):
        if mod != mod:
            assert got != got
        elif math.isinf(mod):
            assert got == mod, (got, mod)
            ninf += 1
        else:
            worst = max(worst, ratio(got, tru))
            fin += 1
    return worst, fin - (1 if math.isfinite(model[0]) else 0), ninf - (1 if math.isinf(model[0]) else 0)


# ---- 1: the dense tie ------------------------------------------------------------------------------------------------------------

def tie_groups():
    """(width, [(post, seq, edits)]): every pair under the smallest built width that holds its L + 1 states."""
    tiny = rr.tiny_cases()
    wide = rr.wide_cases(((65, 300, 120),))
    out = [(256, tiny), (256, wide)]
    for c in rr.deletion_cases(lengths=(255, 256, 511, 512)):
        out.append((rb.width_for(len(c[1])), [c]))
    return out


@pytest.mark.parametrize("variant", ["float64", "float32_min_prob"])
def test_dense_tie(variant):
    """lo all 0 and a width that holds every state: score and every ll_edit bit for bit the dense entry's, both entries."""
    need_gpu()
    mp = 1e-5 if variant == "float32_min_prob" else None
    widths = []
    for width, cases in tie_groups():
        posts = [c[0].astype(np.float32) if mp else c[0] for c in cases]
        seqs, edits = [c[1] for c in cases], [c[2] for c in cases]
        want = run(posts, seqs, edits, min_prob=mp)
        got = run_band(posts, seqs, edits, [rb.zero_band(p.shape[0]) for p in posts], width, min_prob=mp)
        assert same(got[0], want[0]), width
        for b in range(len(cases)):
            assert same(got[1][b], want[1][b]), (width, b)
        assert any(np.isfinite(v).any() for v in got[1])
        widths.append(width)
    assert sorted(set(widths)) == [256, 512, 1024]


# ---- 2: the ring -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("S,L,W", rb.RING)
def test_ring_steps(S, L, W):
    """T = 40: band steps 0, 1, ppt - 1, ppt, ppt + 1, 64, 255, W - 1 (and W, W + 1, which lose everything behind them), in
    consecutive rows and fs_ahead rows apart; candidates on the band's edges.  Both pairs in one launch."""
    need_gpu()
    cases = [rb.ring_case(S, L, W, lossy=False), rb.ring_case(S, L, W, lossy=True)]
    score, ll = run_band([c[0] for c in cases], [c[1] for c in cases], [c[2] for c in cases], [c[3] for c in cases], W)
    for b, (post, seq, edits, lo) in enumerate(cases):
        model = rb.rescore(post, seq, edits, lo, W)
        worst, fin, ninf = against_truth(post, seq, edits, lo, W, score[b], ll[b], model)
        print("ring L = %d W = %d %s: %d finite, %d -inf, largest ratio %.3f E_ref" % (L, W, "lossy" if b else "kept", fin, ninf, worst))
        assert worst <= 4.0 and fin >= 5 and ninf >= 5


DIAGONAL = ((700, 600, 256), (1500, 1300, 512), (5300, 5000, 2048), (2300, 2100, 1024))       # (T, L, W)


@pytest.mark.parametrize("T,L,W", DIAGONAL)
def test_ring_diagonal(T, L, W):
    """A planted path that the band follows down the whole sequence: the mass itself goes round the ring, more than twice; float32
    rows with min_prob."""
    need_gpu()
    rng = np.random.default_rng(101 + L)
    post, seq, center = rb.diagonal_long(T, L, 65, seed=103 + L)
    lo = rb.band_lo(center, L, W)
    assert (L + 1) / W > 2 and int(lo[-1]) >= W and rb.valid_band(lo, T, L, W)
    edits = rb.letter_edit_sample(seq, 40, 107, 65)
    edits += [(int(a), 2, rng.integers(0, 64, size=8)) for a in rng.integers(0, L - 2, size=8)]
    mp = 1e-5
    fed = (np.float32(mp) + np.float32(1.0 - mp) * post).astype(np.float32)
    score, ll = run_band([post], [seq], [edits], [lo], W, min_prob=mp)
    worst, fin, ninf = against_truth(fed, seq, edits, lo, W, score[0], ll[0])
    print("diagonal T = %d L = %d W = %d: %d finite, %d -inf, largest ratio %.3f E_ref, score %.3f" % (T, L, W, fin, ninf, worst, score[0]))
    assert worst <= 4.0 and fin >= 40 and math.isfinite(score[0])


def test_few_rows():
    """T = 0 .. 5 under L = 300 at W = 256 (below, at and above fs_ahead): without a row there is no valid band, NaN."""
    need_gpu()
    cases = rb.few_rows_cases()
    nfin = 0
    for post, seq, edits, lo in cases:
        T = post.shape[0]
        if T == 0:                                                # (beside a pair that has a row: a launch needs a posterior)
            assert not rb.valid_band(lo, 0, len(seq), 256)
            p1, s1, e1, l1 = cases[1]
            rc, score, ll, _ = raw_band([p1, post], [s1, seq], [(0,) + e for e in e1] + [(1,) + e for e in edits], [l1, lo], 256)
            assert rc == 0 and math.isinf(score[0]) and np.isnan(score[1]) and np.isnan(ll[len(e1):]).all()
            assert not np.isnan(ll[:len(e1)]).any()
            with pytest.raises(ValueError):
                run_band([p1, post], [s1, seq], [e1, edits], [l1, lo], 256)
            continue
        score, ll = run_band([post], [seq], [edits], [lo], 256)
        worst, fin, ninf = against_truth(post, seq, edits, lo, 256, score[0], ll[0], rb.rescore(post, seq, edits, lo, 256))
        print("few rows T = %d: %d finite, %d -inf, largest ratio %.3f E_ref" % (T, fin, ninf, worst))
        assert worst <= 4.0
        nfin += fin
    assert nfin >= 20


# ---- 3: bits -----------------------------------------------------------------------------------------------------------------------

def near_edits(rng, center, L, S, n):
    """Edits beside the centre line of a band: a drawn over the whole sequence, small d, 0 .. 8 new symbols."""
    out = []
    for _ in range(n):
        a = int(rng.integers(0, L + 1))
        d = int(rng.integers(0, min(3, L - a) + 1))
        out.append((a, d, rng.integers(0, S - 1, size=int(rng.integers(0, 9)))))
    return out


@pytest.fixture(scope="module")
def mixed():
    """7 pairs of mixed lengths under W = 256, bands along the diagonal (three of them longer than the ring), one with L = 0 and
    one without candidates: -> [(post, seq, edits, lo)]."""
    rng = np.random.default_rng(43)
    out = []
    for b, (T, L) in enumerate(((40, 12), (9, 0), (600, 300), (7, 5), (64, 40), (1200, 600), (900, 700))):
        post = rng.uniform(size=(T, 65)) * rng.uniform(size=(T, 65))
        post[:, -1] += 0.3
        seq = rng.integers(0, 64, size=L)
        rows = np.sort(rng.choice(T, size=L, replace=False))
        if L >= 300:
            post[rows, seq] += 1.0
        post /= post.sum(axis=1, keepdims=True)
        lo = rb.band_lo(rb.center_from_rows(rows, T), L, 256)
        out.append((post, seq, near_edits(rng, None, L, 65, 0 if b == 4 else (300 if b == 6 else 70)), lo))
    return out


def run_mixed(ms, **kw):
    return run_band([m[0] for m in ms], [m[1] for m in ms], [m[2] for m in ms], [m[3] for m in ms], 256, **kw)


@pytest.fixture(scope="module")
def mixed_alone(mixed):
    need_gpu()
    return [run_mixed([m]) for m in mixed]


def test_bits_among_other_candidates(mixed):
    need_gpu()
    post, seq, edits, lo = mixed[6]
    score, ll = run_band([post], [seq], [edits[:257]], [lo], 256)
    assert np.isfinite(ll[0]).sum() > 100
    for n in (1, 63, 64, 65, 255, 256):
        s2, l2 = run_band([post], [seq], [edits[:n]], [lo], 256)
        assert same(s2, score) and same(l2[0], ll[0][:n]), n
    for k in (0, 100, 256):                                       # alone: the workgroup walks this candidate's rows only
        s2, l2 = run_band([post], [seq], [edits[k:k + 1]], [lo], 256)
        assert same(l2[0], ll[0][k:k + 1]), k
    s2, l2 = run_band([post], [seq], [edits[:257][::-1]], [lo], 256)
    assert same(l2[0], ll[0][::-1])
    # the entry itself, which does not sort: every candidate in another lane and another workgroup
    rc, s3, l3, _ = raw_band([post], [seq], [(0,) + e for e in edits[:257][::-1]], [lo], 256)
    assert rc == 0 and same(l3, ll[0][::-1]) and same(s3, score)


def test_bits_in_a_batch(mixed, mixed_alone):
    need_gpu()
    score, ll = run_mixed(mixed)
    assert len(ll[4]) == 0
    for b in range(len(mixed)):
        assert same(score[b:b + 1], mixed_alone[b][0]) and same(ll[b], mixed_alone[b][1][0]), b
    assert np.isfinite(score).all() and all(np.isfinite(v).any() for b, v in enumerate(ll) if b != 4)


def test_bits_under_a_workspace_limit(mixed, mixed_alone):
    need_gpu()
    from sloika_amd import _lib, transducer
    L = _lib.lib()
    alone = []
    for m in mixed:
        nrow = np.array([m[0].shape[0]], dtype=np.int32)
        alone.append(int(L.slk_rescore_edits_banded_workspace_bytes(1, nrow.ctypes.data_as(ctypes.c_void_p), 256)))
        assert alone[-1] == 256 + 16 * (m[0].shape[0] + 1) * 257
    limit = max(alone) + 512
    assert len(transducer.workspace_runs([n - 256 + 16 for n in alone], limit - 512)) == 3
    score, ll = run_mixed(mixed, workspace_limit=limit)
    for b in range(len(mixed)):
        assert same(score[b:b + 1], mixed_alone[b][0]) and same(ll[b], mixed_alone[b][1][0]), b
    with pytest.raises(ValueError):
        run_mixed(mixed, workspace_limit=max(alone) - 1)


def test_bits_in_the_network_layout(mixed, mixed_alone):
    need_gpu()
    from sloika_amd import decode
    T = max(m[0].shape[0] for m in mixed)
    post = np.full((T, len(mixed), 67), np.nan)                  # (rows a pair does not own, and two columns past the states)
    for b, m in enumerate(mixed):
        post[:m[0].shape[0], b, :65] = m[0]
    score, ll = decode.rescore_edits_banded_batch(dev(post)[:, :, :65], [m[1] for m in mixed], [m[2] for m in mixed],
                                                  [m[3] for m in mixed], 256, lengths=[m[0].shape[0] for m in mixed])
    for b in range(len(mixed)):
        assert same(score[b:b + 1].cpu().numpy(), mixed_alone[b][0]) and same(ll[b].cpu().numpy(), mixed_alone[b][1][0]), b


def test_float32_entry_is_the_float64_entry_on_widened_rows(mixed):
    need_gpu()
    for post, seq, edits, lo in (mixed[0], mixed[5], mixed[6]):
        p32 = post.astype(np.float32)
        a = run_band([p32], [seq], [edits], [lo], 256)
        b = run_band([p32.astype(np.float64)], [seq], [edits], [lo], 256)
        assert same(a[0], b[0]) and same(a[1][0], b[1][0])
    # 1025 columns: rows of float32 that begin at every 4-byte offset of a 16-byte granule
    post, seq, edits = rr.wide_cases(((1025, 64, 30),))[0]
    p32 = post.astype(np.float32)
    lo = rb.zero_band(64)
    a, b = run_band([p32], [seq], [edits], [lo], 256), run_band([p32.astype(np.float64)], [seq], [edits], [lo], 256)
    assert same(a[0], b[0]) and same(a[1][0], b[1][0])


# ---- 4: past the dense limit -------------------------------------------------------------------------------------------------------

def test_whole_read():
    """T = 20 000 rows, L = 9 000 positions, S = 65, W = 256: 82 MB of workspace where dense lattices would take 2.9 GB and the dense
    entry refuses the pair; 64 seeded single-symbol edits against the truth."""
    need_gpu()
    from sloika_amd import decode
    post, seq, center = rb.diagonal_long()
    T, L = post.shape[0], len(seq)
    assert (T, L) == (20000, 9000) and L > decode.forward_max_positions()
    lo = rb.band_lo(center, L, 256)
    edits = rb.letter_edit_sample(seq, 64, 5, 65)
    pd = dev(post)
    with pytest.raises(ValueError):
        decode.rescore_edits_batch(pd, [seq], [edits], row_off=[0, T])
    score, ll = decode.rescore_edits_banded_batch(pd, [seq], [edits], [lo], 256, row_off=[0, T])
    score, ll = score.cpu().numpy(), ll[0].cpu().numpy()
    worst, fin, ninf = against_truth(post, seq, edits, lo, 256, score[0], ll)
    print("whole read: score %.3f, %d finite, largest ratio %.3f E_ref" % (score[0], fin, worst))
    assert worst <= 4.0 and fin == 64 and math.isfinite(score[0])


# ---- 5: polish ---------------------------------------------------------------------------------------------------------------------

def test_polish_planted_long():
    """T = 3 000, L = 1 000 k-mers, three reads, a substitution, a deletion and an insertion more than 300 letters apart, W = 256:
    polish(band=) takes the model's edits round for round, and the dense polish's; the gains lie within the bound of the model.
    A gain is a sum over the reads of ll_edit - score, each side allowed 4 E_ref max(1, |value|) and every value about the read's
    score: 8 E_ref (|summed score| + 3) bounds it."""
    need_gpu()
    from sloika_amd import polish
    truth, draft, posts, centers = rb.planted_long()
    post = dev(np.stack(posts, axis=1))                          # [T, 3, 65]
    want = rb.polish(posts, draft, 3, centers, 256)
    got = polish.polish(post, [draft] * 3, 3, group=["g"] * 3, blank=0, band=(centers, 256))
    dense = polish.polish(post, [draft] * 3, 3, group=["g"] * 3, blank=0)
    assert got[0].sequence == truth == want[0] == dense[0].sequence and got[0].rounds == want[2] == dense[0].rounds
    assert [a[:4] for a in got[0].applied] == [a[:4] for a in want[1]] == [a[:4] for a in dense[0].applied]
    bound = 8 * E_REF * (abs(want[3]) + 3)
    diff = max(abs(g[4] - w[4]) for g, w in zip(got[0].applied, want[1]))
    print("polish: gains %s, largest distance from the model %.3g (bound %.3g); score %.6f against the dense %.6f"
          % ([round(a[4], 3) for a in got[0].applied], diff, bound, got[0].score, dense[0].score))
    assert diff <= bound and abs(got[0].score - want[3]) <= bound
    # the band never adds likelihood, and round a planted path 256 states lose nothing the bound can tell (design/rescore_band.md 5)
    assert got[0].score <= dense[0].score + bound and abs(got[0].score - dense[0].score) <= bound
    # (the second round ran on centre lines moved by shift_center, nothing was re-aligned); the truth has no positive candidate
    res = polish.rescore_drafts(post, [truth] * 3, 3, group=[0, 0, 0], blank=0, band=(centers, 256))
    assert not bool((res[0].gain > 0).any())


def test_basecaller_rescore_and_polish_reads():
    """Two synthetic reads of unequal length through a small built model: rescore_reads / polish_reads against their own calls are
    polish.rescore_drafts / polish(band=) on the posterior rows of the same reads, bit for bit; the centre lines are recomputed
    here from the calls' moves; given drafts take centre lines, or the remap's."""
    need_gpu()
    import torch
    from sloika_amd import bio, models, pipeline, polish
    net = models.randomise_zero_layers(models.build_model("raw_0.98_rgrgr", klen=5, sd=0.5, seed=7))
    bc = pipeline.Basecaller(net, kmer_len=5, skip=0.0)
    base = pipeline.synthetic_chunks(2, chunk_len=3000, seed=21)
    reads = [base[0], base[1][:2200]]
    res = bc.rescore_reads(reads, width=256)
    scores, paths, lens, move_row, conf, logz, nsamp = bc.call_reads_qual(reads)
    calls = bio.paths_to_bases(paths, lens, 5)
    assert [r.draft for r in res] == calls and [r.pairs for r in res] == [[0], [1]]
    padded, ns = bc._padded_reads(reads, (0, 0), 0.0, None, "test")
    post, steps = bc._read_posteriors(padded, ns)
    rows = steps.cpu().numpy()
    centers = []
    for b in range(2):
        n = int(lens[b])
        states = paths[b, :n].cpu().numpy().astype(np.int64)
        letters = np.concatenate([[5], np.minimum(bio.moves_of_states(states, 5, 4, False), 5)])
        per_row = np.zeros(rows[b] + 1, dtype=np.int64)
        np.add.at(per_row, move_row[b, :n].cpu().numpy() + 1, letters)
        centers.append(np.maximum(np.cumsum(per_row) - 4, 0))
        assert centers[b][-1] == len(calls[b]) - 4 and len(calls[b]) - 4 > 10
    bits = lambda t: t.cpu().numpy().tobytes()                    # noqa: E731  (a random network's own call has more k-mers than
    #                                                               its read has rows: -inf and NaN must agree as well)
    want = polish.rescore_drafts(post, calls, 5, blank=0, min_prob=bc.min_prob, lengths=steps, band=(centers, 256))
    for r, w in zip(res, want):
        assert r.edits == w.edits and bits(r.gain) == bits(w.gain) and bits(r.score) == bits(w.score)
    got = bc.polish_reads(reads, width=256, max_rounds=2)
    want = polish.polish(post, calls, 5, blank=0, min_prob=bc.min_prob, lengths=steps, band=(centers, 256), max_rounds=2)
    assert [tuple(g) for g in got] == [tuple(w) for w in want]
    same_again = bc.rescore_reads(reads, drafts=calls, center=centers, width=256)
    assert all(bits(a.gain) == bits(b.gain) for a, b in zip(same_again, res))
    # given drafts that the reads' rows can emit: a stretch of each call, the centre a straight line, or the remap's path
    drafts = [calls[0][:124], calls[1][10:94]]
    lines = [np.round(np.linspace(0, len(d) - 4, int(r) + 1)).astype(np.int64) for d, r in zip(drafts, rows)]
    res = bc.rescore_reads(reads, drafts=drafts, center=lines, width=256)
    want = polish.rescore_drafts(post, drafts, 5, blank=0, min_prob=bc.min_prob, lengths=steps, band=(lines, 256))
    for r, w in zip(res, want):
        assert r.edits == w.edits and torch.equal(r.gain, w.gain) and torch.equal(r.score, w.score)
        assert bool(torch.isfinite(r.score)) and bool(torch.isfinite(r.gain).all())
    got = bc.polish_reads(reads, drafts=drafts, center=lines, width=256, max_rounds=2)
    want = polish.polish(post, drafts, 5, blank=0, min_prob=bc.min_prob, lengths=steps, band=(lines, 256), max_rounds=2)
    assert [tuple(g) for g in got] == [tuple(w) for w in want]
    for g, r in zip(got, res):
        print("read %s: %d letters, %d edits in %d rounds, score %.6f -> %.6f" % (g.name, len(r.draft), len(g.applied), g.rounds,
                                                                                   float(r.score), g.score))
        assert math.isfinite(g.score)
    remapped = bc.rescore_reads(reads, drafts=drafts, center="remap", width=256)
    assert all(bool(torch.isfinite(r.score)) for r in remapped)
    # (W = 256 holds every state of these drafts: any valid centre line gives the band of all zeros, and the same bits)
    assert all(torch.equal(a.gain, b.gain) for a, b in zip(remapped, res))
    with pytest.raises(ValueError):
        bc.rescore_reads(reads, drafts=calls, width=256)
    with pytest.raises(ValueError):
        bc.rescore_reads(reads, drafts=calls[:1], center=centers[:1], width=256)
    with pytest.raises(NotImplementedError):
        bc2 = pipeline.Basecaller(net, kmer_len=5, skip=0.0)
        bc2.transducer = False
        bc2.rescore_reads(reads)


def test_read_bands_follow_a_planted_call():
    """Basecaller._read_bands, which rescore_reads / polish_reads take their drafts and centre lines from, on a planted posterior of
    two reads (900 and 700 rows, 400 5-mers: more states than the band of 256 holds, fewer than the rows): the call is the planted
    string, the centre from the call's moves IS the planted path's (an off-by-k centre or a wrong letter count would not be), the
    remap's centre follows it, and the banded scores under either are finite and, the band lying round the path, the dense score
    within the bound."""
    need_gpu()
    import torch
    from sloika_amd import decode, models, pipeline, polish
    rng = np.random.default_rng(113)
    k, S, L = 5, 1025, 400
    text = ''.join('ACGT'[i] for i in rng.integers(0, 4, size=L + k - 1))
    states = np.array(rr.states_of(text, k))
    assert (states[1:] != states[:-1]).all()
    nrow = [900, 700]
    post = np.zeros((max(nrow), 2, S), dtype=np.float32)
    post[:, :, 0] = 1.0                                           # (rows no read owns)
    planted = []
    for b, T in enumerate(nrow):
        p = 0.02 * rng.uniform(size=(T, S))
        # (the decoder is in SOME state from the first row on: the planted path enters its first state there)
        rows = np.concatenate([[0], 1 + np.sort(rng.choice(T - 1, size=L - 1, replace=False))])
        p[:, 0] += 1.0
        p[rows, 0] -= 1.0
        p[rows, states + 1] += 1.0
        post[:T, b] = (p / p.sum(axis=1, keepdims=True)).astype(np.float32)
        planted.append(rb.center_from_rows(rows, T))
    bc = pipeline.Basecaller(models.build_model("raw_0.98_rgrgr", klen=k, sd=0.5, seed=7), kmer_len=k, skip=0.0)
    pd, steps = dev(post), dev(np.array(nrow, dtype=np.int32))
    drafts, centers = bc._read_bands(pd, steps, None, None, 5.0)
    assert drafts == [text, text]
    for c, want in zip(centers, planted):
        assert np.array_equal(c.cpu().numpy(), want)
    again, remap = bc._read_bands(pd, steps, drafts, "remap", 5.0)
    assert again == drafts
    for c, want in zip(remap, planted):
        c = c.cpu().numpy()
        assert len(c) == len(want) and c[0] == 0 and np.abs(c - want).max() <= 2
    dense = polish.rescore_drafts(pd, drafts, k, blank=0, min_prob=bc.min_prob, lengths=steps, kinds=())
    for cen in (centers, remap):
        lo = decode.band_lo(cen[0], L, 256).cpu().numpy()
        assert lo.max() == L + 1 - 256 and (np.diff(lo) > 0).sum() > 100          # the band moves with the call
        res = polish.rescore_drafts(pd, drafts, k, blank=0, min_prob=bc.min_prob, lengths=steps, band=(cen, 256))
        for r, d in zip(res, dense):
            s, ds = float(r.score), float(d.score)
            assert math.isfinite(s) and s <= ds + 4 * E_REF * abs(ds) and abs(s - ds) <= 8 * E_REF * abs(ds)
            assert bool(torch.isfinite(r.gain).all()) and not bool((r.gain > 0).any())


def test_shift_center_and_band_helpers():
    need_gpu()
    import torch
    from sloika_amd import decode
    rng = np.random.default_rng(5)
    center = np.sort(rng.integers(0, 900, size=400))
    edits = [(100, 1, 0), (500, 0, 1), (300, 2, 5), (899, 1, 1)]
    got = decode.shift_center(center, edits).cpu().numpy()
    assert np.array_equal(got, rb.shift_center(center, edits))
    for width in (256, 512):
        c = np.concatenate([[0], center, [900]])
        assert np.array_equal(decode.band_lo(c, 900, width).cpu().numpy(), rb.band_lo(c, 900, width))
    with pytest.raises(ValueError):
        decode.band_lo(center + 300, 900, 256)                    # does not begin at the sequence's start
    with pytest.raises(ValueError):
        decode.band_lo(np.minimum(center, 300), 900, 256)         # does not reach its end
    path = torch.as_tensor(center)
    assert np.array_equal(decode.band_center_from_path(path).cpu().numpy(), np.concatenate([[0], center + 1]))
    # moves: 5 k-mers entered at rows 2, 3, 7, 7 (a row cannot be entered twice: 8), 11 of 12, k = 3, the first emits 3 letters
    cen = decode.band_center_from_moves([2, 3, 7, 8, 11], [3, 1, 2, 0, 1], 12, 3).cpu().numpy()
    assert list(cen) == [0, 0, 0, 1, 2, 2, 2, 2, 4, 4, 4, 4, 5]


# ---- 6: refusals -------------------------------------------------------------------------------------------------------------------

def test_refused_bands(mixed):
    need_gpu()
    post, seq, edits, lo = mixed[2]
    good = mixed[0]
    T, L = post.shape[0], len(seq)
    bad = {}
    bad["decreasing"] = lo.copy()
    bad["decreasing"][T // 2] = lo[T // 2 - 1] - 1
    bad["first"] = np.maximum(lo, 1)
    bad["negative"] = lo.copy()
    bad["negative"][0] = -1
    bad["short"] = np.minimum(lo, L - 256)
    want = run_mixed([good])
    for name, v in bad.items():
        assert not rb.valid_band(v, T, L, 256), name
        with pytest.raises(ValueError):
            run_band([post], [seq], [edits], [v], 256)
        cands = [(0,) + e for e in good[2][:4]] + [(1,) + e for e in edits[:4]]
        rc, score, ll, _ = raw_band([good[0], post], [good[1], seq], cands, [good[3], v], 256)
        assert rc == 0, name
        assert same(score[:1], want[0]) and same(ll[:4], want[1][0][:4]), name
        assert np.isnan(score[1]) and np.isnan(ll[4:]).all(), name
    # a symbol that is no column: NaN for the pair, as the dense entry
    broken = seq.copy()
    broken[L - 1] = 65
    rc, score, ll, _ = raw_band([post], [broken], [(0,) + e for e in edits[:4]], [lo], 256)
    assert rc == 0 and np.isnan(score).all() and np.isnan(ll).all()


def test_entry_refusals(mixed):
    need_gpu()
    from sloika_amd import _lib, decode
    post, seq, edits, lo = mixed[0]
    cands = [(0,) + e for e in edits[:3]]
    top = _lib.lib().slk_rescore_band_max_width()
    assert top in rb.WIDTHS and decode.band_widths() == tuple(w for w in (256, 512, 1024, 2048, 4096, 8192) if w <= top)
    rc, score, ll, need = raw_band([post], [seq], cands, [lo], 256)
    assert rc == 0 and need == 256 + 16 * (post.shape[0] + 1) * 257 and np.isfinite(score).all()
    for width in (300, 2 * top, 0, -256):
        rc, score, ll, _ = raw_band([post], [seq], cands, [lo], width)
        assert rc == _lib.SLK_ERR_INVALID_ARG and (score == SENTINEL).all() and (ll == SENTINEL).all(), width
        with pytest.raises(ValueError):
            run_band([post], [seq], [edits], [lo], width)
    rc, score, ll, _ = raw_band([post], [seq], cands, [lo], 256, ws_bytes=need - 1)
    assert rc == _lib.SLK_ERR_WORKSPACE and (score == SENTINEL).all() and (ll == SENTINEL).all()
    rc, score, ll, _ = raw_band([post], [seq], cands, [lo], 256, band_off=[0, len(lo) - 1])      # disagrees with nrow
    assert rc == _lib.SLK_ERR_INVALID_ARG and (score == SENTINEL).all() and (ll == SENTINEL).all()
    rc, score, ll, _ = raw_band([post, post], [seq, seq], [(1,) + edits[0], (0,) + edits[1]], [lo, lo], 256)      # pairs out of order
    assert rc == _lib.SLK_ERR_INVALID_ARG and (score == SENTINEL).all() and (ll == SENTINEL).all()
    for e in ((1, 1, [1] * 9), (len(seq), 1, [1]), (-1, 0, [1]), (1, 1, [65])):
        with pytest.raises(ValueError):
            run_band([post], [seq], [[e]], [lo], 256)
