"""The forward score on the device (csrc/forward_score.hip through decode.forwards / forwards_batch and
pipeline.Basecaller.score_chunks; design/forward_score.md).

Accuracy is measured against tests/golden/forward.npz: per entry the reference's own score and an extended-precision value of the
same recursion (make_forward_goldens.py).  The yardstick is E_ref, the reference's largest distance from the extended value over
the fixture; the device may be 4 x E_ref away from it (it sums in another tree, uses another log and scales one row late: the
allowance design/olddecode.md gives a float64 score).  Everything else is bit equality or exact structure."""
import os
import sys

import numpy as np
import pytest

from tests.conftest import GOLDEN
from tests.gpu_util import need_gpu, dev

sys.path.insert(0, GOLDEN)
import forward_cases as fc                               # noqa: E402

from tests import forward_ref                            # noqa: E402

pytestmark = pytest.mark.gpu

ALLOW = 4.0
NAN32 = np.float32(np.nan)


@pytest.fixture(scope="module")
def fixture():
    return dict(np.load(os.path.join(GOLDEN, "forward.npz")))


@pytest.fixture(scope="module")
def inputs(fixture, golden_decode):
    out = {}
    for name in fc.NAMES:
        post, seq = fc.build(name, golden_decode)
        assert fc.digest(post, seq) == str(fixture[name + "/sha256"]), "regenerated input differs from the one the reference saw: " + name
        out[name] = (post, seq)
    return out


def bits(t):
    return t.detach().cpu().numpy().view(np.int64)


def ragged_pairs():
    """Seven float32 pairs over 65 states with different row counts and lengths: no positions, one row, a wave's and the workgroup's
    edge, two and four states per thread."""
    shapes = [(1, 1), (40, 0), (300, 254), (600, 256), (200, 64), (77, 30), (50, 700)]
    return [(fc.make_post(900 + i, T, 65, "float32"), fc.make_seq(900 + i, 65, L, "random")) for i, (T, L) in enumerate(shapes)]


def network_layout(pairs, pad=0):
    """[Tmax, B, S + pad] with NaN in every pad column and in every row past a pair's own, and the int32 lengths."""
    S = pairs[0][0].shape[1]
    tmax = max(p.shape[0] for p, _ in pairs)
    x = np.full((tmax, len(pairs), S + pad), NAN32, dtype=np.float32)
    for b, (p, _) in enumerate(pairs):
        x[:p.shape[0], b, :S] = p
    return x, np.array([p.shape[0] for p, _ in pairs], dtype=np.int32)


def packed_layout(pairs):
    rows = np.concatenate([p for p, _ in pairs])
    off = np.concatenate([[0], np.cumsum([p.shape[0] for p, _ in pairs])]).astype(np.int64)
    return rows, off


def test_against_the_fixture(fixture, inputs):
    """|dev - truth| / max(1, |truth|) <= 4 E_ref for every entry; the pairs of one width and dtype share a launch."""
    need_gpu()
    from sloika_amd import decode
    e_ref = float(fixture["E_ref"])
    got = {}
    groups = {}
    for name in fc.NAMES:
        c = fc.CASES[name]
        groups.setdefault((c["S"], c["dtype"]), []).append(name)
    for names in groups.values():
        pairs = [inputs[n] for n in names]
        rows, off = packed_layout(pairs)
        rows_d = dev(rows)
        for full in (False, True):
            sc = decode.forwards_batch(rows_d, [s for _, s in pairs], full=full, row_off=off).cpu().numpy()
            for n, v in zip(names, sc):
                got[(n, full)] = float(v)
    worst, where = 0.0, None
    fails = []
    for key, name, full in fc.entries():
        hi, lo = (float(v) for v in fixture[key + "/truth"])
        d = got[(name, full)]
        ratio = abs((d - hi) - lo) / max(1.0, abs(hi)) / e_ref
        print("%-22s dev %-24.16g ref %-24.16g |dev - truth| / E_ref %.3f" % (key, d, float(fixture[key + "/ref"]), ratio))
        if ratio > worst:
            worst, where = ratio, key
        if not ratio <= ALLOW:
            fails.append((key, d, hi, ratio))
    print("largest |dev - truth| / max(1, |truth|) = %.3f E_ref (E_ref %.3e) at %s" % (worst, e_ref, where))
    assert not fails, fails


def test_known_answers_through_the_reference_signatures(golden_decode, fixture):
    """score / forwards on the reference's float64 known answers, numpy in, numpy float64 out."""
    need_gpu()
    from sloika_amd import decode
    post, bases = golden_decode["kat_post"], golden_decode["kat_bases"]
    tol = ALLOW * float(fixture["E_ref"])
    for full, want in ((False, -4.4275354890527474), (True, -5.0702616325672301)):
        s = decode.score(post, bases, full=full)
        assert isinstance(s, np.float64) and s == decode.forwards(dev(post), bases, full=full)
        assert abs(s - want) / abs(want) <= tol + 2.0 ** -52, (s, want)


def test_pair_alone_in_a_batch_in_either_layout_and_twice():
    need_gpu()
    from sloika_amd import decode
    pairs = ragged_pairs()
    seqs = [s for _, s in pairs]
    net, lens = network_layout(pairs)
    rows, off = packed_layout(pairs)
    net_d, rows_d = dev(net), dev(rows)
    for full in (False, True):
        a = decode.forwards_batch(net_d, seqs, lengths=lens, full=full)
        a2 = decode.forwards_batch(net_d, seqs, lengths=dev(lens), full=full)            # lengths on the device, a second launch
        p = decode.forwards_batch(rows_d, seqs, full=full, row_off=off)
        alone = np.array([decode.forwards(post, seq, full=full) for post, seq in pairs])
        assert np.array_equal(bits(a), bits(a2)) and np.array_equal(bits(a), bits(p))
        assert np.array_equal(bits(a), alone.view(np.int64))
        # another batch: reversed order, and the four-states-per-thread pair left out (a launch with a smaller register budget)
        rev = decode.forwards_batch(rows_d, seqs[-2::-1], full=full, row_off=off[-3::-1], lengths=lens[-2::-1])
        assert np.array_equal(bits(rev), bits(a)[-2::-1])
        got = a.cpu().numpy()
        want = np.array([forward_ref.forwards(post, seq, full=full) for post, seq in pairs])
        assert np.array_equal(np.isfinite(got), np.isfinite(want))
        ok = np.isfinite(want)
        assert np.all(np.abs(got[ok] - want[ok]) <= 1e-12 * np.maximum(1.0, np.abs(want[ok])))     # (a sanity check, not the accuracy test)


def test_padding_is_never_read():
    """ld = S and ld = S + 3 with NaN in the pad columns and in the rows past nrow give the same bits."""
    need_gpu()
    from sloika_amd import decode
    pairs = ragged_pairs()
    seqs = [s for _, s in pairs]
    tight, lens = network_layout(pairs)
    wide, _ = network_layout(pairs, pad=3)
    wide_d = dev(wide)
    for full in (False, True):
        a = decode.forwards_batch(dev(tight), seqs, lengths=lens, full=full)
        b = decode.forwards_batch(wide_d[:, :, :65], seqs, lengths=lens, full=full)
        assert np.array_equal(bits(a), bits(b))
        assert not np.isnan(a.cpu().numpy()).any()


def test_blank_column():
    """blank last = blank at column 0 with every symbol shifted by one."""
    need_gpu()
    from sloika_amd import decode
    pairs = ragged_pairs()
    rows, off = packed_layout(pairs)
    rolled = np.roll(rows, 1, axis=1)
    for full in (False, True):
        a = decode.forwards_batch(dev(rows), [s for _, s in pairs], full=full, row_off=off)
        b = decode.forwards_batch(dev(rolled), [s + 1 for _, s in pairs], full=full, row_off=off, blank=0)
        assert np.array_equal(bits(a), bits(b))


def test_min_prob_is_prepare_post():
    """min_prob on the device = decode.prepare_post on the host side of the call, then min_prob=None."""
    need_gpu()
    from sloika_amd import decode
    pairs = ragged_pairs()
    rows, off = packed_layout(pairs)
    seqs = [s for _, s in pairs]
    rows_d = dev(rows)
    prepared = decode.prepare_post(rows_d[:, None, :], min_prob=1e-5)
    assert not np.array_equal(prepared.cpu().numpy(), rows)
    for full in (False, True):
        a = decode.forwards_batch(rows_d, seqs, full=full, row_off=off, min_prob=1e-5)
        b = decode.forwards_batch(prepared, seqs, full=full, row_off=off, min_prob=None)
        raw = decode.forwards_batch(rows_d, seqs, full=full, row_off=off)
        assert np.array_equal(bits(a), bits(b))
        assert not np.array_equal(bits(a), bits(raw))


def test_structure(fixture, golden_decode):
    need_gpu()
    from sloika_amd import decode
    tol = ALLOW * float(fixture["E_ref"])
    # more positions than rows: exactly -inf under `full`, finite without
    post = fc.make_post(31, 5, 9, "float32")
    seq = fc.make_seq(31, 9, 6, "random")
    assert decode.forwards(post, seq, full=True) == -np.inf
    assert np.isfinite(decode.forwards(post, seq, full=False))
    assert np.isfinite(decode.forwards(post, seq[:5], full=True))                    # L = T: one alignment
    # no positions: three uniform rows of four states, the reference's value in both modes
    uni = np.full((3, 4), 0.25)
    for full in (False, True):
        s = decode.forwards(uni, [], full=full)
        assert abs(s - -4.1588830833596715) <= tol * 4.1588830833596715, s
        assert decode.forwards(uni.astype(np.float32), np.zeros(0, dtype=np.int64), full=full) == s
    # the reference's ordering test (test/unit/test_decode.py): free >= full >= the best path's score
    kp, kb = golden_decode["kat_post"], golden_decode["kat_bases"]
    free, full = decode.score(kp, kb), decode.score(kp, kb, full=True)
    assert free >= full >= np.sum(np.log(kp.max(axis=1)))


def test_the_limit():
    """L = forward_max_positions() runs (three rows); one position more is refused, naming the limit."""
    need_gpu()
    from sloika_amd import decode
    limit = decode.forward_max_positions()
    post = fc.make_post(41, 3, 5, "float32")
    seq = fc.make_seq(41, 5, limit + 1, "random")
    got = decode.forwards(post, seq[:limit])
    want = forward_ref.forwards(post, seq[:limit])
    assert np.isfinite(got) and abs(got - want) <= 1e-12 * max(1.0, abs(want)), (got, want)
    assert decode.forwards(post, seq[:limit], full=True) == -np.inf
    with pytest.raises(ValueError, match=str(limit)):
        decode.forwards(post, seq)


def test_score_chunks_end_to_end(fixture):
    """Convolution + Gru + Softmax(65), k = 3, five chunks of 200 samples."""
    torch = need_gpu()
    from sloika_amd import activation, bio, decode, layers, pipeline
    rs = np.random.RandomState(12)
    init = lambda shape: (rs.normal(size=shape) * 0.3).astype(np.float32)            # noqa: E731
    net = layers.Serial([layers.Convolution(1, 48, 11, 5, init=init, has_bias=True, fun=activation.tanh),
                         layers.Gru(48, 64, init=init, has_bias=True, fun=activation.tanh),
                         layers.Softmax(64, 65, init=init, has_bias=True)])
    bc = pipeline.Basecaller(net, kmer_len=3)
    chunks = dev(pipeline.synthetic_chunks(5, chunk_len=200, seed=12))
    letters = ["".join("ACGT"[v] for v in rs.randint(0, 4, size=n)) for n in (3, 9, 14, 20, 11)]
    states = [np.array([bio.kmer_mapping(3)[k] for k in bio.seq_to_kmers(s, 3)]) for s in letters]
    post = bc.posteriors(chunks).clone()
    T = post.shape[0]
    assert post.shape == (T, 5, 65) and all(len(s) <= T // 2 for s in states)
    host = post.cpu().numpy()
    mp = bc.min_prob
    prepared = (np.float32(mp) + np.float32(1.0 - mp) * host).astype(np.float32)     # decode.py:36 in float32
    # the restatement is itself up to E_ref from the exact value, the device up to 4 E_ref
    tol = (ALLOW + 1.0) * float(fixture["E_ref"])
    for full in (True, False):
        by_states = bc.score_chunks(chunks, states, full=full).clone()
        by_letters = bc.score_chunks(chunks, letters, full=full).clone()
        direct = decode.forwards_batch(post, [s + 1 for s in states], full=full, blank=0, min_prob=mp)
        assert by_states.dtype == torch.float64 and by_states.is_cuda and by_states.shape == (5,)
        assert np.array_equal(bits(by_states), bits(direct)) and np.array_equal(bits(by_states), bits(by_letters))
        got = by_states.cpu().numpy()
        for b in range(5):
            want = forward_ref.forwards(prepared[:, b], states[b] + 1, full=full, blank=0)
            assert abs(got[b] - want) <= tol * max(1.0, abs(want)), (b, full, got[b], want)
    # a call scored against its own chunk
    scores, paths, lens = bc.call_chunks(chunks)
    paths, lens = paths.cpu().numpy(), lens.cpu().numpy()
    own = bc.score_chunks(chunks, [paths[b, :lens[b]] for b in range(5)]).cpu().numpy()
    assert np.isfinite(own).all() and (own < 0).all()
