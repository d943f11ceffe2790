"""The sequence loss of the training step (sloika_amd/train.py SequenceTrainingStep, csrc/seq_loss.hip; design/sequence_loss.md): the
kernel that turns the occupancies of forward-backward into d loss / d logits against the float64 formula and at its edges, and the
step against the float64 oracle of tests/sequence_loss_ref.py (oracle/oracle_train.py's passes around tests/forward_backward_ref.py)."""
import os

import numpy as np
import pytest

from tests import sequence_loss_ref as slr
from tests.gpu_util import need_gpu, dev, stream, assert_grads_close, nan_filled, Out, PATTERN, GUARD

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24


# ------------------------------------------------------------------------------------------------------------------ the kernel
def _stats(x):
    """[.., 2] = (max, 1 / sum exp(x - max)) of float32 logits, as slk_linear_rowstats_* writes them (the sum taken in float64)."""
    x64 = x.astype(np.float64)
    mx = x64.max(axis=-1, keepdims=True)
    inv = 1.0 / np.exp(x64 - mx).sum(axis=-1, keepdims=True)
    return np.ascontiguousarray(np.concatenate([mx, inv], axis=-1).astype(np.float32))


def _seq_grad(logits_ptr, ld, stats, occ_ptr, occ_ld, score, scale, T, B, nstate, min_prob):
    from sloika_amd import _lib
    return _lib.lib().slk_softmax_seq_grad_f32(logits_ptr, ld, stats.data_ptr(), occ_ptr, occ_ld, score.data_ptr(), scale.data_ptr(), T, B,
                                               nstate, min_prob, stream())


@pytest.mark.parametrize("T,B,nstate,ld,occ_ld", [(7, 3, 5, 32, 5), (33, 2, 65, 96, 65), (19, 5, 1025, 1056, 1032), (3, 1, 2049, 2049, 2049)])
@pytest.mark.parametrize("min_prob", [0.0, 1e-5, 1e-3])
def test_kernel_vs_float64_formula(T, B, nstate, ld, occ_ld, min_prob):
    """Per entry within 64 * 2^-24 * c_b of -c_b * logits_grad on the kernel's own float32 inputs widened to float64: every term is at
    most c_b, W sums non-negative terms of total <= 1 through a tree, and p from a float32 exp of x - max is off by a few 2^-24 at most
    whatever the column."""
    torch = need_gpu()
    from sloika_amd import _lib, decode
    rs = np.random.RandomState(T + nstate)
    x = (2.0 * rs.normal(size=(T, B, nstate))).astype(np.float32)
    stats = _stats(x)
    logits = nan_filled((T, B, ld))
    logits[:, :, :nstate] = x
    # occ: the device's own forward-backward on the softmax of these logits, rows occ_ld apart
    post = nan_filled((T, B, occ_ld))
    post[:, :, :nstate] = slr.softmax(x).astype(np.float32)
    seqs = [rs.randint(1, nstate, size=rs.randint(0, T // 2 + 1)) for _ in range(B)]
    post_d = dev(post)
    score, occ, _, _ = decode.forwards_backwards_batch(post_d[:, :, :nstate], seqs, full=True, blank=0, min_prob=min_prob, positions=False)
    assert occ.stride(1) == occ_ld and bool(torch.isfinite(score).all())
    scale = rs.uniform(0.5, 1.5, size=B).astype(np.float32) / np.float32(T * B)
    logits_d, stats_d, scale_d = dev(logits), dev(stats.reshape(-1, 2)), dev(scale)
    _lib.check(_seq_grad(logits_d.data_ptr(), ld, stats_d, occ.data_ptr(), occ_ld, score, scale_d, T, B, nstate, min_prob), "seq_grad")
    got = logits_d.cpu().numpy()
    occ_h = occ.cpu().numpy()
    assert np.abs(occ_h.sum(axis=2) - 1.0).max() < 1e-4
    want = -scale.astype(np.float64)[None, :, None] * slr.logits_grad(x, occ_h, float(np.float32(min_prob)))
    err = np.abs(got[:, :, :nstate].astype(np.float64) - want) / (EPS * scale.astype(np.float64)[None, :, None])
    print("seq_grad %s min_prob %g: largest error %.2f x 2^-24 c_b" % ((T, B, nstate, ld, occ_ld), min_prob, err.max()))
    assert err.max() <= 64.0
    assert (got[:, :, nstate:].view(np.uint32) == 0).all()


@pytest.mark.parametrize("nstate,ld,occ_ld,lead", [(5, 8, 8, 0), (5, 7, 6, 1), (70, 72, 70, 0)])
def test_kernel_edges(nstate, ld, occ_ld, lead):
    """Padding columns zeroed, nothing else written; chunks whose score is NaN or -inf become exact zeros whatever their occ holds and
    leave the others' bits alone; a zero occ row gives a zero row; an underflowing p with occ = 0 at min_prob = 0 stays finite; every
    chunk alone has the bits it has in the batch.  (16-byte accesses, four-byte ones off a 16-byte boundary, and one of each.)"""
    need_gpu()
    from sloika_amd import _lib
    T, B = 4, 3
    rs = np.random.RandomState(nstate + ld)
    x = (2.0 * rs.normal(size=(T, B, nstate))).astype(np.float32)
    x[1, 0, 3] = x[1, 0].max() - np.float32(200.0)                  # exp underflows: p = p' = 0 at min_prob = 0
    occ = rs.uniform(size=(T, B, nstate)) * (rs.uniform(size=(T, B, nstate)) < 0.5)
    occ[:, :, 0] += 0.1
    occ[1, 0, 3] = 0.0
    occ = (occ / occ.sum(axis=2, keepdims=True)).astype(np.float32)
    occ[2, 0, :] = 0.0                                              # the degenerate z_t
    scale = (rs.uniform(0.5, 1.5, size=B) / (T * B)).astype(np.float32)
    stats = _stats(x)

    def run(xs, occs, score, scales, stat):
        nb = xs.shape[1]
        out = Out(T, nb, ld, lead=lead)
        body = nan_filled((T, nb, ld))
        body[:, :, :nstate] = xs
        host = out.buf.cpu().numpy()
        a = GUARD + lead
        host[a:a + body.size] = body.reshape(-1)
        out.buf.copy_(dev(host))
        ob = nan_filled((T, nb, occ_ld))
        ob[:, :, :nstate] = occs
        ob_d = dev(np.concatenate([nan_filled(lead), ob.reshape(-1)]))
        rc = _seq_grad(out.ptr(), ld, dev(np.ascontiguousarray(stat).reshape(-1, 2)), ob_d.data_ptr() + 4 * lead, occ_ld,
                       dev(np.asarray(score, np.float64)), dev(scales), T, nb, nstate, 0.0)
        _lib.check(rc, "seq_grad")
        out.fetch()
        out.assert_untouched_outside(None, "seq_grad")
        return out.body().copy()                                    # uint32 bits [T, nb, ld]

    base = run(x, occ, np.zeros(B), scale, stats)
    assert (base[:, :, nstate:] == 0).all()                          # exactly +0 behind the states
    vals = base[:, :, :nstate].view(np.float32)
    assert np.isfinite(vals).all() and (vals[2, 0] == 0).all() and np.isfinite(vals[1, 0, 3])
    want = -scale.astype(np.float64)[None, :, None] * slr.logits_grad(x, occ, 0.0)
    assert np.abs(vals - want).max() <= 64 * EPS * scale.max()
    for bad in (np.nan, -np.inf):
        score = np.zeros(B)
        score[1] = bad
        occ_bad = occ.copy()
        occ_bad[:, 1, :] = PATTERN.view(np.float32)
        got = run(x, occ_bad, score, scale, stats)
        assert (got[:, 1, :] == 0).all(), "an invalid chunk's rows must be exact zeros"
        assert np.array_equal(got[:, [0, 2]], base[:, [0, 2]])
    for b in range(B):
        alone = run(x[:, b:b + 1], occ[:, b:b + 1], np.zeros(1), scale[b:b + 1], stats[:, b:b + 1])
        assert np.array_equal(alone[:, 0], base[:, b]), "chunk %d alone" % b


def test_kernel_refusals():
    torch = need_gpu()
    from sloika_amd import _lib
    buf = torch.zeros(4096, dtype=torch.float32, device="cuda")
    sc = torch.zeros(4, dtype=torch.float64, device="cuda")
    p = buf.data_ptr()
    call = lambda ld, occ_ld, nstate, mp: _lib.lib().slk_softmax_seq_grad_f32(p, ld, p, p, occ_ld, sc.data_ptr(), p, 2, 2, nstate, mp, stream())
    bad, unsupported = _lib.SLK_ERR_INVALID_ARG, _lib.SLK_ERR_UNSUPPORTED
    assert call(8, 8, 1, 0.0) == bad and call(4, 8, 5, 0.0) == bad and call(8, 4, 5, 0.0) == bad
    assert call(8, 8, 5, 1.0) == bad and call(8, 8, 5, -0.1) == bad
    assert call((1 << 24) + 4, 8, 5, 0.0) == unsupported
    assert call(8, 8, 5, 0.0) == _lib.SLK_OK


# -------------------------------------------------------------------------------------------------------------------- the step
def _build(rs, n=32, nstate=17, winlen=5, stride=2, nlayer=3, conv=True, bias=True, scale=0.5):
    from sloika_amd import activation, layers
    init = lambda shape: (rs.normal(size=shape) * scale).astype(np.float32)
    subs = []
    if conv:
        subs.append(layers.Convolution(1, n, winlen, stride, init=init, has_bias=bias, fun=activation.elu))
    for l in range(nlayer):
        g = layers.Gru(n, n, init=init, has_bias=bias, fun=activation.tanh)
        subs.append(layers.Reverse(g) if l % 2 == 0 else g)
    subs.append(layers.Softmax(n, nstate, init=init, has_bias=bias))
    return layers.Serial(subs)


def _batch(rs, net, T, B, nfeat=1):
    """x, a label matrix with about 60 % blanks whose chunk 0 is all blank and chunk 1 has no blank, per-label weights."""
    x = rs.normal(size=(T, B, nfeat)).astype(np.float32)
    first = net.layers[0]
    To = first.out_len(T) if hasattr(first, "out_len") else T
    labels = (rs.randint(1, net.size, size=(To, B)) * (rs.uniform(size=(To, B)) > 0.6)).astype(np.int32)
    labels[:, 0] = 0
    labels[:, 1] = rs.randint(1, net.size, size=To)
    weights = rs.uniform(0.5, 1.5, size=(To, B)).astype(np.float32)
    return x, labels, weights


def _spec(net, bias=True):
    spec = net.spec()
    for sub in [spec] + spec["sublayers"] + [s.get("sublayer", {}) for s in spec["sublayers"]]:
        if not bias and "b" in sub:
            sub["b"] = None                          # the oracle returns gradients for the parameters that exist
    return spec


def _cols(labels):
    return [col[col != 0].astype(np.int64) for col in labels.T]


def _net(n, nstate, seed, bias=True):
    return _build(np.random.RandomState(seed), n=n, nstate=nstate, stride=5 if n == 96 else 2, winlen=11 if n == 96 else 5,
                  nlayer=5 if n == 96 else 3, bias=bias)


@pytest.mark.parametrize("n,nstate,T,B,min_prob,l2,bias,wkind", [
    (32, 17, 61, 5, 0.0, 0.0, True, "none"),
    (32, 17, 40, 3, 1e-3, 0.01, True, "chunk"),
    (16, 5, 24, 2, 1e-30, 0.0, False, "label"),
    (96, 1025, 75, 4, 1e-30, 0.0, True, "none"),       # the shapes of models/raw_0.98_rgrgr.py
])
def test_loss_and_gradients_vs_oracle(n, nstate, T, B, min_prob, l2, bias, wkind):
    need_gpu()
    from sloika_amd import train
    net = _net(n, nstate, n + T, bias)
    x, labels, wl = _batch(np.random.RandomState(n + T + 1), net, T, B)
    weights = {"none": None, "chunk": wl[0].copy(), "label": wl}[wkind]
    w_ref = {"none": None, "chunk": wl[0].astype(np.float64), "label": wl.astype(np.float64).mean(axis=0)}[wkind]
    want_loss, want_acc, want = slr.loss_and_grads(_spec(net, bias), x, _cols(labels), w_ref, min_prob, l2, True)
    assert want_acc == 1.0
    step = train.SequenceTrainingStep(net, min_prob=min_prob, l2=l2, full=True)
    loss, accepted = step.forward_backward(x, labels, weights)
    print("sequence loss %r against the oracle's %r" % (loss, want_loss))
    assert accepted == 1.0
    assert loss == pytest.approx(want_loss, rel=2e-5)
    assert_grads_close(step.gradients(), want)


def test_one_alignment_is_the_cross_entropy_step():
    """Every chunk with as many positions as rows, unit weights, full: one alignment, and the two losses are the same function."""
    need_gpu()
    from sloika_amd import train
    n, nstate, T, B = 32, 17, 40, 3
    x, labels, _ = _batch(np.random.RandomState(2), _net(n, nstate, 1), T, B)
    labels = np.random.RandomState(3).randint(1, nstate, size=labels.shape).astype(np.int32)
    ce = train.TrainingStep(_net(n, nstate, 1), min_prob=1e-5, drop=0)
    want_loss, _ = ce.forward_backward(x, labels, np.ones(labels.shape, np.float32))
    sq = train.SequenceTrainingStep(_net(n, nstate, 1), min_prob=1e-5, full=True)
    loss, accepted = sq.forward_backward(x, labels, None)
    assert accepted == 1.0 and loss == pytest.approx(want_loss, rel=2e-5)
    assert_grads_close(sq.gradients(), [g.astype(np.float64) for g in ce.gradients()])


def test_unaccepted_chunk_adds_nothing():
    need_gpu()
    from sloika_amd import train
    n, nstate, T, B = 32, 17, 40, 4
    net = _net(n, nstate, 6)
    x, labels, wl = _batch(np.random.RandomState(7), net, T, B)
    To = labels.shape[0]
    cols = _cols(labels)
    cols[2] = np.random.RandomState(8).randint(1, nstate, size=To + 1)          # one position more than rows: no alignment under full
    w = wl[0].astype(np.float64)
    w0, cols0 = w.copy(), list(cols)
    w0[2], cols0[2] = 0.0, np.zeros(0, np.int64)
    want_loss, _, want = slr.loss_and_grads(_spec(net), x, cols0, w0, 1e-3, 0.0, True)
    step = train.SequenceTrainingStep(net, min_prob=1e-3, full=True)
    loss, accepted = step.forward_backward(x, cols, wl[0])
    got = step.gradients()
    assert accepted == (B - 1) / B
    assert np.isfinite(loss) and all(np.isfinite(g).all() for g in got)
    assert loss == pytest.approx(want_loss, rel=2e-5)
    assert_grads_close(got, want)


def test_evaluate_and_workspace_split(monkeypatch):
    """evaluate: the bits of forward_backward's loss, no gradient touched.  A workspace_limit that forces three forward-backward launches
    changes neither the loss nor the softmax bias's gradient (a column sum of d loss / d logits), bit for bit."""
    need_gpu()
    from sloika_amd import train, transducer
    n, nstate, T, B = 32, 17, 61, 5
    x, labels, wl = _batch(np.random.RandomState(10), _net(n, nstate, 9), T, B)
    step = train.SequenceTrainingStep(_net(n, nstate, 9), min_prob=1e-5, l2=0.01, full=True)
    loss, accepted = step.forward_backward(x, labels, wl)
    grads = [g.copy() for g in step.gradients()]
    ev = step.evaluate(x, labels, wl)
    assert ev == (loss, accepted)
    assert all(np.array_equal(a, b) for a, b in zip(grads, step.gradients()))
    # the workspace of a launch: 8 * 256 * ppt bytes per row of a pair (ppt = 1 here) and a table of offsets: two chunks per launch
    To = labels.shape[0]
    limit = 2 * (8 * 256 * To + 8) + 512
    runs = []
    cut = transducer.workspace_runs
    monkeypatch.setattr(transducer, "workspace_runs", lambda *a: (runs.append(cut(*a)), runs[-1])[1])
    split = train.SequenceTrainingStep(_net(n, nstate, 9), min_prob=1e-5, l2=0.01, full=True, workspace_limit=limit)
    loss2, accepted2 = split.forward_backward(x, labels, wl)
    assert runs == [[(0, 2), (2, 4), (4, 5)]]
    assert (loss2, accepted2) == (loss, accepted)
    assert np.array_equal(split.gradients()[-1], grads[-1])


def test_bad_input_raises_and_changes_nothing():
    torch = need_gpu()
    from sloika_amd import activation, layers, train
    n, nstate, T, B = 16, 5, 24, 2
    net = _net(n, nstate, 12)
    x, labels, wl = _batch(np.random.RandomState(13), net, T, B)
    step = train.SequenceTrainingStep(net, min_prob=1e-5)
    before = step.flat.clone()
    bad = labels.copy()
    bad[3, 1] = nstate
    with pytest.raises(ValueError):
        step(x, bad, wl, 1e-3)
    with pytest.raises(ValueError):
        step(x, [np.array([1, 0, 2]), np.array([3])], None, 1e-3)                 # a blank inside a list entry
    with pytest.raises(ValueError):
        step(x, [np.array([1, 2])], None, 1e-3)                                   # one sequence for two chunks
    assert torch.equal(step.flat, before)
    loss, accepted = step(x, labels, wl, 1e-3)                                    # ... and a good batch still trains
    assert np.isfinite(loss) and accepted == 1.0 and not torch.equal(step.flat, before)
    # no Softmax with a blank at the end: not a transducer model
    rs = np.random.RandomState(1)
    init = lambda shape: (rs.normal(size=shape) * 0.5).astype(np.float32)
    plain = layers.Serial([layers.Gru(1, n, init=init, has_bias=True), layers.FeedForward(n, nstate, init=init, has_bias=True, fun=activation.tanh)])
    with pytest.raises(NotImplementedError):
        train.SequenceTrainingStep(plain)
    with pytest.raises(ValueError, match="drop"):
        train.train_loop(net, {}, "unused", drop=20, loss="sequence")
    with pytest.raises(ValueError, match="transducer"):
        train.train_loop(net, {}, "unused", drop=0, transducer=False, loss="sequence")


def test_train_loop_learns_with_the_sequence_loss(tmp_path, monkeypatch):
    """The toy task of tests/test_gpu_train.py::test_train_loop_end_to_end (label = quantised local signal level, half of the positions
    blank) through train_loop(loss="sequence", drop=0) for as many iterations."""
    need_gpu()
    from sloika_amd import helpers, train
    rs = np.random.RandomState(3)
    n, clen, stride = 64, 200, 2
    level = rs.randint(1, 5, size=(n, clen // stride))
    chunks = (np.repeat(level, stride, axis=1).astype(np.float32) - 2.5 + 0.1 * rs.normal(size=(n, clen)))[:, :, None]
    labels = level.astype(np.int32)
    labels[:, 1::2] = 0
    chunks[:, 2::4, 0] += 3.0
    chunks[:, 3::4, 0] += 3.0
    path = os.path.join(str(tmp_path), "chunks.npz")
    np.savez(path, chunks=chunks.astype(np.float32), labels=labels, bad=np.zeros_like(labels, dtype='i1'),
             weights=np.ones(n, dtype=np.float32), kmer=np.int64(1), alphabet=np.bytes_(b"ACGT"))
    net = _build(np.random.RandomState(4), n=32, nstate=5, winlen=5, stride=stride, nlayer=2, scale=0.3)
    seen = []
    wrap = train.wrap_sequence_network

    def recording(*args, **kwargs):
        step = wrap(*args, **kwargs)

        class Recording(type(step)):
            def __call__(self, *a):
                seen.append(train.SequenceTrainingStep.__call__(self, *a))
                return seen[-1]

        step.__class__ = Recording
        return step

    monkeypatch.setattr(train, "wrap_sequence_network", recording)
    out = os.path.join(str(tmp_path), "run")
    fg = train.train_loop(net, train.load_chunk_file(path), out, niteration=200, batch_size=32, drop=0, adam=(4e-3, 0.9, 0.999),
                          save_every=100, seed=9, quiet=True, loss="sequence")
    assert isinstance(fg, train.SequenceTrainingStep) and len(seen) == 200
    first, last = np.mean([s[0] for s in seen[:10]]), np.mean([s[0] for s in seen[-10:]])
    print("sequence loss, mean of the first ten iterations %.4f, of the last ten %.4f" % (first, last))
    assert all(np.isfinite(s[0]) and s[1] == 1.0 for s in seen)      # full: a chunk's own labels always have an alignment
    assert last < first
    assert "model_final.pkl" in os.listdir(out)
    final = helpers.load_model(os.path.join(out, "model_final.pkl"))
    assert final.size == 5
