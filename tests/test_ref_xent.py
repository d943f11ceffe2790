"""tests/ref_xent.py on the CPU: the float64 head against the training oracle (oracle/oracle_train.py, itself pinned to the reference's
own automatic differentiation and to finite differences) on a one-layer Softmax network, so that it is no third opinion of unknown
standing; and the properties of the generated cases and of the float32 yardstick that tests/test_gpu_xent_head.py leans on."""
import numpy as np
import pytest

from oracle import oracle_train as ot
from tests import ref_xent as rx

MIN_PROBS = (0.0, 1e-30, 1e-5, 1e-3, 0.5)                 # what the GPU file runs
REGIME_SHAPES = ((12, 11, 5, 1025), (8, 16, 0, 192))      # (T, B, drop, N) of its regime cases
K_OF = {1025: 96, 192: 64}
SEED = 5


def _close(got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape
    assert np.abs(got - want).max() <= 1e-9 * np.abs(want).max(), float(np.abs(got - want).max() / np.abs(want).max())


@pytest.mark.parametrize("drop", [0, 2])
@pytest.mark.parametrize("min_prob", [0.0, 1e-30, 1e-3])
def test_head_from_x_vs_training_oracle(min_prob, drop):
    """dW = g^T x, db = sum_m g, the loss and the accuracy of a one-layer Softmax network: loss_and_grads / loss_only."""
    rs = np.random.RandomState(17 + drop)
    T, B, K, N = 9, 4, 6, 7
    x, W, b = rs.normal(size=(T, B, K)), rs.normal(size=(N, K)) * 0.8, rs.normal(size=N) * 0.5
    labels, weights = rs.randint(0, N, size=(T, B)), rs.uniform(0.5, 1.5, size=(T, B))
    weights[2, 1] = 0.0
    spec = {"type": "softmax", "W": W, "b": b}
    mp = float(np.float32(min_prob))                     # the head takes min_prob as the float32 the kernels receive
    h = rx.head_from_x_f64(x.reshape(T * B, K), W, b, labels.ravel(), weights.ravel(), T, B, drop, min_prob)
    loss, acc, grads = ot.loss_and_grads(spec, x, labels, weights, min_prob=mp, drop=drop)
    _close(h.g.T @ x.reshape(T * B, K), grads[0])
    _close(h.g.sum(axis=0), grads[1])
    assert h.loss.sum() == pytest.approx(loss, rel=1e-9) and h.flag.sum() == pytest.approx(acc, abs=1e-12)
    loss2, acc2 = ot.loss_only(spec, x, labels, weights, min_prob=mp, drop=drop)
    assert h.loss.sum() == pytest.approx(loss2, rel=1e-9) and h.flag.sum() == pytest.approx(acc2, abs=1e-12)
    # the pieces the GPU tests use on their own
    t = np.arange(T * B) // B
    counted = (t >= drop) & (t < T - drop)
    assert np.array_equal(h.w, np.where(counted, weights.ravel() / ((T - 2 * drop) * B), 0.0))
    assert not h.g[~counted].any() and not h.loss[~counted].any() and not h.flag[~counted].any() and not h.g[2 * B + 1].any()
    assert h.scale.shape == (T * B, N) and (h.scale >= np.abs(h.logits)).all()
    srt = np.sort(h.logits, axis=1)
    assert np.array_equal(h.gap, srt[:, -1] - srt[:, -2])
    ev_loss, ev_flag = rx.eval_f64(h.logits, labels.ravel(), N)
    h0 = rx.head_from_x_f64(x.reshape(T * B, K), W, b, labels.ravel(), np.ones(T * B), T, B, 0, 0.0)
    np.testing.assert_allclose(ev_loss, h0.loss * T * B, rtol=1e-12)
    assert ev_flag.dtype == np.int32 and np.array_equal(ev_flag, (h0.flag > 0).astype(np.int32))


@pytest.mark.parametrize("regime", rx.REGIMES)
def test_given_statistics_agree_with_the_logits_own(regime):
    """head_f64 on float32 logits with the exact maximum and the float64 inverse sum rounded to float32 -- what the in-place kernel is
    handed -- against the same logits' own float64 statistics: p moves by a factor within 2^-24 of 1, the gradient by at most twice
    that of w' (coef and p both carry it), flags not at all.  And those float32 logits against the float64 ones from x: the
    derivable 2 w' dl with dl = 2^-24 |l|."""
    T, B, drop, N = 12, 11, 2, 1025
    x, W, b, labels, weights, ties = rx.case_x(SEED, T, B, N, 96, regime, 1e-5, drop)
    h = rx.head_from_x_f64(x, W, b, labels, weights, T, B, drop, 1e-5, ties)
    l32 = h.logits.astype(np.float32)
    mx, inv = rx.stats_f64(l32)
    own = rx.head_f64(l32, mx, inv, labels, weights, T, B, N, drop, 1e-5)
    given = rx.head_f64(l32, l32.max(axis=1), inv.astype(np.float32), labels, weights, T, B, N, drop, 1e-5)
    assert np.array_equal(l32.max(axis=1).astype(np.float64), mx)
    assert rx.row_error(given.g, own.g, own.w).max() <= 2 * 2.0 ** -24
    assert rx.row_error(given.loss, own.loss, own.w).max() <= 2.0 ** -23
    assert np.array_equal(given.flag, own.flag)
    dl = 2.0 ** -24 * np.abs(h.logits).max(axis=1)
    assert (rx.row_error(own.g, h.g, h.w) <= 2 * dl + 1e-15).all()


def _conditions(l, labels, ref, min_prob, N):
    rows = np.arange(len(l))
    if min_prob == 0:
        assert (l.max(axis=1) - l[rows, labels]).max() <= rx.LABEL_GAP
    assert np.isfinite(ref.g).all() and np.isfinite(ref.loss).all() and np.isfinite(ref.flag).all()
    counted = ref.w > 0
    assert (ref.flag[counted] > 0).any() and (ref.flag[counted] == 0).any()
    assert (ref.w == 0).sum() > counted.sum() * 0.01 or len(l) < 100          # zero weights occur
    assert set(rx.special_labels(N)) <= set(labels.tolist())
    assert ((l == l.max(axis=1, keepdims=True)).sum(axis=1) >= 2).sum() >= 2 * len(rx.tie_pairs(N))    # the constructed ties


@pytest.mark.parametrize("min_prob", MIN_PROBS)
@pytest.mark.parametrize("regime", rx.REGIMES)
def test_generated_cases_meet_their_conditions(regime, min_prob):
    for T, B, drop, N in REGIME_SHAPES:
        l, labels, weights = rx.case(SEED, T, B, N, regime, min_prob, drop)
        assert l.dtype == np.float32 and labels.dtype == np.int32 and weights.dtype == np.float32
        mx, inv = rx.stats_f64(l)
        _conditions(l, labels, rx.head_f64(l, mx, inv.astype(np.float32), labels, weights, T, B, N, drop, min_prob), min_prob, N)
        if regime == "flat":
            assert (l == l[0, 0]).all()
        x, W, b, labels, weights, ties = rx.case_x(SEED, T, B, N, K_OF[N], regime, min_prob, drop)
        h = rx.head_from_x_f64(x, W, b, labels, weights, T, B, drop, min_prob, ties)
        _conditions(h.logits, labels, h, min_prob, N)
        for row, a, c in ties:                                   # the pair is on top of its two rows, by far
            assert h.logits[row, a] == h.logits[row, c] == h.mx[row] and labels[row] in (a, c)
            assert np.sort(h.logits[row])[-3] < h.mx[row] - 1.0
        if regime == "flat":                                     # every row an exact tie of all its columns: W is zero
            assert not W.any() and (h.logits == h.logits[0, 0]).all()
        else:
            keep = np.setdiff1d(np.arange(N), [c for _, _, c in ties])
            assert (rx.top_two_gap(h.logits[:, keep]) > 1e-4).mean() >= 0.9


def test_tie_pairs_and_special_labels():
    assert rx.tie_pairs(1) == [] and rx.tie_pairs(5) == [(1, 2), (3, 4)]
    assert rx.tie_pairs(1025) == [(1, 2), (3, 4), (31, 32), (6, 70)]          # the partial tile is one column wide
    assert rx.tie_pairs(92) == [(1, 2), (3, 4), (31, 32), (6, 70), (64, 91)]
    assert rx.tie_pairs(128) == [(1, 2), (3, 4), (31, 32), (6, 70), (64, 127)]
    assert rx.tie_pairs(2047)[-1] == (1984, 2046)
    assert rx.special_labels(1025) == [0, 3, 4, 31, 32, 1024] and rx.special_labels(92) == [0, 3, 4, 31, 32, 64, 91]
    assert rx.special_labels(1) == [0]


@pytest.mark.parametrize("min_prob", [0.0, 1e-30, 1e-5, 1e-3])
@pytest.mark.parametrize("regime", rx.REGIMES)
def test_yardstick_figures(regime, min_prob):
    """head_f32 against head_f64 at (T, B, N) = (12, 11, 1025), drop = 2, in units of w': the case's largest gradient error 5e-8 to
    9.2e-7, rows whose coefficient is vanishing (below 1e-6 of w': the label's posterior is far below min_prob) 5e-9 at the most;
    the loss rows 4.7e-7 to 6.9e-6 of w' and at most 1.3e-7 of the case's largest row loss -- each within a factor 2."""
    T, B, N, drop = 12, 11, 1025, 2
    l, labels, weights = rx.case(SEED, T, B, N, regime, min_prob, drop)
    mx, inv = l.max(axis=1), rx.stats_f64(l)[1].astype(np.float32)
    r64 = rx.head_f64(l, mx, inv, labels, weights, T, B, N, drop, min_prob)
    r32 = rx.head_f32(l, mx, inv, labels, weights, T, B, N, drop, min_prob)
    assert r32.g.dtype == np.float32 and np.array_equal(r32.flag, r64.flag.astype(np.float32))
    eg, el = rx.row_error(r32.g, r64.g, r64.w), rx.row_error(r32.loss, r64.loss, r64.w)
    print("%s min_prob %g: gradient %.2e, loss %.2e of w'" % (regime, min_prob, eg.max(), el.max()))
    assert 5e-8 / 2 <= eg.max() <= 9.2e-7 * 2
    assert 4.7e-7 / 2 <= el.max() <= 6.9e-6 * 2
    assert np.abs(r32.loss - r64.loss).max() <= 2 * 1.3e-7 * r64.loss.max()
    p_lab = np.exp(l[np.arange(T * B), labels].astype(np.float64) - mx) * inv
    mp = float(np.float32(min_prob))
    vanishing = (1 - mp) * p_lab < 1e-6 * (mp + (1 - mp) * p_lab)
    assert eg[vanishing].max(initial=0.0) <= 2 * 5e-9
    if min_prob >= 1e-5 and regime in ("peaked", "wide"):
        assert vanishing.sum() > 10
