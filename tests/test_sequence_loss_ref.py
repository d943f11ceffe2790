"""The numpy helper of the sequence-loss tests (tests/sequence_loss_ref.py) pinned without a GPU: its gradient by the logits is the
slope of the forward score (tests/forward_ref.py, extended precision) taken through a softmax and min_prob -- the scheme
tests/test_forward_backward_ref.py uses for the occupancies: central differences, step 1e-9, bound 1e-7.  (design/sequence_loss.md)"""
import numpy as np
import pytest

from tests import forward_backward_ref as fbr
from tests import forward_ref
from tests import sequence_loss_ref as slr

LD = np.longdouble


def _ll(x, seq, full, min_prob):
    post = LD(min_prob) + (1 - LD(min_prob)) * slr.softmax(x, LD)
    hi, lo = forward_ref.forwards_exact(post, seq, full=full, blank=0)
    return LD(hi) + LD(lo)


def _sequence(rs, S, L, kind):
    if kind == "empty":
        return np.zeros(0, dtype=np.int64)
    seq = rs.randint(1, S, size=L).astype(np.int64)             # never the blank, column 0
    if kind == "repeat":
        seq[L // 2:L // 2 + 3] = seq[L // 2]
    return seq


@pytest.mark.parametrize("T,S,L", [(12, 5, 6), (30, 65, 11)])
@pytest.mark.parametrize("min_prob", [0.0, 1e-3])
@pytest.mark.parametrize("full", [False, True])
@pytest.mark.parametrize("kind", ["random", "repeat", "empty"])
def test_logits_grad_is_the_slope_of_the_forward_score(T, S, L, min_prob, full, kind):
    assert np.finfo(LD).eps < 1e-18, "needs an extended long double"
    rs = np.random.RandomState(T + S + (7 if full else 0))
    x = (2.0 * rs.normal(size=(T, S))).astype(np.float64)
    seq = _sequence(rs, S, L, kind)
    post = LD(min_prob) + (1 - LD(min_prob)) * slr.softmax(x, LD)
    occ = fbr.forwards_backwards(post, seq, full=full, blank=0, dtype=LD)[1]
    got = slr.logits_grad(x, occ, min_prob, dtype=LD)
    assert float(np.abs(got.sum(axis=1)).max()) <= 1e-15                       # a gradient by the logits of a softmax: rows sum to 0
    h = LD(1e-9)
    worst = 0.0
    for t in (0, T // 2, T - 1):
        for c in range(S) if S <= 8 else (0, 1, int(seq[0]) if len(seq) else 2, S // 2, S - 1):
            up, down = x.astype(LD), x.astype(LD)
            up[t, c] += h
            down[t, c] -= h
            slope = (_ll(up, seq, full, min_prob) - _ll(down, seq, full, min_prob)) / (2 * h)
            d = float(abs(got[t, c] - slope))
            worst = max(worst, d)
            assert d <= 1e-7, (t, c, d)
    print("logits_grad against central differences of the forward score: largest difference %.3e" % worst)
    # float64 is what the GPU tests use
    occ64 = fbr.forwards_backwards(np.asarray(post, np.float64), seq, full=full, blank=0)[1]
    assert float(np.abs(slr.logits_grad(x, occ64, min_prob) - got).max()) <= 1e-13


@pytest.mark.parametrize("min_prob", [0.0, 1e-3])
def test_one_alignment_gives_the_cross_entropy_gradient(min_prob):
    """L = T under full: every row emits its own position, occ is one-hot, and -d ll / d x is the cross-entropy's gradient per row,
    (1 - min_prob) p_label / p'_label * (p - onehot) (csrc/train.hip, softmax_xent_grad_kernel) -- p - onehot at min_prob = 0."""
    T, S = 12, 5
    rs = np.random.RandomState(5)
    x = 2.0 * rs.normal(size=(T, S))
    seq = rs.randint(1, S, size=T)
    p = slr.softmax(x)
    post = min_prob + (1 - min_prob) * p
    score, occ, _, _ = fbr.forwards_backwards(post, seq, full=True, blank=0)
    onehot = np.zeros((T, S))
    onehot[np.arange(T), seq] = 1.0
    assert np.abs(occ - onehot).max() <= 1e-15
    assert score == pytest.approx(np.log(post[np.arange(T), seq]).sum(), rel=1e-12)
    coef = ((1 - min_prob) * p / post)[np.arange(T), seq][:, None]
    assert np.abs(-slr.logits_grad(x, occ, min_prob) - coef * (p - onehot)).max() <= 1e-14


def test_step_helper_on_one_softmax_layer():
    """loss_and_grads against central differences of its own loss, on a network that is one Softmax layer: an empty sequence, a
    repeated symbol, an unaccepted chunk (more positions than rows under full) that must add nothing."""
    rs = np.random.RandomState(11)
    T, B, n, S = 6, 3, 4, 5
    spec = {"type": "serial", "sublayers": [{"type": "softmax", "W": rs.normal(size=(S, n)), "b": rs.normal(size=S)}]}
    x = rs.normal(size=(T, B, n))
    cols = [np.zeros(0, np.int64), np.array([2, 2, 3]), rs.randint(1, S, size=T + 1)]
    w = np.array([0.7, 1.3, 1.1])
    loss, accepted, grads = slr.loss_and_grads(spec, x, cols, w, 1e-3, 0.01, True)
    assert accepted == pytest.approx(2.0 / 3.0)
    h = 1e-6
    for k, name in enumerate(("W", "b")):
        par = spec["sublayers"][0][name]
        for idx in [(1, 2), (4, 0)] if name == "W" else [(0,), (3,)]:
            keep = par[idx]
            par[idx] = keep + h
            up = slr.loss_and_grads(spec, x, cols, w, 1e-3, 0.01, True)[0]
            par[idx] = keep - h
            down = slr.loss_and_grads(spec, x, cols, w, 1e-3, 0.01, True)[0]
            par[idx] = keep
            assert grads[k][idx] == pytest.approx((up - down) / (2 * h), abs=1e-8)
