"""The sequence loss of a training step (design/sequence_loss.md) in plain numpy for this repository's tests: the chain rule from the
occupancies of forward-backward to the logits (design/forward_backward.md section 6), and the whole step on the float64 oracle of the
cross-entropy step (oracle/oracle_train.py: its forward pass and its reverse pass, imported, nothing of it changed).  Not a test."""
import numpy as np

from oracle import oracle_train as ot
from tests import forward_backward_ref as fbr


def softmax(x, dtype=np.float64):
    x = np.asarray(x).astype(dtype)
    e = np.exp(x - x.max(axis=-1, keepdims=True))
    return e / e.sum(axis=-1, keepdims=True)


def logits_grad(x, occ, min_prob, dtype=np.float64):
    """d ll / d x of a [..., nstate] block of logits whose rows have the occupancies `occ` under post' = min_prob + (1 - min_prob)
    softmax(x):  w = occ (1 - min_prob) p / p' (0 where occ is 0),  d ll / d x = w - p sum(w).  The loss of a chunk is -c ll."""
    p = softmax(x, dtype)
    occ = np.asarray(occ).astype(dtype)
    mp = dtype(min_prob)
    pp = mp + (1 - mp) * p
    with np.errstate(divide="ignore", invalid="ignore"):
        w = np.where(occ != 0, occ * ((1 - mp) * p / pp), 0)
    return w - p * w.sum(axis=-1, keepdims=True)


def loss_and_grads(spec, x, cols, w, min_prob=0.0, l2=0.0, full=True):
    """(loss, accepted, d loss / d params in network.params() order) of
        loss = l2 |params|^2 + sum_{b: ll_b finite} w_b (-ll_b) / (T' B)
    with ll_b the forward-backward score (blank = column 0) of cols[b] under min_prob + (1 - min_prob) y, y the network's output."""
    x = np.asarray(x, np.float64)
    y, tape = ot._forward(spec, x)
    T, B, _ = y.shape
    post = min_prob + (1.0 - min_prob) * y
    w = np.ones(B) if w is None else np.asarray(w, np.float64)
    params = ot.params_of(spec)
    loss = l2 * sum(float(np.sum(np.square(np.asarray(p, np.float64)))) for p in params)
    dy = np.zeros_like(y)
    accepted = 0
    for b in range(B):
        score, occ, _, _ = fbr.forwards_backwards(post[:, b], cols[b], full=full, blank=0)
        if not np.isfinite(score):
            continue
        accepted += 1
        c = w[b] / (T * B)
        loss += c * -float(score)
        with np.errstate(divide="ignore", invalid="ignore"):
            dy[:, b] = np.where(occ != 0, -c * (1.0 - min_prob) * occ / post[:, b], 0.0)
    _, grads = ot._backward(spec, tape, dy)
    grads = [g + 2.0 * l2 * np.asarray(p, np.float64) for g, p in zip(grads, params)]
    return float(loss), accepted / float(B), grads
