"""The softmax cross-entropy head of the training step (train_network.py:128-136) and of a validation batch
(validate_network.py:46-54) as plain numpy: the float64 reference the GPU tests compare with (tests/test_gpu_xent_head.py), the same
formulas in float32 as the yardstick of what the arithmetic costs, and the generator of the cases.  tests/test_ref_xent.py ties the
float64 form to the training oracle (oracle/oracle_train.py) and asserts what the GPU tests take for granted about the cases.

Rows are (t, b) in time order, M = T * B of them.  The formulas are the block above softmax_xent_grad_kernel (csrc/train.hip):

    p = exp(l - mx) * inv ; post = min_prob + (1 - min_prob) p ; row loss = -w' log post[label]
    coef = w' (1 - min_prob) p[label] / post[label] ; g = coef (p - onehot) ; w' = w / ((T - 2 drop) B) on counted steps, else 0
    flag = 1 / count where the first column with l == mx is the label (T.argmax's rule), on counted steps

Errors are measured in units of the row's w' (row_error), not of the row's own largest gradient entry: where the label's posterior
underflows the coefficient is around 1e-40 of w' and the row's top entry is itself rounding noise."""
import collections

import numpy as np

REGIMES = ("moderate", "peaked", "flat", "wide")
SIGMA = {"moderate": 2.0, "peaked": 2.0, "flat": 0.0, "wide": 15.0}       # standard deviation of the logits
PEAK = 40.0                                                                # "peaked": added to one column per row
LABEL_GAP = 60.0                  # at min_prob == 0 no label lies further below its row's maximum (float32 exp underflows past ~87)
TILE = 64                         # columns per tile of the two-pass kernel (GH_BN, csrc/gemm_rows_f16x3.hip)

Head = collections.namedtuple("Head", "g loss flag w gap scale logits mx inv")
Head.__new__.__defaults__ = (None,) * 5


def _row_weights(weights, T, B, drop, dtype):
    t = np.arange(T * B) // B
    counted = (t >= drop) & (t < T - drop)
    count = dtype(T - 2 * drop) * dtype(B)
    return np.where(counted, np.asarray(weights, dtype) / count, dtype(0)).astype(dtype), counted, count


def _head(logits, mx, inv, labels, weights, T, B, nstate, drop, min_prob, dtype):
    f = dtype
    M = T * B
    l = np.asarray(logits)[:, :nstate].astype(f)
    mx, inv, min_prob = np.asarray(mx).astype(f), np.asarray(inv).astype(f), f(min_prob)
    labels = np.asarray(labels).astype(np.int64)
    rows = np.arange(M)
    w, counted, count = _row_weights(weights, T, B, drop, f)
    with np.errstate(under="ignore", divide="ignore", invalid="ignore"):
        p = np.exp(l - mx[:, None]) * inv[:, None]
        p_lab = p[rows, labels]
        post_lab = min_prob + (f(1) - min_prob) * p_lab
        loss = np.where(counted, -w * np.log(post_lab), f(0)).astype(f)
        coef = w * (f(1) - min_prob) * p_lab / post_lab
        onehot = np.zeros((M, nstate), f)
        onehot[rows, labels] = 1
        g = coef[:, None] * (p - onehot)
    at_max = l == mx[:, None]
    first = np.where(at_max.any(axis=1), at_max.argmax(axis=1), -1)
    flag = np.where(counted & (first == labels), f(1) / count, f(0)).astype(f)
    assert g.dtype == f and loss.dtype == f and flag.dtype == f and w.dtype == f
    return Head(g, loss, flag, w)


def head_f64(logits, mx, inv, labels, weights, T, B, nstate, drop, min_prob):
    """Gradient [M][nstate], loss rows, flag rows and w' in float64 from the logits, row maxima and inverse sums as given (float32
    values are taken as they are)."""
    return _head(logits, mx, inv, labels, weights, T, B, nstate, drop, np.float32(min_prob), np.float64)


def head_f32(logits, mx, inv, labels, weights, T, B, nstate, drop, min_prob):
    """head_f64 with every operation in float32: the yardstick."""
    return _head(logits, mx, inv, labels, weights, T, B, nstate, drop, min_prob, np.float32)


def stats_f64(logits):
    """Row maximum and 1 / sum exp(l - max) in float64."""
    l = np.asarray(logits, np.float64)
    mx = l.max(axis=1)
    with np.errstate(under="ignore"):
        return mx, 1.0 / np.exp(l - mx[:, None]).sum(axis=1)


def logits_f64(x, W, b, ties=()):
    """x W^T + b in float64 and |x| |W|^T + |b|; the columns of a duplicated pair get the same value to the last bit, as identical
    weight rows give in any one arithmetic."""
    x, W, b = (np.asarray(a, np.float64) for a in (x, W, b))
    l, scale = x @ W.T + b, np.abs(x) @ np.abs(W).T + np.abs(b)
    for _, a, c in ties:
        l[:, c] = l[:, a]
    return l, scale


def head_from_x_f64(x, W, b, labels, weights, T, B, drop, min_prob, ties=()):
    """The same from float64 logits x W^T + b with their own maximum and sum; also each row's gap between its two largest logits
    (inf for a single column), scale = |x| |W|^T + |b| per element, and the logits, maxima and inverse sums themselves."""
    l, scale = logits_f64(x, W, b, ties)
    mx, inv = stats_f64(l)
    h = head_f64(l, mx, inv, labels, weights, T, B, l.shape[1], drop, min_prob)
    return Head(h.g, h.loss, h.flag, h.w, top_two_gap(l), scale, l, mx, inv)


def top_two_gap(l):
    if l.shape[1] < 2:
        return np.full(l.shape[0], np.inf)
    top = np.partition(l, l.shape[1] - 2, axis=1)[:, -2:]
    return top[:, 1] - top[:, 0]


def _eval(logits, labels, nstate, mx, inv, dtype):
    l = np.asarray(logits)[:, :nstate].astype(dtype)
    if mx is None:
        mx, inv = stats_f64(l)
    mx, inv = np.asarray(mx).astype(dtype), np.asarray(inv).astype(dtype)
    labels = np.asarray(labels).astype(np.int64)
    with np.errstate(under="ignore", divide="ignore"):
        loss = -np.log(np.exp(l[np.arange(len(l)), labels] - mx) * inv)
    at_max = l == mx[:, None]
    first = np.where(at_max.any(axis=1), at_max.argmax(axis=1), -1)
    assert loss.dtype == dtype
    return loss, (first == labels).astype(np.int32)


def eval_f64(logits, labels, nstate, mx=None, inv=None):
    """The validation form: loss rows -log p[label], undivided, and an int32 flag per row.  Without (mx, inv) the statistics are the
    logits' own in float64."""
    return _eval(logits, labels, nstate, mx, inv, np.float64)


def eval_f32(logits, labels, nstate, mx, inv):
    return _eval(logits, labels, nstate, mx, inv, np.float32)


def row_error(got, ref, w):
    """Largest |got - ref| of each row in units of the row's w' (rows with w' == 0 give 0: they are checked to be exactly zero
    elsewhere).  got/ref: [M][n] or [M]."""
    d = np.abs(np.asarray(got, np.float64) - np.asarray(ref, np.float64))
    d = d.reshape(len(d), -1).max(axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(w > 0, d / w, 0.0)


# ------------------------------------------------------------------------------------------------------------- cases
def tie_pairs(N):
    """Column pairs (a, b), a < b, that are made to tie for a row's maximum: in the same group of four, across the lane-half seam
    (3/4), across the column-wave seam (31/32), in different tiles, and in the last partial tile (the whole last tile when N is a
    multiple of the tile).  Pairs share no column; those that N has no room for are left out."""
    last = (N // TILE) * TILE if N % TILE else N - TILE
    out, used = [], set()
    for a, b in ((1, 2), (3, 4), (31, 32), (6, TILE + 6), (max(last, 0), N - 1)):
        if 0 <= a < b < N and not {a, b} & used:
            out.append((a, b))
            used |= {a, b}
    return out


def special_labels(N):
    """Columns every case labels some row with: 0, N-1, 3/4, 31/32, the first column of the last partial tile."""
    cols = [0, N - 1, 3, 4, 31, 32] + ([(N // TILE) * TILE] if N % TILE else [])
    return sorted({c for c in cols if 0 <= c < N})


def _counted_rows(T, B, drop):
    return np.arange(drop * B, (T - drop) * B)


def _tie_rows(T, B, drop, N):
    """[(row, a, b)]: counted rows spread over the case, two per pair; `labels_for_ties` labels the first with a, the second with b."""
    rows, pairs = _counted_rows(T, B, drop), tie_pairs(N)
    want = [(a, b) for a, b in pairs for _ in (0, 1)]
    if not want:
        return []
    stride = max(1, len(rows) // (len(want) + 1))
    return [(int(rows[(k + 1) * stride - 1]), a, b) for k, (a, b) in enumerate(want) if (k + 1) * stride - 1 < len(rows)]


def _labels_weights(rs, T, B, N, drop, ties, argmax):
    M = T * B
    labels = rs.randint(0, N, size=M)
    special = special_labels(N)
    for m in range(M):
        if m % 3 == 0:
            labels[m] = special[(m // 3) % len(special)]
        elif m % 3 == 1:
            labels[m] = argmax[m]
    seen = collections.Counter()
    for row, a, b in ties:
        labels[row] = (a, b)[seen[(a, b)] % 2]
        seen[(a, b)] += 1
    weights = rs.uniform(0.5, 1.5, size=M).astype(np.float32)
    weights[rs.uniform(size=M) < 0.05] = 0.0
    return labels.astype(np.int32), weights


def case(seed, T, B, N, regime, min_prob, drop):
    """Float32 logits [M][N], labels and weights of one case on given logits (the module docstring of tests/test_gpu_xent_head.py
    says what the regimes are for).  At min_prob == 0 a label's logit further than LABEL_GAP below its row's maximum is raised to
    within it."""
    rs = np.random.RandomState(seed)
    M = T * B
    if regime == "flat":
        l = np.full((M, N), rs.normal() * 3.0)
    else:
        l = rs.normal(size=(M, N)) * SIGMA[regime]
        if regime == "peaked":
            l[np.arange(M), rs.randint(0, N, size=M)] += PEAK
    l = l.astype(np.float32)
    ties = _tie_rows(T, B, drop, N) if regime != "flat" else []       # a flat row IS a tie of all its columns
    for row, a, b in ties:
        l[row, a] = l[row, b] = l[row].max() + np.float32(1.5)
    labels, weights = _labels_weights(rs, T, B, N, drop, ties, l.argmax(axis=1))
    if min_prob == 0:
        rows = np.arange(M)
        mx = l.max(axis=1)
        far = mx - l[rows, labels] > LABEL_GAP - 5.0
        l[rows[far], labels[far]] = (mx[far] - rs.uniform(0.0, LABEL_GAP - 5.0, size=int(far.sum()))).astype(np.float32)
    return l, labels, weights


def case_x(seed, T, B, N, K, regime, min_prob, drop):
    """x [M][K], W [N][K], b [N] (float32), labels, weights and the tie rows [(row, a, b)] of one case from the layer's input.  Ties
    are duplicated weight rows and biases (W[b] = W[a] along one input feature of their own) that the two rows of the pair, which
    have that feature alone, put on top."""
    rs = np.random.RandomState(seed)
    M = T * B
    sigma = SIGMA[regime]
    x = rs.normal(size=(M, K))
    W = rs.normal(size=(N, K)) * sigma / np.sqrt(K)
    b = rs.normal(size=N) * 0.5 if regime != "flat" else np.full(N, rs.normal() * 3.0)
    if regime == "peaked":                                            # feature k >= 8 lifts a column of its own by 5 * 8
        cols, feat = rs.randint(0, N, size=K), rs.randint(8, K, size=M)   # (the first features are the tie pairs')
        W[cols[8:], np.arange(8, K)] += 8.0
        x[np.arange(M), feat] += 5.0
    ties = _tie_rows(T, B, drop, N) if regime != "flat" else []
    feature = {}
    for row, a, c in ties:
        k = feature.setdefault((a, c), len(feature))
        W[a] = 0.0
        W[a, k] = 1.5 * sigma
        W[c], b[c] = W[a], b[a]
        x[row] = 0.0
        x[row, k] = 4.0
    x, W, b = x.astype(np.float32), W.astype(np.float32), b.astype(np.float32)
    l, _ = logits_f64(x, W, b, ties)
    labels, weights = _labels_weights(rs, T, B, N, drop, ties, l.argmax(axis=1))
    if min_prob == 0:                                                 # labels too far down move onto a column that is not
        rows = np.arange(M)
        far = np.flatnonzero(l.max(axis=1) - l[rows, labels] > LABEL_GAP - 5.0)
        for m in far:
            near = np.flatnonzero(l[m].max() - l[m] <= LABEL_GAP - 5.0)
            labels[m] = near[rs.randint(len(near))]
    return x, W, b, labels, weights, ties
