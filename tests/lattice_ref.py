"""numpy oracle of the lattice marginals (design/lattice_marginals.md), generic in dtype: the Viterbi of sloika/decode.py:39-93
with the row at which every position is entered, the sum-product pass over the same lattice, and the per-position confidence.

The lattice: N = nbase^klen states, column 0 of a row the blank.  Row 0 weighs state s with p[0][1+s]; a later row i is reached
from state q by a stay (s == q, weight p[i][0]), a step (s // nbase == q % (N / nbase), weight p[i][1+s]) or a skip
(s // nbase^2 == q % (N / nbase^2), weight e p[i][1+s], e = exp(-skip_pen)); a stay and a step into the same state are two paths.
"""
import numpy as np


def viterbi(lpost, klen, skip_pen=0.0, nbase=4):
    """decode.viterbi (decode.py:56-91) on LOG posteriors [T, N + 1], in their own dtype (float32 rows give the float32 recursion the
    device runs): first maximum for step, skip and the final argmax, a step/skip tie goes to skip, a move/stay tie to stay.
    -> (score, path, move_row): move_row[j] is the row at which the path enters path[j]; move_row[0] = 0."""
    lpost = np.asarray(lpost)
    dt = lpost.dtype.type
    nev, nst = lpost.shape
    assert klen >= 3
    nkmer = nbase ** klen
    assert nst == nkmer + 1
    nstep, nskip = nbase, nbase ** 2
    pen = dt(skip_pen)
    vscore = lpost[0][1:].copy()
    traceback = np.empty((nev, nkmer), dtype=np.int64)
    for i in range(1, nev):
        pscore = vscore.reshape(nstep, -1)
        nrem = pscore.shape[1]
        score_step = np.repeat(np.amax(pscore, axis=0), nstep)
        from_step = np.repeat(nrem * np.argmax(pscore, axis=0) + np.arange(nrem), nstep)
        pscore = pscore.reshape(nskip, -1)
        nrem = pscore.shape[1]
        score_skip = np.repeat(np.amax(pscore, axis=0), nskip) - pen
        from_skip = np.repeat(nrem * np.argmax(pscore, axis=0) + np.arange(nrem), nskip)
        moved = lpost[i][1:] + np.maximum(score_step, score_skip)
        tb = np.where(score_step > score_skip, from_step, from_skip)
        score_stay = pscore.reshape(-1) + lpost[i][0]
        traceback[i] = np.where(moved > score_stay, tb, -1)
        vscore = np.maximum(moved, score_stay)
    cur = int(np.argmax(vscore))
    path, rows = [cur], []
    for i in range(nev - 1, 0, -1):
        prev = int(traceback[i][cur])
        if prev >= 0:
            rows.append(i)
            path.append(prev)
            cur = prev
    rows.append(0)
    return np.amax(vscore), path[::-1], rows[::-1]


def _scale(x):
    """x / 2^e with e the binary exponent of its total: exact."""
    tot = x.sum()
    e = int(np.frexp(tot)[1]) if tot > 0 and np.isfinite(tot) else 0
    return np.ldexp(x, -e), e


def marginals(p, klen, skip_pen=0.0, nbase=4, dtype=np.float64):
    """The sum over every path of the lattice.  p: [T, N + 1] weights (prepare_post's float32 values), widened to `dtype`.
    -> (gamma [T, N] in dtype: the share of Z that passes through s at row i; log Z in dtype).  Rows are scaled by exact powers of two."""
    p = np.asarray(p).astype(dtype)
    T, nst = p.shape
    N = nbase ** klen
    assert nst == N + 1 and klen >= 3
    e = np.exp(-dtype(np.float32(skip_pen)))
    n1, n2 = nbase, nbase ** 2
    a = np.empty((T, N), dtype=dtype)
    ea = np.zeros(T, dtype=np.int64)                       # a[i] = alpha_i / 2^ea[i]
    a[0] = p[0, 1:]
    for i in range(1, T):
        prev = a[i - 1]
        step = np.repeat(prev.reshape(n1, -1).sum(axis=0), n1)
        skip = np.repeat(prev.reshape(n2, -1).sum(axis=0), n2)
        a[i], ex = _scale(prev * p[i, 0] + p[i, 1:] * (step + e * skip))
        ea[i] = ea[i - 1] + ex
    z = a[T - 1].sum()
    logz = np.log(z) + dtype(ea[T - 1]) * np.log(dtype(2))
    gamma = np.empty((T, N), dtype=dtype)
    b = np.ones(N, dtype=dtype)
    eb = 0                                                 # b = beta_i / 2^eb
    for i in range(T - 1, -1, -1):
        gamma[i] = np.ldexp(a[i] * b, int(ea[i] + eb - ea[T - 1])) / z
        if i > 0:
            w = p[i, 1:] * b
            g1 = np.tile(w.reshape(-1, n1).sum(axis=1), n1)             # the step successors of q: the states of group q % (N / nbase)
            g2 = np.tile(w.reshape(-1, n2).sum(axis=1), n2)
            b, ex = _scale(p[i, 0] * b + g1 + e * g2)
            eb += ex
    return gamma, logz


def confidence(gamma, path, move_row):
    """Per called position the largest gamma of its state over its dwell (rows move_row[j] .. move_row[j + 1] - 1, the last dwell up to
    the last row)."""
    T = gamma.shape[0]
    ends = list(move_row[1:]) + [T]
    return np.array([gamma[r0:r1, s].max() for s, r0, r1 in zip(path, move_row, ends)], dtype=gamma.dtype)


def enumerate_paths(p, klen, skip_pen=0.0, nbase=2, dtype=np.float64):
    """The same quantities from the weight of every state sequence on its own (N^T of them: tiny lattices only), the transitions written
    out one pair of states at a time.  -> (gamma [T, N], log Z)."""
    p = np.asarray(p).astype(dtype)
    T = p.shape[0]
    N = nbase ** klen
    e = np.exp(-dtype(np.float32(skip_pen)))
    weight = p[0, 1:].copy()                               # weight[s0, s1, ..]: the summed weight of the paths through that state sequence
    for i in range(1, T):
        W = np.zeros((N, N), dtype=dtype)
        for q in range(N):
            for s in range(N):
                if s == q:
                    W[q, s] += p[i, 0]
                if s // nbase == q % (N // nbase):
                    W[q, s] += p[i, 1 + s]
                if s // nbase ** 2 == q % (N // nbase ** 2):
                    W[q, s] += e * p[i, 1 + s]
        weight = weight[..., :, None] * W.reshape((1,) * (i - 1) + (N, N))
    z = weight.sum()
    gamma = np.stack([weight.sum(axis=tuple(k for k in range(T) if k != i)) for i in range(T)]) / z
    return gamma, np.log(z)
