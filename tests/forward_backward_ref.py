"""Forward-backward over the recursion of the forward score (tests/forward_ref.py; design/forward_backward.md), in plain numpy for
this repository's tests.  Not a test; nothing of the reference is imported or needed.

    f_0 = 1 (full: e_0)      f_t[j]     = f_{t-1}[j] p_t[blank] + f_{t-1}[j-1] p_t[seq[j-1]]
    b_T = 1 (full: e_L)      b_{t-1}[j] = b_t[j] p_t[blank] + b_t[j+1] p_t[seq[j]]
    stay_t[j] = f_{t-1}[j] p_t[blank] b_t[j]        move_t[j] = f_{t-1}[j-1] p_t[seq[j-1]] b_t[j]        z_t = sum stay + sum move
    occ[t, blank] += sum_j stay_t[j] / z_t          occ[t, seq[j-1]] += move_t[j] / z_t
    emit_prob[j-1] = max_t move_t[j] / z_t          emit_row[j-1] = the lowest t that attains it

Every row of f and of b is normalised by its own sum, as tests/forward_ref.py does; occ does not depend on that, because a row is
divided by its own z_t.  `dtype` is float64 or np.longdouble (the truth the tests measure against).
"""
import numpy as np


def forwards_backwards(post, seq, full=False, blank=-1, dtype=np.float64, gaps=False):
    """-> (score, occ [T, S], emit_row [L] int32, emit_prob [L]), all in `dtype`; with gaps=True also, per position, the distance
    between the two largest values of move_t[j] / z_t over the rows (inf for a single row)."""
    post = np.asarray(post)
    seq = np.asarray(seq, dtype=np.int64).reshape(-1)
    T, S = post.shape
    L = len(seq)
    blank = blank % S
    p = post.astype(dtype)                                    # exact for float32 and float64 rows
    pb = p[:, blank]
    pe = p[:, seq]                                            # [T, L]: the emission of the move into state j + 1

    f = np.zeros((T + 1, L + 1), dtype=dtype)                 # f[t]: in front of row t
    f[0, 0] = 1
    if not full:
        f[0, :] = 1
    total = dtype(0)
    for t in range(T):
        nxt = f[t] * pb[t]
        nxt[1:] += f[t, :-1] * pe[t]
        norm = nxt.sum()
        f[t + 1] = nxt / norm
        total += np.log(norm)
    with np.errstate(divide="ignore"):
        score = total + np.log(f[T, L]) if full else total

    occ = np.zeros((T, S), dtype=dtype)
    ratio = np.zeros((T, L), dtype=dtype)                     # move_t[j] / z_t
    b = np.zeros(L + 1, dtype=dtype)
    b[L] = 1
    if not full:
        b[:] = 1
    for t in range(T - 1, -1, -1):
        stay = f[t] * pb[t] * b
        move = f[t, :-1] * pe[t] * b[1:]
        z = stay.sum() + move.sum()
        if z > 0 and np.isfinite(z):
            occ[t, blank] += stay.sum() / z
            np.add.at(occ[t], seq, move / z)
            ratio[t] = move / z
        nxt = b * pb[t]
        nxt[:-1] += b[1:] * pe[t]
        norm = nxt.sum()
        b = nxt / norm if norm > 0 else nxt
    emit_prob = ratio.max(axis=0) if T else np.zeros(L, dtype=dtype)
    emit_row = np.where(emit_prob > 0, ratio.argmax(axis=0) if T else 0, -1).astype(np.int32)     # argmax: the first, i.e. lowest, row
    if not gaps:
        return score, occ, emit_row, emit_prob
    if T >= 2:
        top = np.sort(ratio, axis=0)[-2:]
        gap = top[1] - top[0]
    else:
        gap = np.full(L, np.inf, dtype=dtype)
    return score, occ, emit_row, emit_prob, gap
