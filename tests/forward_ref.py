"""The forward (sum-product) score of a sequence under a transducer posterior, restated in plain float64 numpy for this
repository's tests (what sloika/decode.py:108-139 computes; nothing of the reference is imported or needed).

    alpha_0[j] = 1 for every j in 0..L              (full: only alpha_0[0] = 1)
    alpha_t[j] = alpha_{t-1}[j] * post[t, blank] + alpha_{t-1}[j-1] * post[t, seq[j-1]]
    normalise every row by its sum, add up the logs of the sums       (full: + log of the last entry)

`blank` may be any column (the reference's is the last).  Serves the GPU tests that have no fixture, and reproduces the fixture's
reference scores within its E_ref (tests/test_forward_host.py).
"""
import numpy as np


def forwards(post, seq, full=False, blank=-1, parts=False):
    """-> the score; with parts=True -> (sum of the log row totals, log of the end state's share of the last row)."""
    post = np.asarray(post)
    seq = np.asarray(seq, dtype=np.int64).reshape(-1)
    npos = len(seq)
    alpha = np.zeros(npos + 1, dtype=np.float64)
    if full:
        alpha[0] = 1.0
    else:
        alpha[:] = 1.0
    total = np.float64(0.0)
    for row in post:
        row = row.astype(np.float64)                      # exact for float32 rows
        nxt = alpha * row[blank]
        nxt[1:] += alpha[:-1] * row[seq]
        norm = np.sum(nxt)
        alpha = nxt / norm
        total += np.log(norm)
    with np.errstate(divide="ignore"):
        end = np.log(alpha[-1])
    if parts:
        return np.float64(total), np.float64(end)
    return np.float64(total + end) if full else np.float64(total)


def forwards_exact(post, seq, full=False, blank=-1):
    """The same recursion in np.longdouble with exact power-of-two scaling: -> (hi, lo) float64 with hi + lo the extended value.
    Needs an extended long double (eps < 1e-18): the fixture generator refuses to run without one."""
    ld = np.longdouble
    post = np.asarray(post)
    seq = np.asarray(seq, dtype=np.int64).reshape(-1)
    alpha = np.zeros(len(seq) + 1, dtype=ld)
    if full:
        alpha[0] = 1
    else:
        alpha[:] = 1
    esum = 0
    for row in post:
        row = row.astype(ld)
        nxt = alpha * row[blank]
        nxt[1:] += alpha[:-1] * row[seq]
        _, e = np.frexp(nxt.sum())
        alpha = np.ldexp(nxt, -int(e))
        esum += int(e)
    with np.errstate(divide="ignore"):
        val = np.log(alpha[-1] if full else alpha.sum()) + ld(esum) * np.log(ld(2))
    hi = np.float64(val)
    lo = np.float64(val - ld(hi)) if np.isfinite(hi) else np.float64(0.0)
    return hi, lo
