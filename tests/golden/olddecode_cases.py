"""The seeded synthetic inputs behind tests/golden/olddecode.npz (the decoder of non-transducer models), the float64 yardsticks both
sides are measured against, and a restatement of numpy's float32 summation order.  Shared by the generator
(make_olddecode_goldens.py) and the tests; nothing here touches the reference or a GPU.

Every transcendental is evaluated in float64 and rounded (to float32, or to a grid) afterwards, so that the inputs do not depend on
which vectorised float32 exp / log a numpy build carries."""
import hashlib

import numpy as np

TRANS_PRIOR = [0.1, 0.8, 0.1]
SLIPS = (0.0, 0.05)
MIN_PROB = 1e-5
ETA = 1e-10

#: name -> (rows, k-mer length, bad state column, transition prior, seed, kind)
#:   walk  : a random walk over the 4^k states with stays, steps and skips; logits peaked by 2 to 7 on the walk; 3 % bad rows
#:   tie   : the same, the posterior rounded to multiples of 2^-12 and the log-posteriors to multiples of 1/4: exact ties
#:   allbad: every row's largest value is the bad column
CASES = {
    "t1": (1, 5, True, None, 101, "walk"),
    "t2": (2, 5, True, None, 102, "walk"),
    "t7": (7, 5, True, TRANS_PRIOR, 103, "walk"),
    "t300": (300, 5, True, None, 104, "walk"),
    "t300_prior": (300, 5, True, TRANS_PRIOR, 105, "walk"),
    "t300_nobad": (300, 5, False, None, 106, "walk"),
    "t120_nobad_prior": (120, 5, False, TRANS_PRIOR, 107, "walk"),
    "t2000": (2000, 5, True, None, 108, "walk"),
    "allbad": (20, 5, True, None, 109, "allbad"),
    "k3": (50, 3, True, None, 110, "walk"),
    "k4": (50, 4, True, TRANS_PRIOR, 111, "walk"),
    "k6": (50, 6, True, None, 112, "walk"),
    "k6_nobad": (50, 6, False, None, 113, "walk"),
    "tie_k3": (60, 3, False, None, 114, "tie"),
    "tie_k5": (80, 5, False, TRANS_PRIOR, 115, "tie"),
    "tie_k4": (40, 4, False, None, 116, "tie"),
}


def _walk_logits(T, klen, bad, rs, all_bad=False):
    """float64 logits [T, 4^k + bad] of a k-mer walk."""
    n = 4 ** klen
    state = int(rs.randint(n))
    walk = np.zeros(T, dtype=np.int64)
    for t in range(T):
        u = rs.rand()
        if t and u >= 0.3:
            if u < 0.9:
                state = (state % (n // 4)) * 4 + int(rs.randint(4))
            else:
                state = (state % (n // 16)) * 16 + int(rs.randint(16))
        walk[t] = state
    logits = rs.normal(size=(T, n + bool(bad)))
    peak = rs.uniform(2.0, 7.0, size=T)
    logits[np.arange(T), walk + bool(bad)] += peak
    if bad:
        logits[:, 0] -= 2.0
        rows = np.ones(T, dtype=bool) if all_bad else rs.rand(T) < 0.03
        logits[rows, 0] += 14.0
    return logits


def _softmax64(x):
    e = np.exp(x - x.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)


def posterior(name):
    """The network posterior of a case: float32 [rows, 1, 4^k + bad], what basecall.decode_post takes."""
    T, klen, bad, _, seed, kind = CASES[name]
    rs = np.random.RandomState(seed)
    p = _softmax64(_walk_logits(T, klen, bad, rs, all_bad=(kind == "allbad")))
    if kind == "tie":
        p = np.round(p * 4096.0) / 4096.0
    return p.astype(np.float32)[:, None, :]


def log_posterior(name):
    """Log-posteriors for decode_profile(log=True) / decode_simple(log=True): float32 [rows, 4^k] on a grid of 2^-10 (tie cases: 1/4),
    and per-event log weights float64 [rows, 3] on a grid of 2^-20."""
    T, klen, _, _, seed, kind = CASES[name]
    rs = np.random.RandomState(seed + 1000)
    lp = np.log(_softmax64(_walk_logits(T, klen, False, rs)))
    grid = 4.0 if kind == "tie" else 1024.0
    lp = (np.round(lp * grid) / grid).astype(np.float32)
    w = np.log(rs.dirichlet([3.0, 6.0, 1.0], size=T))
    wgrid = 4.0 if kind == "tie" else float(2 ** 20)
    return lp, np.round(w * wgrid) / wgrid


def digest(name):
    h = hashlib.sha256()
    lp, w = log_posterior(name)
    for a in (posterior(name), lp, w):
        h.update(np.ascontiguousarray(a).tobytes())
    return np.frombuffer(h.digest(), dtype=np.uint8)


def sha256(a):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), dtype=np.uint8)


def row_picks(n):
    """The rows of a prepared posterior that the fixture stores whole."""
    return sorted(set([0, n // 2, n - 1])) if n > 0 else []


# ---- numpy's float32 summation of a contiguous row -------------------------------------------------------------------------------

def pairwise_sum32(a):
    """np.sum of a contiguous float32 vector, restated: blocks of at most 128 values with eight strided accumulators combined as
    ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)), longer vectors split at n/2 rounded down to a multiple of 8.  This is the order
    csrc/olddecode.hip sums a row in."""
    a = np.asarray(a, dtype=np.float32)
    n = len(a)
    if n < 8:
        s = np.float32(0.0)
        for v in a:
            s = np.float32(s + v)
        return s
    if n <= 128:
        r = a[:8].copy()
        top = n - n % 8
        for i in range(8, top, 8):
            r = (r + a[i:i + 8]).astype(np.float32)
        s = np.float32(np.float32(np.float32(r[0] + r[1]) + np.float32(r[2] + r[3]))
                       + np.float32(np.float32(r[4] + r[5]) + np.float32(r[6] + r[7])))
        for v in a[top:]:
            s = np.float32(s + v)
        return s
    half = n // 2
    half -= half % 8
    return np.float32(pairwise_sum32(a[:half]) + pairwise_sum32(a[half:]))


# ---- float64 yardsticks ----------------------------------------------------------------------------------------------------------

def prepare_np(post, bad, min_prob=MIN_PROB):
    """decode.prepare_post(drop_bad=bad) (sloika/decode.py:21-36) -> (float32 result as numpy evaluates it, indices of the rows kept)."""
    p = np.squeeze(post, axis=1)
    rows = np.arange(len(p))
    if bad:
        keep = np.argmax(p, axis=1) > 0
        rows = rows[keep]
        p = p[keep, 1:]
        p = p / np.sum(p, axis=1, keepdims=True)
    return min_prob + (1.0 - min_prob) * p, rows


def transitions64(post, trans=None):
    """olddecode.estimate_transitions (sloika/olddecode.py:93-117) evaluated in float64 on the same float32 posterior."""
    p = np.asarray(post, dtype=np.float64)
    T, n = p.shape
    res = np.full((T, 3), 1e-10)
    if T > 1:
        prev, cur = p[:-1], p[1:]
        res[:-1, 0] = np.sum(prev * cur, axis=1)
        g4 = cur.reshape(T - 1, n // 4, 4).sum(axis=2)
        res[:-1, 1] = np.sum(prev * np.tile(g4, (1, 4)), axis=1) / 4
        g16 = cur.reshape(T - 1, n // 16, 16).sum(axis=2)
        res[:-1, 2] = np.sum(prev * np.tile(g16, (1, 16)), axis=1) / 16
    if trans is None:
        trans = np.sum(res, axis=0)
        trans = trans / np.sum(trans)
    res = res * np.asarray(trans, dtype=np.float64)
    return res / np.sum(res, axis=1, keepdims=True)
