"""Inputs for the stand-alone Viterbi decoder's edge tests (tests/test_gpu_viterbi_edges.py, tests/test_viterbi_cases_host.py).
Importable without a GPU: numpy only, the library is touched by plan() alone (a host-only entry point).

A batch is built as float32 scores L [T, B, nbase^klen + 1] (column 0 the blank), one chunk KIND per slot, and then handed to the
decoder in one of its input modes:

    log     L itself
    plain   softmax(L): the decoder takes log(p + 1e-10)
    raw     softmax(L): the decoder takes log(min_prob + (1 - min_prob) p + 1e-10)
    logits  L plus a random offset per row, with the row statistics (max, 1 / sum exp(l - max)) and a row stride `ld`

Chunk kinds, in slot order (a batch of B chunks holds the first B):

    tied    random Dirichlet rows (as tests/test_gpu_decode.py draws them), with fully tied rows and rows whose k-mers all tie at the
            steps the caller names (block edges).  What these rows tie: the candidates INSIDE the step maximum and inside the skip
            maximum of the step after a k-mer tied row (the to-states of one thread leave it with equal scores), so np.argmax's
            first-maximum rule, and, where one such group holds both the best step and the best skip predecessor at skip
            penalty 0, the step-versus-skip tie (decode.py:76).  No tied row falls on step 0, the score vector after a tied
            row is not itself tied, and the move-versus-stay tie (decode.py:81) is only met where scores are -inf (`ninf`,
            `dead`): do not read more into this kind
    stay    blank 0, every k-mer column lowered by 5: no state ever moves, the path has length 1
    move    blank -30, k-mer rows close to uniform: every state moves at every step, the path has length T
    ninf    random rows with 30 % of the entries at -inf (log mode only; a plain random chunk in the other modes)
    random  random Dirichlet rows
    dead    random rows, and one row (step T // 2) that is all -inf: from there on no score is above -inf, and the
            decoder must end in state 0 as np.argmax does (log mode only; a plain random chunk in the other modes)
"""
import collections

import numpy as np

KINDS = ("tied", "stay", "move", "ninf", "random", "dead")
MODES = ("log", "plain", "raw", "logits")
MIN_PROB = 1e-5
ETA = np.float32(1e-10)

Plan = collections.namedtuple("Plan", "kernel blank_steps staged_rows tb_row_bytes walker_rows walker_dma")
GENERIC, WORKGROUP4, WAVE4 = 0, 1, 2
LONG = 1 << 20          # a chunk length no block size reaches: plan(LONG, ...) gives the unclamped rows per walker block


def plan(T, B, nbase, klen, ws_align=16):
    """slk_viterbi_kmer_plan: what the decoder launches for this shape (host only)."""
    import ctypes
    from sloika_amd import _lib
    p = _lib.ViterbiPlan()
    rc = _lib.lib().slk_viterbi_kmer_plan(T, B, nbase, klen, ws_align, ctypes.byref(p))
    assert rc == 0, "slk_viterbi_kmer_plan(%d, %d, %d, %d, %d) = %d" % (T, B, nbase, klen, ws_align, rc)
    return Plan(p.kernel, p.blank_steps, p.staged_rows, p.tb_row_bytes, p.walker_rows, p.walker_dma)


def wave_threshold(klen, limit=1 << 16):
    """Smallest batch the wave-per-chunk kernel takes (nbase 4), by bisection on the plan."""
    assert plan(LONG, 1, 4, klen).kernel == WORKGROUP4 and plan(LONG, limit, 4, klen).kernel == WAVE4
    lo, hi = 1, limit                      # lo: workgroup kernel, hi: wave kernel
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if plan(LONG, mid, 4, klen).kernel == WAVE4:
            hi = mid
        else:
            lo = mid
    return hi


def walker_lengths(r):
    """Chunk lengths whose rows 1 .. T-1 fill 1, 2, 3, 4 and 5 walker blocks of r rows, whole and partial first blocks."""
    return sorted(set(x + 1 for x in (r - 1, r, r + 1, 2 * r, 2 * r + 1, 3 * r, 3 * r + 1, 4 * r + 1) if x >= 0))


def blank_lengths(n):
    """Chunk lengths around one and two blocks of n blank-column steps."""
    return sorted(set(x for x in (n - 1, n, n + 1, n + 2, 2 * n, 2 * n + 1) if x >= 1))


def staging_lengths(s):
    """Chunk lengths around one and two blocks of s staged traceback rows, and the two-step unrolled time loop's first trips."""
    return sorted(set([2, s - 1, s, s + 1, s + 2, 2 * s - 1, 2 * s, 2 * s + 1]))


def tie_steps(T, p):
    """(fully tied steps, k-mer tied steps) for a chunk of T steps under plan p: first and last steps of a blank block, of a staged
    traceback block and of the walker's last block; T // 2 where the chunk is too short for any of them."""
    full, kmer = set(), set()
    r = p.walker_rows
    for edge in (p.blank_steps, p.staged_rows, T - r):
        if edge and 1 <= edge < T:
            full.add(edge)
        if edge and 1 <= edge - 1 < T:
            kmer.add(edge - 1)
    if not full and T > 4:
        full.add(T // 2)
    return sorted(full), sorted(kmer - full)


def _log_dirichlet(rs, shape, nst, alpha):
    d = rs.standard_gamma(alpha, size=tuple(shape) + (nst,))
    d /= d.sum(axis=-1, keepdims=True)
    return np.log(d.astype(np.float32) + np.float32(1e-6))


def kinds_of(B, log_mode=True):
    k = [KINDS[i] if i < len(KINDS) else "random" for i in range(B)]
    return [("random" if x in ("ninf", "dead") and not log_mode else x) for x in k]


def scores(T, B, nbase, klen, seed, tied_full=(), tied_kmer=(), log_mode=True):
    """float32 L [T, B, nstate] with one chunk kind per slot (kinds_of(B, log_mode))."""
    nst = nbase ** klen + 1
    rs = np.random.RandomState(seed)
    L = _log_dirichlet(rs, (T, B), nst, 0.3)
    for b, kind in enumerate(kinds_of(B, log_mode)):
        if kind == "tied":
            for t in tied_full:
                L[t, b, :] = L[t, b, 0]
            for t in tied_kmer:
                L[t, b, 1:] = L[t, b, 1]
        elif kind == "stay":
            L[:, b, 1:] -= np.float32(5.0)
            L[:, b, 0] = 0.0
        elif kind == "move":
            L[:, b, :] = _log_dirichlet(rs, (T,), nst, 50.0)
            L[:, b, 0] = -30.0
        elif kind == "ninf":
            L[:, b, :][rs.uniform(size=(T, nst)) < 0.3] = -np.inf
        elif kind == "dead":
            L[T // 2, b, :] = -np.inf
    return L


def softmax(L):
    """softmax over the state axis in float64, rounded to float32 (the posterior of the plain and raw modes)."""
    x = L.astype(np.float64)
    x -= x.max(axis=-1, keepdims=True)
    e = np.exp(x)
    return (e / e.sum(axis=-1, keepdims=True)).astype(np.float32)


def logits_of(L, seed, ld=None):
    """(buffer [T*B, ld] with NaN behind each row's nstate logits, stats [T*B, 2], ld): L shifted by a random offset per row."""
    T, B, nst = L.shape
    ld = nst if ld is None else ld
    assert ld >= nst
    rs = np.random.RandomState(seed)
    lg = (L + rs.normal(scale=3.0, size=(T, B, 1)).astype(np.float32)).reshape(T * B, nst)
    mx = lg.max(axis=1)
    inv = 1.0 / np.exp(lg.astype(np.float64) - mx[:, None]).sum(axis=1)
    buf = np.full((T * B, ld), np.nan, dtype=np.float32)
    buf[:, :nst] = lg
    return buf, np.stack([mx, inv.astype(np.float32)], axis=1).astype(np.float32), ld


def numpy_log_post(mode, data, stats=None, nst=None, min_prob=MIN_PROB):
    """What numpy's float32 makes of the decoder's input transform (decode.py:36, :56): the device's own conversion must be
    within rtol 1e-6, atol 2e-6 of it, and the host tests decode it."""
    if mode == "log":
        return data
    if mode == "logits":
        data = np.exp(data[:, :nst] - stats[:, :1]) * stats[:, 1:]
    if mode in ("raw", "logits"):
        data = np.float32(min_prob) + np.float32(1.0 - min_prob) * data
    with np.errstate(divide="ignore"):
        return np.log(data + ETA)


def ragged_lengths(T, B, edges):
    """int32 [B]: T, 1, 2 and the edge values below T first, then the same again for as long as the batch lasts.  The `move`
    chunk (slot 2) keeps a length of its own that is more than 2, where the batch allows."""
    vals = [T, 1, 2] + [e for e in edges if 2 < e < T]
    vals = list(dict.fromkeys(v for v in vals if 1 <= v <= T))
    if len(vals) > 3:
        vals[2], vals[3] = vals[3], vals[2]
    return np.asarray([vals[i % len(vals)] for i in range(B)], dtype=np.int32)


def poison(buf, stats, lens, T, B):
    """NaN in every logit and statistic at t >= lens[b]: one read past a chunk's own end poisons its score."""
    dead = (np.arange(T)[:, None] >= np.asarray(lens)[None, :]).reshape(T * B)
    buf[dead] = np.nan
    stats[dead] = np.nan


def expected(orc, lp, klen, skip, nbase, lens=None):
    """The oracle's (scores, paths [B, T] padded with -1, lens) on log-posteriors lp [T, B, nstate]; a ragged batch chunk by
    chunk over its own first lens[b] rows."""
    T, B, _ = lp.shape
    if lens is None:
        return orc.viterbi_batch(lp, klen, skip_pen=skip, nbase=nbase)
    s = np.empty(B, dtype=np.float32)
    p = np.full((B, T), -1, dtype=np.int32)
    n = np.empty(B, dtype=np.int32)
    for b in range(B):
        tb = int(lens[b])
        sb, pb, nb = orc.viterbi_batch(np.ascontiguousarray(lp[:tb, b:b + 1]), klen, skip_pen=skip, nbase=nbase)
        s[b], n[b] = sb[0], nb[0]
        p[b, :tb] = pb[0]
    return s, p, n
