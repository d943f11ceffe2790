"""The banded form of tests/rescore_ref.py, restated in plain float64 loops from design/rescore_band.md for this repository's tests
(nothing of the device code is imported), the np.longdouble truth of the same identity, and the cases the CPU and GPU tests share.

A pair has a width W and lo[0 .. T]; state j exists in row t when lo[t] <= j < lo[t] + W and 0 <= j <= L.  F and B follow the dense
recursions with every other state 0, the scaling is the dense one with the row total taken over the band.  Since lo does not decrease
the rows in which state j exists are one interval [t0(j), t1(j)]; a candidate's chain starts in row t0(a), its cut sum runs over
t = t0(a) .. t1(a + d + 1) - 1 and its own first term initialises the (mantissa, exponent) pair.
"""
import math

import numpy as np

from tests import rescore_ref as rr

MAX_NEW = rr.MAX_NEW
WIDTHS = (256, 512, 1024, 2048)
THREADS = 256


def valid_band(lo, T, L, W):
    lo = [int(v) for v in lo]
    return len(lo) == T + 1 and lo[0] == 0 and all(v >= 0 for v in lo) and all(lo[t] <= lo[t + 1] for t in range(T)) and lo[T] + W > L


def rows_of(lo, W, j):
    """(t0, t1): the rows in which state j exists; t0 > t1 when there is none."""
    T = len(lo) - 1
    t0 = next((t for t in range(T + 1) if lo[t] + W > j), T + 1)
    t1 = max((t for t in range(T + 1) if lo[t] <= j), default=-1)
    return t0, t1


def lattice(post, seq, lo, W, blank=-1):
    """rescore_ref.lattice with every state outside its row's band 0: -> (F [T+1][L+1], B, EF, EB)."""
    post = np.asarray(post).astype(np.float64)
    seq = [int(s) for s in seq]
    T, L = post.shape[0], len(seq)
    inside = lambda t, j: lo[t] <= j < lo[t] + W and 0 <= j <= L          # noqa: E731
    F = np.zeros((T + 1, L + 1))
    B = np.zeros((T + 1, L + 1))
    EF, EB = [0] * (T + 1), [0] * (T + 1)
    F[0, 0] = 1.0
    for t in range(T):
        e = rr._exponent(float(np.sum(F[t])))
        for j in range(max(lo[t + 1], 0), min(lo[t + 1] + W, L + 1)):
            g = F[t, j] * post[t, blank]
            if j >= 1:
                g += F[t, j - 1] * post[t, seq[j - 1]]
            F[t + 1, j] = math.ldexp(g, -e)
        EF[t + 1] = EF[t] + e
    if inside(T, L):
        B[T, L] = 1.0
    for t in range(T - 1, -1, -1):
        e = rr._exponent(float(np.sum(B[t + 1])))
        for j in range(max(lo[t], 0), min(lo[t] + W, L + 1)):
            g = B[t + 1, j] * post[t, blank]
            if j < L:
                g += B[t + 1, j + 1] * post[t, seq[j]]
            B[t, j] = math.ldexp(g, -e)
        EB[t] = EB[t + 1] + e
    return F, B, EF, EB


def rescore(post, seq, edits, lo, W, blank=-1):
    """-> (banded score of seq, [ll_edit]); everything NaN for an invalid band, NaN for an edit rescore_ref.rescore refuses."""
    post = np.asarray(post).astype(np.float64)
    seq = [int(s) for s in seq]
    lo = [int(v) for v in lo]
    T, S = post.shape
    L = len(seq)
    if not valid_band(lo, T, L, W):
        return math.nan, [math.nan] * len(edits)
    F, B, EF, EB = lattice(post, seq, lo, W, blank)
    score = rr._log_scaled(F[T, L], EF[T])
    out = []
    for a, d, new in edits:
        new = [int(c) for c in new]
        m = len(new)
        if a < 0 or d < 0 or a + d > L or m > MAX_NEW or any(c < 0 or c >= S for c in new):
            out.append(math.nan)
            continue
        t0 = rows_of(lo, W, a)[0]
        tend = rows_of(lo, W, a + d + 1)[1] if a + d < L else T       # terms t0 .. tend - 1; a chain that ends the sequence runs to T
        if t0 > T:
            out.append(-math.inf)
            continue
        g = [0.0] * (m + 1)
        g[0] = F[t0, a]
        acc, acce = 0.0, 0
        for t in range(t0, max(tend, t0)):
            if a + d < L:
                term = (g[m] * post[t, seq[a + d]]) * math.ldexp(B[t + 1, a + d + 1],
                                                                 max(min((EF[t] - EF[t + 1]) + (EB[t + 1] - EB[t]), 4096), -4096))
                e = EF[t + 1] + EB[t]
                if t == t0 or e > acce:
                    acc = math.ldexp(acc, max(acce - e, -4096)) + term
                    acce = e
                else:
                    acc += math.ldexp(term, max(e - acce, -4096))
            de = EF[t + 1] - EF[t]
            for i in range(m, 0, -1):
                g[i] = math.ldexp(g[i - 1] * post[t, new[i - 1]] + g[i] * post[t, blank], -de)
            g[0] = F[t + 1, a]                                        # (0 once a has left the band)
        out.append(rr._log_scaled(acc, acce) if a + d < L else rr._log_scaled(g[m], EF[T]))
    return score, out


# ---- the same identity with one vector operation per row: the np.longdouble truth, and the float64 model of long pairs ----------------

def _band_pass(post, seq, lo, W, blank, down, ld):
    """Band-indexed rows V [T+1][W] (V[t][k] is state lo[t] + k) in `ld` arithmetic and the running exponents."""
    T, L = post.shape[0], len(seq)
    V = np.zeros((T + 1, W), dtype=ld)
    E = np.zeros(T + 1, dtype=np.int64)
    k = np.arange(W)
    if not down:
        V[0, 0] = 1
        order = range(T)
    else:
        if lo[T] <= L:
            V[T, L - lo[T]] = 1
        order = range(T - 1, -1, -1)
    zero = np.zeros(W, dtype=ld)
    for t in order:
        src, dst = (t, t + 1) if not down else (t + 1, t)
        row = post[t].astype(ld)
        shift = int(lo[dst] - lo[src])                                # >= 0 upwards, <= 0 downwards
        if abs(shift) <= W + 1:
            ext = np.zeros(3 * W + 4, dtype=ld)                       # state lo[src] + i sits at ext[W + 2 + i]
            ext[W + 2:2 * W + 2] = V[src]
            own = ext[W + 2 + shift:2 * W + 2 + shift]
            nb = ext[W + 1 + shift:2 * W + 1 + shift] if not down else ext[W + 3 + shift:2 * W + 3 + shift]
        else:
            own = nb = zero
        j = lo[dst] + k
        em = np.zeros(W, dtype=ld)
        ok = ((j >= 1) & (j <= L)) if not down else (j < L)
        em[ok] = row[seq[j[ok] - (0 if down else 1)]]
        nxt = own * row[blank]
        nxt = nxt + nb * em
        nxt[j > L] = 0
        tot = V[src].sum()
        e = int(np.frexp(tot)[1]) if 0 < tot < np.inf else 0
        V[dst] = np.ldexp(nxt, -e)
        E[dst] = E[src] + e
    return V, E


def evaluate(post, seq, edits, lo, W, blank=-1, ld=np.longdouble):
    """-> (score, ll_edit array) in `ld` arithmetic (NaN and -inf as the model has them): np.longdouble is the truth (the scaling is
    exact), np.float64 the model of `rescore` with every operation in its order, but the row totals, which numpy adds pairwise over
    the band here and over the whole row there.  The candidates walk the rows together, each within its own rows only."""
    post = np.asarray(post)
    seq = np.asarray(seq, dtype=np.int64).reshape(-1)
    lo = np.asarray(lo, dtype=np.int64).reshape(-1)
    T, S = post.shape
    L = len(seq)
    n = len(edits)
    if not valid_band(lo, T, L, W):
        return ld(np.nan), np.full(n, np.nan, dtype=ld)
    clamp = 4096 if ld is np.float64 else 30000
    F, EF = _band_pass(post, seq, lo, W, blank, False, ld)
    B, EB = _band_pass(post, seq, lo, W, blank, True, ld)
    ln2 = np.log(ld(2))

    def at(V, t, j):
        k = j - lo[t]
        inb = (k >= 0) & (k < W)
        return np.where(inb, V[t, np.where(inb, k, 0)], ld(0))

    def logs(mant, expo):
        with np.errstate(divide="ignore"):
            return np.log(mant) + expo.astype(ld) * ln2

    score = logs(at(F, T, np.array([L]))[:1], EF[T:T + 1])[0]
    out = np.full(n, np.nan, dtype=ld)
    good = [i for i, (a, d, new) in enumerate(edits)
            if a >= 0 and d >= 0 and a + d <= L and len(new) <= MAX_NEW and all(0 <= int(c) < S for c in new)]
    if not good:
        return score, out
    good.sort(key=lambda i: edits[i][0])
    a = np.array([edits[i][0] for i in good], dtype=np.int64)
    d = np.array([edits[i][1] for i in good], dtype=np.int64)
    m = np.array([len(edits[i][2]) for i in good], dtype=np.int64)
    M = int(m.max())
    inj = M - m
    sym = np.full((len(good), max(M, 1)), -1, dtype=np.int64)        # sym[:, i] enters slot i + 1; the chain sits at the end
    for r, i in enumerate(good):
        if m[r]:
            sym[r, M - m[r]:M] = np.asarray(edits[i][2], dtype=np.int64)
    cut = a + d < L
    cb = a + d + 1
    nxt = np.where(cut, seq[np.minimum(a + d, max(L - 1, 0))] if L else 0, 0)
    t0 = np.searchsorted(lo, a - W, side="right")
    tend = np.where(cut, np.searchsorted(lo, cb, side="right") - 1, T)
    rows = np.arange(len(good))
    symok, symc = sym[:, :M] >= 0, np.maximum(sym[:, :M], 0)
    g = np.zeros((len(good), M + 1), dtype=ld)
    g[rows, inj] = np.where(t0 <= T, F[np.minimum(t0, T), np.clip(a - lo[np.minimum(t0, T)], 0, W - 1)], 0)      # (a is inside row t0)
    acc = np.zeros(len(good), dtype=ld)
    acce = np.zeros(len(good), dtype=np.int64)
    t0m = np.minimum.accumulate(t0[::-1])[::-1]
    tem = np.maximum.accumulate(tend)
    for t in range(int(t0.min()), int(tend.max())):
        i0, i1 = int(np.searchsorted(tem, t, side="right")), int(np.searchsorted(t0m, t, side="right"))
        if i0 >= i1:
            continue
        sl = slice(i0, i1)
        act = (t0[sl] <= t) & (t < tend[sl])
        row = post[t].astype(ld)
        gs = g[sl]
        # the cut term of t (a lane that ends the sequence reads column L + 1 of B, which is 0, and is masked besides)
        shift = int(np.clip((EF[t] - EF[t + 1]) + (EB[t + 1] - EB[t]), -clamp, clamp))
        term = (gs[:, M] * row[nxt[sl]]) * np.ldexp(at(B, t + 1, cb[sl]), shift)
        e = int(EF[t + 1] + EB[t])
        ae = acce[sl]
        first = (t0[sl] == t) | (e > ae)
        tact = act & cut[sl]
        down = np.where(first, np.maximum(ae - e, -clamp), 0).astype(np.int32)       # the sum comes down to e, or
        up = np.where(first, 0, np.maximum(e - ae, -clamp)).astype(np.int32)         # the term to the sum's exponent
        acc[sl] = np.where(tact, np.ldexp(acc[sl], down) + np.ldexp(term, up), acc[sl])
        acce[sl] = np.where(tact & first, e, ae)
        # g_t -> g_{t+1}
        de = int(EF[t + 1] - EF[t])
        new = np.empty_like(gs)
        new[:, 1:] = np.ldexp(gs[:, :-1] * np.where(symok[sl], row[symc[sl]], ld(0)) + gs[:, 1:] * row[blank], -de)
        new[:, 0] = 0
        new[rows[:i1 - i0], inj[sl]] = at(F, t + 1, a[sl])
        g[sl] = np.where(act[:, None], new, gs)
    res = np.where(cut, logs(acc, acce), logs(g[:, M], np.full(len(good), EF[T])))
    res = np.where(t0 > T, ld(-np.inf), res)
    out[np.array(good)] = res
    return score, out


def truth(post, seq, edits, lo, W, blank=-1):
    """-> (score, [ll_edit]) as np.longdouble."""
    return evaluate(post, seq, edits, lo, W, blank, np.longdouble)


# ---- bands ---------------------------------------------------------------------------------------------------------------------------

def band_lo(center, npos, width):
    """clamp(center - width // 2, 0, max(0, npos + 1 - width)), then a running maximum (decode.band_lo)."""
    c = np.asarray(center, dtype=np.int64)
    return np.maximum.accumulate(np.clip(c - width // 2, 0, max(0, npos + 1 - width))).astype(np.int32)


def center_from_rows(rows, T):
    """The planted path's state per row index 0 .. T: how many of the sorted emitting rows lie before it."""
    return np.searchsorted(np.asarray(rows), np.arange(T + 1), side="left")


def zero_band(T):
    return np.zeros(T + 1, dtype=np.int32)


def width_for(L):
    """The smallest built width that holds L + 1 states."""
    return next(w for w in WIDTHS if w >= L + 1)


# ---- the ring, restated from design/rescore_band.md 3 (shapes only) ---------------------------------------------------------------------

def ppt_of(W):
    assert W in WIDTHS
    return W // THREADS


def ahead_of(W):
    return rr.ahead_of(ppt_of(W))


def ring_facts(lo, W, L):
    """What a band does to the ring: how often a slot changes its state (wraps), the steps of lo, and whether a step moves the
    band's first state across a thread, a wave and the ring's end."""
    lo = np.asarray(lo, dtype=np.int64)
    ppt = ppt_of(W)
    steps = np.diff(lo)
    cross = lambda unit: bool(((lo[1:] // unit) != (lo[:-1] // unit)).any())          # noqa: E731
    return dict(wraps=int(lo[-1] // W), steps=sorted(set(int(s) for s in steps)), thread=cross(ppt), wave=cross(64 * ppt), ring=cross(W),
                consecutive=bool(((steps[1:] > 0) & (steps[:-1] > 0)).any()) if len(steps) > 1 else False,
                step_rows=[int(t) for t in np.nonzero(steps)[0]])


# ---- the cases the CPU and the GPU tests share ---------------------------------------------------------------------------------------------

RING_T = 40
RING = ((5, 600, 256), (17, 1300, 512), (17, 5000, 2048))                          # (S, L, W)


def ring_steps(W):
    """One pair's band steps (design/rescore_band.md 6): W and W + 1 lose all mass and come last."""
    ppt = ppt_of(W)
    return [0, 1, ppt - 1, ppt, ppt + 1, 64, 255, W - 1, W, W + 1]


def ring_lo(L, W, T=RING_T, lossy=False):
    """lo for T rows that ends with lo[T] + W > L.  Steps of ring_steps(W), each once, in consecutive rows and fs_ahead rows apart;
    without `lossy` the steps W and W + 1 are left out and the rest is made up by steps of W - 1; with it a step of W + 3 follows,
    which skips three states altogether (a step of W + 1 skips one, so no edit can have both its columns skipped)."""
    D = ahead_of(W)
    steps = [s for s in ring_steps(W) if lossy or s < W]
    if lossy:                                                        # (the skipping steps before the band has passed the sequence's end)
        steps = steps[:-3] + [W + 3, W, W + 1, W - 1]
    inc = np.zeros(T, dtype=np.int64)
    t = 1
    for i, s in enumerate(steps):
        inc[t] = s
        t += 1 if i % 2 == 0 else D                                  # pairs of consecutive rows, then fs_ahead rows on
    assert t <= T
    lo = np.concatenate([[0], np.cumsum(inc)])
    free = [r for r in range(t, T)]
    while lo[-1] + W <= L:
        assert free, "the band cannot reach the end"
        inc[free.pop(0)] = W - 1
        lo = np.concatenate([[0], np.cumsum(inc)])
    return lo.astype(np.int32)


def ring_case(S, L, W, T=RING_T, seed=83, lossy=False, dtype=np.float64):
    """A pair of T rows against L positions whose band runs down the whole sequence, and edits that leave few enough positions for T
    rows: the head up to a kept column `a`, a long deletion, the tail from a + d on.  Candidates sit on the band's edges: a == lo[t]
    and a == lo[t] + W - 1 in the first and last row of a's interval, a + d + 1 one past the band, t0(a) > t1(a + d + 1), both ends,
    m = 0, 1 and 8.  -> (post, seq, edits, lo)"""
    rng = np.random.default_rng(seed + L + (1 if lossy else 0))
    lo = ring_lo(L, W, T, lossy)
    post = rng.uniform(0.05, 1.0, size=(T, S))
    post[:, -1] += 1.0
    post = (post / post.sum(axis=1, keepdims=True)).astype(dtype)
    seq = rng.integers(0, S - 1, size=L)
    sym = lambda m: rng.integers(0, S - 1, size=m)                    # noqa: E731
    edits = []
    # the sequence cut down to its head and tail: (a, d) with a small and a + d close to L, so that T rows can emit what is left
    for a in (0, 1, 5):
        for end in (L, L - 1, L - 4):
            for m in (0, 1, 8):
                if a + m + (L - end) <= T:
                    edits.append((a, end - a, sym(m)))
    # columns on the band's edges: for some rows t, a = lo[t] and a = lo[t] + W - 1, and a + d + 1 at, and one past, the edges of later rows
    for t in (1, 2, 3, 5, 9, 17, 33, T - 1, T):
        for a in (int(lo[t]), int(lo[t]) + W - 1):
            if not 0 <= a <= L:
                continue
            for t2 in (t, min(t + 1, T), T):
                for cb in (int(lo[t2]) + W - 1, int(lo[t2]) + W, int(lo[t2])):
                    d = cb - 1 - a
                    if d >= 0 and a + d <= L:
                        edits.append((a, d, sym((0, 1, 8)[len(edits) % 3])))
    # columns the band skips: a exists in no row, and the last row of a + d + 1 lies before the first of a
    for t in range(T):
        if lo[t + 1] - lo[t] > W and lo[t] + W <= L:
            a = int(lo[t]) + W
            edits += [(a, 0, sym(1)), (a, 1, sym(0))] if a + 1 <= L else [(a, 0, sym(1))]
    edits += [(0, 0, sym(1)), (L, 0, sym(1)), (L, 0, sym(0)), (0, L, sym(8))]
    return post, seq, edits, lo


def few_rows_cases(L=300, W=256, rows=(0, 1, 2, 3, 4, 5), S=65, seed=89, dtype=np.float64):
    """T = 0 .. 5 under L = 300 at W = 256: the band must step by at least 45 to end above L; below, at and above fs_ahead = 4."""
    rng = np.random.default_rng(seed)
    out = []
    for T in rows:
        post = rng.uniform(0.05, 1.0, size=(T, S))
        post = (post / post.sum(axis=1, keepdims=True)).astype(dtype)
        lo = np.zeros(T + 1, dtype=np.int32)
        if T:
            lo[1:] = np.linspace(L + 1 - W, L + 1 - W + T - 1, T).astype(np.int32) if T > 1 else L + 1 - W
        seq = rng.integers(0, S - 1, size=L)
        out.append((post, seq, rr.few_rows_edits(L, T, rng, S), lo))
    return out


def diagonal_long(T=20000, L=9000, S=65, seed=97):
    """One planted float32 pair past the dense limit (rescore_ref.diagonal_case's recipe) and the centre of its planted path.
    -> (post, seq, center [T + 1])"""
    rng = np.random.default_rng(seed)
    seq = rng.integers(0, S - 1, size=L)
    post = (rng.uniform(size=(T, S)) * rng.uniform(size=(T, S))).astype(np.float32)
    rows = np.sort(rng.choice(T, size=L, replace=False))
    post[rows, seq] += 1.0
    post[:, -1] += 0.3
    post = (post / post.sum(axis=1, keepdims=True)).astype(np.float32)
    return post, seq, center_from_rows(rows, T)


def letter_edit_sample(seq, n, seed, S):
    """n seeded single-symbol edits (substitution, deletion, insertion) spread over the sequence, both ends among them."""
    rng = np.random.default_rng(seed)
    L = len(seq)
    pos = np.concatenate([[0, L - 1], rng.integers(1, L - 1, size=n - 2)])
    out = []
    for i, a in enumerate(pos):
        kind = i % 3
        a = int(a)
        if kind == 0:
            out.append((a, 1, rng.integers(0, S - 1, size=1)))
        elif kind == 1:
            out.append((a, 1, np.zeros(0, dtype=np.int64)))
        else:
            out.append((a + (1 if a == L - 1 else 0), 0, rng.integers(0, S - 1, size=1)))
    return out


def planted_long(seed=7, k=3, nletters=1002, nrow=3000, nread=3, alphabet='ACGT'):
    """rescore_ref.planted_case scaled to whole-read proportions (T = 3000, L = 1000 k-mers): a substitution at letter 200, a deletion
    at 520 and an insertion at 850, and per read the centre of its planted path.  -> (truth, draft, [post], [center of the draft])"""
    rng = np.random.default_rng(seed)
    truth_s = ''.join(alphabet[i] for i in rng.integers(0, 4, size=nletters))
    states = rr.states_of(truth_s, k, alphabet)
    posts, centers = [], []
    for _ in range(nread):
        post = 0.2 * rng.uniform(size=(nrow, len(alphabet) ** k + 1))
        rows = np.sort(rng.choice(nrow, size=len(states), replace=False))
        post[:, 0] += 1.0
        post[rows, 0] -= 1.0
        post[rows, np.array(states) + 1] += 1.0
        posts.append((post / post.sum(axis=1, keepdims=True)).astype(np.float32))
        centers.append(center_from_rows(rows, nrow))
    other = lambda c: alphabet[(alphabet.index(c) + 1 + int(rng.integers(0, 3))) % 4]          # noqa: E731
    draft = list(truth_s)
    draft[200] = other(truth_s[200])
    ins = alphabet[int(rng.integers(0, 4))]
    draft = draft[:520] + draft[521:850] + [ins] + draft[850:]
    return truth_s, ''.join(draft), posts, centers


def shift_center(center, edits):
    """Every centre value above an applied edit's start moves by that edit's m - d (decode.shift_center): edits = [(start, ndel, nnew)]."""
    c = np.asarray(center, dtype=np.int64)
    if not len(edits):
        return c.copy()
    e = sorted(edits)
    starts = np.array([s for s, _, _ in e], dtype=np.int64)
    delta = np.concatenate([[0], np.cumsum([m - d for _, d, m in e])]).astype(np.int64)
    return c + delta[np.searchsorted(starts, c, side="left")]


# ---- polish with a band: rescore_ref.gains / polish on `evaluate` in float64 ----------------------------------------------------------

def _states_np(text, k, alphabet='ACGT'):
    """rescore_ref.states_of as an array (a thousand-letter draft has eight thousand edited strings per round)."""
    table = np.zeros(256, dtype=np.int64)
    table[np.frombuffer(alphabet.encode(), dtype=np.uint8)] = np.arange(len(alphabet))
    code = table[np.frombuffer(text.encode(), dtype=np.uint8)]
    n = len(text) - k + 1
    out = np.zeros(max(n, 0), dtype=np.int64)
    for i in range(k):
        out += code[i:i + n] * len(alphabet) ** (k - 1 - i)
    return out


def _strip_common_np(old, new):
    """rescore_ref.strip_common on arrays: the longest common prefix, then the longest common suffix of what is left."""
    n = min(len(old), len(new))
    ne = np.nonzero(old[:n] != new[:n])[0]
    pre = int(ne[0]) if len(ne) else n
    r = n - pre
    ne = np.nonzero(old[len(old) - r:][::-1] != new[len(new) - r:][::-1])[0] if r else np.zeros(0, dtype=np.int64)
    suf = int(ne[0]) if len(ne) else r
    return pre, len(old) - pre - suf, [int(v) for v in new[pre:len(new) - suf]]


def gains(posts, text, k, centers, W, blank=0, alphabet='ACGT'):
    """rescore_ref.gains with the band of W states round each read's centre line: -> (rows, gain, summed score, [(a, d, m)])."""
    S = np.asarray(posts[0]).shape[1]
    bl = blank + S if blank < 0 else blank
    col = lambda st: [s + (1 if s >= bl else 0) for s in st]          # noqa: E731
    old = rr.states_of(text, k, alphabet)
    rows = [r for r in rr.letter_edits(text, alphabet) if len(r[3]) >= k]
    olda = _states_np(text, k, alphabet)
    edits = []
    for r in rows:
        a, d, new = _strip_common_np(olda, _states_np(r[3], k, alphabet))
        edits.append((a, d, col(new)))
    gain = np.zeros(len(rows))
    total = 0.0
    for post, center in zip(posts, centers):
        score, ll = evaluate(post, col(old), edits, band_lo(center, len(old), W), W, blank, np.float64)
        gain += ll - score
        total += float(score)
    return rows, gain, total, [(a, d, len(new)) for a, d, new in edits]


def polish(posts, text, k, centers, W, blank=0, min_gain=0.0, max_rounds=8, most=None, alphabet='ACGT'):
    """rescore_ref.polish with a band; the centre lines follow the applied edits (shift_center), nothing is re-aligned.
    -> (polished string, [(round, kind, letter_pos, letter, gain)], rounds that applied something, summed score of the result)."""
    applied, rounds, total = [], 0, None
    centers = [np.asarray(c, dtype=np.int64) for c in centers]
    for r in range(max_rounds + 1):
        rows, gain, total, trip = gains(posts, text, k, centers, W, blank, alphabet)
        taken = rr.accept(rows, gain, k, min_gain, most) if r < max_rounds else []
        if not taken:
            break
        applied += [(r, rows[i][0], rows[i][1], rows[i][2], float(gain[i])) for i in taken]
        text = rr.apply_edits(text, [rows[i][:3] for i in taken])
        centers = [shift_center(c, [trip[i] for i in taken]) for c in centers]
        rounds += 1
    return text, applied, rounds, total
