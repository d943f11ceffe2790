"""The forward score of an edited sequence from the stored lattices of the unedited one, restated in plain float64 loops from
design/rescore_edits.md for this repository's tests (nothing of the device code is imported).

    F_0 = e_0      F_t[j]     = F_{t-1}[j] p_t[blank] + F_{t-1}[j-1] p_t[seq[j-1]]
    B_T = e_L      B_{t-1}[j] = B_t[j] p_t[blank] + B_t[j+1] p_t[seq[j]]
    edit (a, d, c[0..m)):  g_t[0] = F_t[a], g_0[i > 0] = 0, g_t[i] = g_{t-1}[i] p_t[blank] + g_{t-1}[i-1] p_t[c[i-1]]
    a + d < L:  Z' = sum_{t=0}^{T-1} g_t[m] p_{t+1}[seq[a+d]] B_{t+1}[a+d+1]          a + d = L:  Z' = g_T[m]

Rows are scaled by the exact power of two of the previous row's total (integer running exponents EF_t, EB_t), g with its row's
EF_t - EF_{t-1}; a term's B_{t+1} is first freed of the scales of row t of F and of its own row (times 2^-(EF_{t+1} - EF_t) and
2^-(EB_t - EB_{t+1}), exact), the term carries EF_{t+1} + EB_t, and the terms are added in ascending t as (mantissa, exponent).
"""
import math

import numpy as np

MAX_NEW = 8
KINDS = ('sub', 'del', 'ins')


def _exponent(total):
    return math.frexp(total)[1] if 0.0 < total < math.inf else 0


def lattice(post, seq, blank=-1):
    """-> (F [T+1][L+1], B [T+1][L+1], EF [T+1], EB [T+1]): the true F_t is F[t] * 2^EF[t], likewise B."""
    post = np.asarray(post).astype(np.float64)
    seq = [int(s) for s in seq]
    T, L = post.shape[0], len(seq)
    F = np.zeros((T + 1, L + 1))
    B = np.zeros((T + 1, L + 1))
    EF, EB = [0] * (T + 1), [0] * (T + 1)
    F[0, 0] = 1.0
    for t in range(T):
        e = _exponent(float(np.sum(F[t])))
        for j in range(L + 1):
            g = F[t, j] * post[t, blank]
            if j >= 1:
                g += F[t, j - 1] * post[t, seq[j - 1]]
            F[t + 1, j] = math.ldexp(g, -e)
        EF[t + 1] = EF[t] + e
    B[T, L] = 1.0
    for t in range(T - 1, -1, -1):
        e = _exponent(float(np.sum(B[t + 1])))
        for j in range(L + 1):
            g = B[t + 1, j] * post[t, blank]
            if j < L:
                g += B[t + 1, j + 1] * post[t, seq[j]]
            B[t, j] = math.ldexp(g, -e)
        EB[t] = EB[t + 1] + e
    return F, B, EF, EB


def _log_scaled(mant, expo):
    if mant != mant:
        return math.nan
    return (math.log(mant) if mant > 0.0 else -math.inf) + expo * math.log(2.0)


def spell(seq, edit):
    a, d, new = edit
    seq = [int(s) for s in seq]
    return seq[:a] + [int(c) for c in new] + seq[a + d:]


def rescore(post, seq, edits, blank=-1):
    """-> (score of seq, [ll_edit]); NaN for an edit that lies outside the sequence, has more than MAX_NEW new symbols or a new
    symbol that is no column."""
    post = np.asarray(post).astype(np.float64)
    seq = [int(s) for s in seq]
    T, S = post.shape
    L = len(seq)
    F, B, EF, EB = lattice(post, seq, blank)
    score = _log_scaled(F[T, L], EF[T])
    out = []
    for a, d, new in edits:
        new = [int(c) for c in new]
        m = len(new)
        if a < 0 or d < 0 or a + d > L or m > MAX_NEW or any(c < 0 or c >= S for c in new):
            out.append(math.nan)
            continue
        g = [0.0] * (m + 1)
        g[0] = F[0, a]
        acc, acce = 0.0, 0
        for t in range(T):
            if a + d < L:
                term = (g[m] * post[t, seq[a + d]]) * math.ldexp(B[t + 1, a + d + 1], max(min((EF[t] - EF[t + 1]) + (EB[t + 1] - EB[t]), 4096), -4096))
                e = EF[t + 1] + EB[t]
                if t == 0 or e > acce:
                    acc = math.ldexp(acc, max(acce - e, -4096)) + term
                    acce = e
                else:
                    acc += math.ldexp(term, max(e - acce, -4096))
            de = EF[t + 1] - EF[t]
            for i in range(m, 0, -1):
                g[i] = math.ldexp(g[i - 1] * post[t, new[i - 1]] + g[i] * post[t, blank], -de)
            g[0] = F[t + 1, a]
        out.append(_log_scaled(acc, acce) if a + d < L else _log_scaled(g[m], EF[T]))
    return score, out


# ---- polish ------------------------------------------------------------------------------------------------------------------------

def states_of(text, k, alphabet='ACGT'):
    return [sum(alphabet.index(c) * len(alphabet) ** (k - 1 - i) for i, c in enumerate(text[p:p + k])) for p in range(len(text) - k + 1)]


def letter_edits(text, alphabet='ACGT'):
    """(kind, letter_pos, letter, edited string) by letter_pos, kind, letter."""
    rows = []
    for p in range(len(text) + 1):
        if p < len(text):
            rows += [('sub', p, c, text[:p] + c + text[p + 1:]) for c in alphabet if c != text[p]]
            rows.append(('del', p, '', text[:p] + text[p + 1:]))
        rows += [('ins', p, c, text[:p] + c + text[p:]) for c in alphabet]
    return rows


def strip_common(old, new):
    pre = 0
    while pre < min(len(old), len(new)) and old[pre] == new[pre]:
        pre += 1
    suf = 0
    while suf < min(len(old), len(new)) - pre and old[len(old) - 1 - suf] == new[len(new) - 1 - suf]:
        suf += 1
    return pre, len(old) - pre - suf, new[pre:len(new) - suf]


def gains(posts, text, k, blank=0, alphabet='ACGT'):
    """-> (rows of letter_edits, gain per row summed over the posteriors, summed score); columns are state + (state >= blank)."""
    S = np.asarray(posts[0]).shape[1]
    bl = blank + S if blank < 0 else blank
    col = lambda st: [s + (1 if s >= bl else 0) for s in st]
    old = states_of(text, k, alphabet)
    rows = [r for r in letter_edits(text, alphabet) if len(r[3]) >= k]
    edits = []
    for r in rows:
        a, d, new = strip_common(old, states_of(r[3], k, alphabet))
        edits.append((a, d, col(new)))
    gain = np.zeros(len(rows))
    total = 0.0
    for post in posts:
        score, ll = rescore(post, col(old), edits, blank)
        gain += np.array(ll) - score
        total += score
    return rows, gain, total


def accept(rows, gain, k, min_gain=0.0, most=None):
    good = [i for i in range(len(rows)) if gain[i] > min_gain]
    good.sort(key=lambda i: (-gain[i], rows[i][1], KINDS.index(rows[i][0]), rows[i][2]))
    taken, seen = [], set()
    for i in good:
        if most is not None and len(taken) >= most:
            break
        if rows[i][3] in seen:                            # the same edited string again (a homopolymer run): the same edit
            continue
        seen.add(rows[i][3])
        if all(abs(rows[i][1] - rows[j][1]) >= k for j in taken):
            taken.append(i)
    return taken


def apply_edits(text, picked):
    for kind, p, c in sorted(picked, key=lambda e: -e[1]):
        text = text[:p] + (c if kind != 'del' else '') + text[p + (0 if kind == 'ins' else 1):]
    return text


def polish(posts, text, k, blank=0, min_gain=0.0, max_rounds=8, most=None, alphabet='ACGT'):
    """-> (polished string, [(round, kind, letter_pos, letter, gain)], rounds that applied something, summed score of the result)."""
    applied, rounds, total = [], 0, None
    for r in range(max_rounds + 1):
        rows, gain, total = gains(posts, text, k, blank, alphabet)
        taken = accept(rows, gain, k, min_gain, most) if r < max_rounds else []
        if not taken:
            break
        applied += [(r, rows[i][0], rows[i][1], rows[i][2], float(gain[i])) for i in taken]
        text = apply_edits(text, [rows[i][:3] for i in taken])
        rounds += 1
    return text, applied, rounds, total


# ---- the cases the CPU and the GPU tests share -------------------------------------------------------------------------------------

TINY_T = (1, 2, 3, 5, 9)
TINY_L = (0, 1, 2, 4)
TINY_M = (0, 1, 2, 8)


def tiny_cases(seed=11, S=5, dtype=np.float64):
    """Every (T, L) of TINY_T x TINY_L as one pair (rows of S random probabilities, blank last) with every (a, d) and m in TINY_M
    new random symbols: -> [(post, seq, [(a, d, new)])]."""
    rng = np.random.default_rng(seed)
    out = []
    for T in TINY_T:
        for L in TINY_L:
            post = rng.uniform(0.05, 1.0, size=(T, S))
            post = (post / post.sum(axis=1, keepdims=True)).astype(dtype)
            seq = rng.integers(0, S - 1, size=L)
            edits = [(a, d, rng.integers(0, S - 1, size=m)) for a in range(L + 1) for d in range(L - a + 1) for m in TINY_M]
            out.append((post, seq, edits))
    return out


def wide_cases(sizes=((65, 300, 120), (65, 40, 12), (1025, 64, 30), (1025, 150, 60))):
    """(post, seq, edits) on S = 65 and 1025, blank last: substitutions, deletions, insertions and longer replacements at the ends
    and inside."""
    rng = np.random.default_rng(23)
    out = []
    for S, T, L in sizes:
        post = rng.uniform(size=(T, S)) * rng.uniform(size=(T, 1))
        post[np.arange(T), rng.integers(0, S, size=T)] += 1.0
        post[:, -1] += 0.5
        post /= post.sum(axis=1, keepdims=True)
        seq = rng.integers(0, S - 1, size=L)
        edits = []
        for a in (0, 1, L // 3, L // 2, L - 2, L - 1, L):
            for d in (0, 1, 3):
                if a + d > L:
                    continue
                for m in (0, 1, 2, 6, 8):
                    edits.append((a, d, rng.integers(0, S - 1, size=m)))
        edits.append((L // 2, 1, seq[L // 2:L // 2 + 1]))         # an identity edit
        out.append((post, seq, edits))
    return out


def planted_case(seed=7, k=3, nletters=40, nrow=120, nread=3, alphabet='ACGT'):
    """A truth of random letters, `nread` float32 posteriors [nrow, 4^k + 1] (blank 0, state s in column s + 1) that spell it -- 0.2 x
    uniform noise, plus 1.0 on the truth's column at sorted random rows and on the blank elsewhere, rows normalised -- and a draft with
    letter 10 substituted, letter 20 deleted and a letter inserted at 30.  -> (truth, draft, [post])"""
    rng = np.random.default_rng(seed)
    truth = ''.join(alphabet[i] for i in rng.integers(0, 4, size=nletters))
    states = states_of(truth, k, alphabet)
    posts = []
    for _ in range(nread):
        post = 0.2 * rng.uniform(size=(nrow, len(alphabet) ** k + 1))
        rows = np.sort(rng.choice(nrow, size=len(states), replace=False))
        post[:, 0] += 1.0
        post[rows, 0] -= 1.0
        post[rows, np.array(states) + 1] += 1.0
        posts.append((post / post.sum(axis=1, keepdims=True)).astype(np.float32))
    other = lambda c: alphabet[(alphabet.index(c) + 1 + int(rng.integers(0, 3))) % 4]
    draft = list(truth)
    draft[10] = other(truth[10])
    ins = alphabet[int(rng.integers(0, 4))]
    draft = draft[:20] + draft[21:30] + [ins] + draft[30:]
    return truth, ''.join(draft), posts


# ---- the kernels' tiers, restated from design/rescore_edits.md 3 and 4 ------------------------------------------------------------

THREADS = 256


def ppt_of(L):
    """States per thread of the lattice kernel: the smallest of 1, 2, .. 32 with 256 ppt >= L + 1."""
    ppt = 1
    while THREADS * ppt < L + 1:
        ppt *= 2
    assert ppt <= 32
    return ppt


def budget_of(max_npos):
    """The lattice kernel a launch gets by its longest sequence: rescore_lattice_kernel<T, 2 / 8 / 32>."""
    return 2 if max_npos < 2 * THREADS else (8 if max_npos < 8 * THREADS else 32)


def ahead_of(ppt):
    """Rows of emissions in flight per thread (fs_ahead)."""
    return 4 if ppt <= 4 else (2 if ppt <= 8 else 1)


def gran_of(S, itemsize):
    """16-byte granules of one staged row: the row's bytes and one more for its alignment."""
    return (S * itemsize + 15) // 16 + 1


def nch_of(gran):
    """Granules per thread of the candidate kernel: rescore_cand_kernel<T, 2 / 5 / 17, true>."""
    per = (gran + THREADS - 1) // THREADS
    return 2 if per <= 2 else (5 if per <= 5 else 17)


def lds_of(gran):
    """Bytes of dynamic LDS of the candidate kernel: two rows.  Above 64 KB the launch raises the limit first."""
    return 2 * 16 * gran


# ---- 1a: every ownership tier through long deletions --------------------------------------------------------------------------------

TIER_L = (255, 256, 511, 512, 1023, 1024, 2047, 2048, 4095, 4096, 8191)      # L + 1 on both sides of every ppt boundary, and the longest
TIER_T = 40


def deletion_edits(L, T, rng, S=65):
    """Edits that leave at most T positions of a sequence of L: a in {0, 1, 10, 30}, a + d in {L, L - 1, L - 5, L - 20}, m in
    {0, 1, 3, 8}.  Column a of F lies with thread 0 or its neighbours, column a + d + 1 of B with the last owning thread."""
    out = []
    for a in (0, 1, 10, 30):
        for end in (L, L - 1, L - 5, L - 20):
            for m in (0, 1, 3, 8):
                if a <= end and a + m + (L - end) <= T:
                    out.append((a, end - a, rng.integers(0, S - 1, size=m)))
    return out


def deletion_cases(seed=53, lengths=TIER_L, T=TIER_T, S=65, dtype=np.float64):
    """One pair of T rows per L of `lengths` (so its own score is -inf) with deletion_edits: -> [(post, seq, edits)]."""
    rng = np.random.default_rng(seed)
    out = []
    for L in lengths:
        post = rng.uniform(0.05, 1.0, size=(T, S))
        post[:, -1] += 2.0
        post = (post / post.sum(axis=1, keepdims=True)).astype(dtype)
        seq = rng.integers(0, S - 1, size=L)
        out.append((post, seq, deletion_edits(L, T, rng, S)))
    return out


# ---- 1b: one diagonal pair per upper tier ------------------------------------------------------------------------------------------

DIAGONAL = ((8, 1100, 1030), (16, 2100, 2050), (32, 4200, 4100))              # (states per thread, T, L)


def boundary_threads(L):
    """A thread of the first, of a middle and of the last owning wave: thread 1, the first thread of a middle wave (its left neighbour
    sits in another wave) and the last thread that owns a state."""
    ppt = ppt_of(L)
    last = L // ppt                                               # (state L is the last one)
    waves = last // 64 + 1
    mid = 64 * (waves // 2) if waves >= 3 else 64
    return [t for t in (1, min(mid, last - 1), last) if 1 <= t <= last]


def diagonal_case(T, L, seed=59, S=65, full=True):
    """A pair whose float32 posterior follows its sequence: uniform noise, +1.0 on seq's column at L sorted random rows, +0.3 on the
    blank, rows normalised (the scaled end state stays far from underflow).  Edits: at a = 0 and at a + d = L, then for each of
    boundary_threads, with first state j0, the columns j0 - 1, j0, j0 + ppt - 1 and j0 + ppt (no further than L) as `a` and as
    `a + d + 1` of consecutive edits, m cycling through 0, 1 and 8, and an identity edit last.  An edit takes 8 new symbols only
    where it deletes 6 or more: every position gained has to be emitted by one of the T - L rows that emit nothing, which lie some
    40 rows apart in the longer pairs, and until then the path runs beside the planted one at about 2^-2 per row; a gain of 8 is
    below 2^-1074 of its row's total, which is 0 in the stored lattices (design/forward_score.md 4), while a gain of 2 is not.
    full = False leaves out the pure insertions at both ends and the two edits per thread that straddle its neighbours.
    -> (post, seq, edits, [(a, a + d + 1) per thread])"""
    rng = np.random.default_rng(seed + L)
    ppt = ppt_of(L)
    seq = rng.integers(0, S - 1, size=L)
    post = rng.uniform(size=(T, S)) * rng.uniform(size=(T, S))
    rows = np.sort(rng.choice(T, size=L, replace=False))
    post[rows, seq] += 1.0
    post[:, -1] += 0.3
    post = (post / post.sum(axis=1, keepdims=True)).astype(np.float32)
    sym = lambda m: rng.integers(0, S - 1, size=m)                # noqa: E731
    edits = [(0, 1, sym(1)), (0, 8, sym(8)), (L - 1, 1, sym(0)), (L - 8, 8, sym(8))]
    if full:
        edits += [(0, 0, sym(1)), (L, 0, sym(1))]
    named = []
    for tid in boundary_threads(L):
        j0 = tid * ppt
        c = [j0 - 1, j0, min(j0 + ppt - 1, L), min(j0 + ppt, L)]
        spans = [(c[0], c[1]), (c[1], c[2])] + ([(c[2], c[3])] if c[2] < c[3] else [])          # (a, a + d + 1)
        if full:
            spans += [(j0 - 3, j0 - 1)] + ([(j0 + ppt, j0 + ppt + 2)] if j0 + ppt + 2 <= L else [])
        named.append(spans)
        for i, (a, b1) in enumerate(spans):
            d, m = b1 - 1 - a, (0, 1, 8)[(i + tid) % 3]
            edits.append((a, d, sym(8 if d >= 6 else min(m, 1))))
    mid = L // 2
    edits.append((mid, 1, seq[mid:mid + 1]))                      # an identity edit
    return post, seq, edits, named


# ---- 2: every staging tier -------------------------------------------------------------------------------------------------------------

STAGE_S = {np.dtype(np.float32): (2044, 2045, 5116, 5117, 8188, 8189, 8192),
           np.dtype(np.float64): (1022, 1023, 2558, 2559, 4095, 8192)}
STAGE_T, STAGE_L = 12, 6


def row_mis(t, S, itemsize, lead=0):
    """Where row t of packed rows of S values begins inside its 16-byte granule, in values, `lead` values behind an aligned address."""
    return ((lead + t * S) * itemsize % 16) // itemsize


def edge_columns(S, itemsize, ms):
    """The columns of a row that begins `ms` values into a granule at which staging changes hands: 0 and S - 1, the last value of
    the row's first granule and the first of its last, and both sides of every granule 256 k (another register of the thread)."""
    per = 16 // itemsize
    ngran = (ms + S + per - 1) // per
    cols = {0, S - 1, min(per - ms - 1, S - 1), max((ngran - 1) * per - ms, 0)}
    for k in range(1, (ngran - 1) // THREADS + 1):
        cols |= {THREADS * k * per - ms - 1, THREADS * k * per - ms}
    return sorted(c for c in cols if 0 <= c < S)


def planted_columns(S, itemsize):
    """edge_columns for every alignment a row can have, and their neighbours."""
    per = 16 // itemsize
    cols = set()
    for ms in range(per):
        for c in edge_columns(S, itemsize, ms):
            cols |= {c - 1, c, c + 1}
    return sorted(c for c in cols if 0 <= c < S)


def stage_case(S, dtype, seed=61):
    """T = 12 rows of S distinct random probabilities, L = 6; the sequence and the new symbols of the edits run through
    planted_columns (every one is used; the blank is the last column).  -> (post, seq, edits)"""
    dtype = np.dtype(dtype)
    rng = np.random.default_rng(seed + S)
    T, L = STAGE_T, STAGE_L
    post = rng.uniform(0.05, 1.0, size=(T, S))
    cols = np.array(planted_columns(S, dtype.itemsize))
    post[:, cols] += 40.0 * rng.uniform(0.5, 1.0, size=(T, len(cols)))        # (keeps the planted columns' share of a wide row up)
    post = (post / post.sum(axis=1, keepdims=True)).astype(dtype)
    order = rng.permutation(cols)
    seq = order[:L].copy()
    rest = order[L:]
    edits = []
    for i in range(0, len(rest), 8):
        new = rest[i:i + 8]
        a = (i // 8) % (L - 1)
        d = 2 if a + 2 <= L else L - a
        edits.append((a, d, new))                                 # L - 2 + 8 = T positions at the most
    edits += [(0, 0, order[:3]), (L, 0, order[-3:]), (2, 3, []), (0, L, order[3:11]), (L - 1, 1, seq[L - 1:])]
    return post, seq, edits


# ---- 3: few rows ----------------------------------------------------------------------------------------------------------------------

FEW_L = (256, 511, 1023, 2047, 2048, 4095, 8191)                              # 2, 2, 4, 8, 16, 16 and 32 states per thread
FEW_T = (0, 1, 2, 3, 4, 5)                                                    # below, at and above fs_ahead = 1, 2 and 4


def few_rows_edits(L, T, rng, S=65):
    """Edits that leave at most T positions (finite) or T + 1 (-inf): everything deleted, everything replaced by T and by T + 1 new
    symbols, and a kept head of `a` and a kept tail of `r` positions around m new ones."""
    sym = lambda m: rng.integers(0, S - 1, size=m)                # noqa: E731
    out = [(0, L, sym(0)), (0, L, sym(T)), (0, L, sym(T + 1))]
    for a in (0, 1, 2):
        for r in (0, 1, 2):
            for m in sorted({0, 1, T - a - r, T + 1 - a - r}):
                if 0 <= m <= MAX_NEW and a + r + m <= T + 1 and a + r > 0:
                    out.append((a, L - a - r, sym(m)))
    return out


def few_rows_cases(seed=67, lengths=FEW_L, rows=FEW_T, S=65, dtype=np.float64):
    """Every (T, L) of rows x lengths as one pair, and T = 0 with L = 0 and the edit (0, 0, []) last: -> [(post, seq, edits)]."""
    rng = np.random.default_rng(seed)
    out = []
    for L in lengths:
        for T in rows:
            post = rng.uniform(0.05, 1.0, size=(T, S))
            post = (post / post.sum(axis=1, keepdims=True)).astype(dtype)
            out.append((post, rng.integers(0, S - 1, size=L), few_rows_edits(L, T, rng, S)))
    out.append((np.zeros((0, S), dtype=dtype), np.zeros(0, dtype=np.int64), [(0, 0, np.zeros(0, dtype=np.int64))]))
    return out


# ---- 4: the exponent sum ----------------------------------------------------------------------------------------------------------------

SCALED_SIZES = ((65, 300, 120), (65, 40, 12))


def scaled_cases(variant, seed=71):
    """wide_cases' two S = 65 pairs with row t multiplied by 2^-k_t (exact): `random` draws k_t from 0 .. 200, `alternate` takes 0
    and 600 on neighbouring rows.  -> [(scaled post, seq, edits, unscaled post, k)]"""
    rng = np.random.default_rng(seed)
    out = []
    for post, seq, edits in wide_cases(SCALED_SIZES):
        T = post.shape[0]
        k = rng.integers(0, 201, size=T) if variant == "random" else 600 * (np.arange(T) % 2)
        assert variant in ("random", "alternate")
        out.append((np.ldexp(post, -k[:, None]), seq, edits, post, k))
    return out
