"""The forward score of an edited sequence from the stored lattices of the unedited one, restated in plain float64 loops from
design/rescore_edits.md for this repository's tests (nothing of the device code is imported).

    F_0 = e_0      F_t[j]     = F_{t-1}[j] p_t[blank] + F_{t-1}[j-1] p_t[seq[j-1]]
    B_T = e_L      B_{t-1}[j] = B_t[j] p_t[blank] + B_t[j+1] p_t[seq[j]]
    edit (a, d, c[0..m)):  g_t[0] = F_t[a], g_0[i > 0] = 0, g_t[i] = g_{t-1}[i] p_t[blank] + g_{t-1}[i-1] p_t[c[i-1]]
    a + d < L:  Z' = sum_{t=0}^{T-1} g_t[m] p_{t+1}[seq[a+d]] B_{t+1}[a+d+1]          a + d = L:  Z' = g_T[m]

Rows are scaled by the exact power of two of the previous row's total (integer running exponents EF_t, EB_t), g with its row's
EF_t - EF_{t-1}; the terms of the sum carry EF_t + EB_{t+1} and are added in ascending t as (mantissa, exponent).
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
                term = (g[m] * post[t, seq[a + d]]) * B[t + 1, a + d + 1]
                e = EF[t] + EB[t + 1]
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
