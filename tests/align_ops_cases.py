"""Pairs for the traceback tests (tests/test_gpu_align_traceback.py, tests/test_align_ops_host.py), all small enough for the
plain-loop oracle: pairs with an exact number of planted indels (the band's width W = I + D + 1), pairs whose path touches
either edge of its band, and two-letter pairs on which the tie rules decide the path."""
import numpy as np

from tests.align_cases import random_seq

#: widths planted under the default scores (1, 2, 2, 1): single-letter indels, six exact letters apart
WIDTHS = (1, 2, 63, 64, 65, 129)
#: scores under which a long gap is cheap (a gap of k letters costs k, a match earns 5), so that wide bands fit short pairs ...
WIDE_SCORES = (5, 4, 0, 1)
#: ... and the widths planted under them: on both sides of the kernel's layout switches (4, 8, 12, 16 diagonals per lane at 256,
#: 512 and 768 diagonals), and its widest band
WIDE_WIDTHS = (256, 257, 300, 512, 513, 768, 769, 1024)
TIE_SCORES = ((1, 1, 0, 1), (1, 0, 0, 1))


def _other(rs, ch):
    return 'ACGT'[('ACGT'.index(ch) + rs.randint(1, 4)) % 4]


def planted(rs, kinds, run=1, gap=5, flank=30):
    """-> (query, reference): `flank` exact letters, then for every entry of `kinds` ('I' / 'D') a run of `run` letters that only
    the query / only the reference has, followed by `gap` exact letters, then `flank` exact letters.  A run's letters differ from
    the letter in front of them and from the one behind on the other side, so that no shorter gap explains the pair."""
    q, r = [], []
    s = random_seq(rs, flank)
    q.append(s)
    r.append(s)
    for kind in kinds:
        nxt = random_seq(rs, gap)
        extra = ''.join(_other(rs, nxt[0]) for _ in range(run))
        (q if kind == 'I' else r).append(extra)
        q.append(nxt)
        r.append(nxt)
    s = random_seq(rs, flank)
    q.append(s)
    r.append(s)
    return ''.join(q), ''.join(r)


def width_pair(W, seed=0):
    """A pair with W - 1 single-letter indels, four insertions and four deletions in turn, under the default scores."""
    rs = np.random.RandomState(1000 + 7 * W + seed)
    return planted(rs, ['ID'[(k // 4) % 2] for k in range(W - 1)], gap=6)


def wide_pair(W, seed=0):
    """A pair with W - 1 indel letters in runs of up to 50, under WIDE_SCORES.  The runs are 'N' in the query and 'K' in the
    reference: cheap gaps would otherwise align random extra letters with each other."""
    rs = np.random.RandomState(5000 + 7 * W + seed)
    left, q, r = W - 1, [], []
    s = random_seq(rs, 30)
    q.append(s)
    r.append(s)
    k, nruns = 0, (W + 48) // 50
    while left > 0:                                        # the insertions first: the path runs far from the start's diagonal
        run = min(50, left)
        nxt = random_seq(rs, 14)
        (q if k < nruns // 2 else r).append(('N' if k < nruns // 2 else 'K') * run)
        q.append(nxt)
        r.append(nxt)
        left -= run
        k += 1
    s = random_seq(rs, 30)
    q.append(s)
    r.append(s)
    return ''.join(q), ''.join(r)


def edge_pairs(n_ins=9, n_del=7):
    """Two pairs: all insertions before all deletions (the path reaches diagonal +I), and the other way round (-D)."""
    first = planted(np.random.RandomState(61), ['I'] * n_ins + ['D'] * n_del)
    second = planted(np.random.RandomState(62), ['D'] * n_del + ['I'] * n_ins)
    return first, second


def tie_pairs(count=40, seed=77):
    """Pairs over a two-letter alphabet: the reference 30..90 random letters, the query a stretch of it with a fifth of its
    letters substituted, doubled or dropped.  Equal scores are everywhere: the priorities choose the path."""
    rs = np.random.RandomState(seed)
    out = []
    for _ in range(count):
        m = rs.randint(30, 91)
        ref = ''.join('AC'[k] for k in rs.randint(0, 2, size=m))
        lo = rs.randint(0, m // 4 + 1)
        hi = m - rs.randint(0, m // 4 + 1)
        q = []
        for ch in ref[lo:hi]:
            u = rs.uniform()
            if u < 0.07:
                q.append('A' if ch == 'C' else 'C')
            elif u < 0.14:
                q.append(ch + 'AC'[rs.randint(0, 2)])
            elif u < 0.2:
                pass
            else:
                q.append(ch)
        out.append((''.join(q), ref))
    return out
