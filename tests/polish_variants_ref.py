"""CPU model of csrc/polish_variants.hip, plain loops written from design/polish_variants.md section 1: which variants of a sorted list
are a window's candidates and in what order, their (start, ndel, new) triples by spelling out both strings and calling bio.edit_states,
the posterior columns, the sum per variant and strand, and the repeat-unit proposer.  Pure Python and numpy; it shares no arithmetic
with the kernels.  tests/test_polish_variants_ref.py pins it with no GPU, tests/test_gpu_polish_variants.py compares the kernels with
it integer for integer."""
import numpy as np

from sloika_amd import bio
from tests.polish_genome_ref import column, revcomp, window_columns, window_string

OK, CONTIG, SPAN, NDEL, ALT, EMPTY, SAME = 0, -1, -2, -3, -4, -5, -6
MAX_NEW = 8


def max_alt(klen):
    return MAX_NEW - klen + 1


def sort_variants(variants):
    """variants: [(contig offset, pos, ndel, alt)] -> (the list sorted by (offset, pos), stably; order[s] = the caller's number)."""
    order = sorted(range(len(variants)), key=lambda i: (variants[i][0], variants[i][1]))
    return [variants[i] for i in order], order


def variant_status(genome, contig_off, variant, klen):
    """The status of one variant (contig offset, pos, ndel, alt) of the packed genome string; contig_off: the contigs' starts and G."""
    off, pos, ndel, alt = variant
    if off not in list(contig_off[:-1]):
        return CONTIG
    n = contig_off[list(contig_off[:-1]).index(off) + 1] - off
    if ndel < 0:
        return NDEL
    if pos < 0 or pos + ndel > n:
        return SPAN
    if len(alt) > max_alt(klen):
        return ALT
    if ndel + len(alt) < 1:
        return EMPTY
    if genome[off + pos:off + pos + ndel] == alt:
        return SAME
    return OK


def window_candidates(variants, status, window, klen, margin):
    """The sorted-list numbers of a window's candidates, in the kernel's order: ascending in a '+' window, descending in a '-' one."""
    off, w0, w1, minus = window
    n = w1 - w0
    out = []
    if n < klen:
        return out
    for v, (voff, pos, ndel, alt) in enumerate(variants):
        if status[v] != OK or voff != off:
            continue
        if w0 + margin <= pos and pos + ndel <= w1 - margin and n - ndel + len(alt) - klen + 1 >= 1:
            out.append(v)
    return out[::-1] if minus else out


def window_edit(window, variant):
    """(u, ndel, alt) in the window's own coordinates and letters."""
    off, w0, w1, minus = window
    _, pos, ndel, alt = variant
    return (w1 - pos - ndel, ndel, revcomp(alt)) if minus else (pos - w0, ndel, alt)


def states(s, klen):
    """k-mer states of a string over ACGT plus other letters: a k-mer with another letter is a state of its own (-1 - position would
    do; its letters' codes keep equal strings equal)."""
    code = {'A': 0, 'C': 1, 'G': 2, 'T': 3}
    return [sum(code.get(c, 4 + ord(c)) * 1000 ** (klen - 1 - d) for d, c in enumerate(s[i:i + klen])) for i in range(len(s) - klen + 1)]


def triple(s, u, ndel, alt, klen):
    """(start, ndel, the new k-mers as strings) by spelling out both strings: bio.edit_states of the two k-mer lists."""
    t = s[:u] + alt + s[u + ndel:]
    a, d, new = bio.edit_states(states(s, klen), states(t, klen))
    return a, d, [t[a + x:a + x + klen] for x in range(len(new))]


def variant_edits(genome, contig_off, windows, variants, klen, blank, margin):
    """windows: [(contig offset, w0, w1, minus)]; variants: the SORTED list.  -> dict of the arrays the kernels write (cand_var: numbers
    of the sorted list) and var_status."""
    status = [variant_status(genome, contig_off, v, klen) for v in variants]
    pair, start, ndel, nnew, new, var, seq, ncand, nkmer = [], [], [], [], [], [], [], [0], [0]
    for b, win in enumerate(windows):
        s = window_string(genome, *win)
        cands = window_candidates(variants, status, win, klen, margin)
        ncand.append(len(cands))
        cols = window_columns(s, klen, blank) if len(s) >= klen else []
        nkmer.append(len(cols))
        seq.extend(cols)
        for v in cands:
            a, d, kmers = triple(s, *window_edit(win, variants[v]), klen)
            pair.append(b)
            start.append(a)
            ndel.append(d)
            nnew.append(len(kmers))
            new.extend(column(km, blank) for km in kmers)
            var.append(v)
    return dict(cand_off=np.cumsum(ncand).astype(np.int64), pos_off=np.cumsum(nkmer).astype(np.int64),
                cand_pair=np.array(pair, dtype=np.int32), cand_start=np.array(start, dtype=np.int32),
                cand_ndel=np.array(ndel, dtype=np.int32), cand_new_off=np.concatenate([[0], np.cumsum(nnew)]).astype(np.int64),
                cand_new=np.array(new, dtype=np.int32), cand_var=np.array(var, dtype=np.int32), seq=np.array(seq, dtype=np.int32),
                var_status=np.array(status, dtype=np.int32))


def sum_variant_gains(score, ll_edit, cand_read, cand_var, read_minus, V, tables=None):
    """The six tables, each cell a Python loop over its candidates in read order (ties: as they come)."""
    if tables is None:
        tables = (np.zeros(V), np.zeros(V, dtype=np.int32), np.zeros(V, dtype=np.int32), np.zeros((V, 2)), np.zeros((V, 2), dtype=np.int32),
                  np.zeros((V, 2), dtype=np.int32))
    gain, support, pro, gs, ss, ps = [t.copy() for t in tables]
    for i in sorted(range(len(cand_var)), key=lambda i: (int(cand_var[i]), int(cand_read[i]))):
        v, r = int(cand_var[i]), int(cand_read[i])
        if v < 0 or v >= V:
            continue
        l, s, k = float(ll_edit[i]), float(score[r]), 1 if read_minus[r] else 0
        if l != l or s != s:
            gain[v] = np.nan
            gs[v, k] = np.nan
        elif np.isfinite(l) and np.isfinite(s):
            d = l - s
            gain[v] = gain[v] + d
            gs[v, k] = gs[v, k] + d
            support[v] += 1
            ss[v, k] += 1
            if d > 0:
                pro[v] += 1
                ps[v, k] += 1
    return gain, support, pro, gs, ss, ps


def repeat_variants(genome, contig_off, klen, lo=None, hi=None, max_unit=4, max_change=2, min_copies=2):
    """The proposals of the packed positions [lo, hi): [(contig offset, pos, ndel, alt)] in order."""
    lo, hi = 0 if lo is None else lo, contig_off[-1] if hi is None else hi
    out = []
    for ci in range(len(contig_off) - 1):
        off = contig_off[ci]
        c = genome[off:contig_off[ci + 1]]
        n = len(c)
        for p in range(n):
            if not lo <= off + p < hi:
                continue
            for u in range(1, max_unit + 1):
                if p + 2 * u > n or any(c[p + i] != c[p + i + u] for i in range(u)):
                    continue
                if p > 0 and c[p - 1] == c[p - 1 + u]:
                    continue
                unit = c[p:p + u]
                if any(unit == unit[:d] * (u // d) for d in range(1, u) if u % d == 0):
                    continue                                       # (not primitive: a shorter unit spells it)
                l = u
                while p + l < n and c[p + l] == c[p + l - u]:
                    l += 1
                if any(ch not in 'ACGT' for ch in c[p:p + l]):
                    continue
                copies = l // u
                if copies < max(min_copies, 2):
                    continue
                for cnt in range(1, max_change + 1):
                    if u * cnt != 1 and cnt <= copies - 1:
                        out.append((off, p, u * cnt, ''))
                for cnt in range(1, max_change + 1):
                    if u * cnt != 1 and u * cnt <= max_alt(klen):
                        out.append((off, p, 0, unit * cnt))
    return out


# ---- planted repeats -----------------------------------------------------------------------------------------------------------------

#: truth coordinates: (AC)x6, a run of seven A, and where the draft carries two letters too many
REPEAT_AC, REPEAT_RUN, REPEAT_EXTRA = (150, 162), (300, 307), 450


def planted_repeats(seed=5, k=3, nletters=600):
    """tests/polish_genome_ref.planted_genome's construction with repeat errors: a truth of `nletters` random letters that holds (AC)x6
    at REPEAT_AC and seven A at REPEAT_RUN; 12 float32 posteriors that each spell their own window of it (SAMPLE_WINDOWS, the odd ones
    as the reverse complement) over twice as many rows as the window has k-mers, a read that maps nowhere and read 0's window again.
    The draft lacks one AC unit, has the run two letters short, and has 'GT' put in front of truth letter REPEAT_EXTRA.
    -> dict(truth, draft, post, steps, texts, k, fixes: the three true fixes as (pos, ndel, alt) on the draft)"""
    from tests.polish_genome_ref import SAMPLE_WINDOWS
    rng = np.random.default_rng(seed)
    letters = [('ACGT')[i] for i in rng.integers(0, 4, size=nletters)]
    a, b = REPEAT_AC
    letters[a - 1], letters[b] = 'G', 'T'
    letters[a:b] = 'AC' * ((b - a) // 2)
    a, b = REPEAT_RUN
    letters[a - 1], letters[b] = 'C', 'G'
    letters[a:b] = 'A' * (b - a)
    x = REPEAT_EXTRA
    letters[x - 4:x + 6] = 'GATCACTGCA'                           # ... G A T C [G T] A C T G C A ...: the extra letters lengthen no tract and
                                                                 # stand beside none (a random tandem repeat next to them is a third repeat error)
    truth = ''.join(letters)
    draft = truth[:REPEAT_AC[0]] + truth[REPEAT_AC[0] + 2:REPEAT_RUN[0]] + truth[REPEAT_RUN[0] + 2:x] + 'GT' + truth[x:]
    fixes = [(REPEAT_AC[0], 0, 'AC'), (REPEAT_RUN[0] - 2, 0, 'AA'), (x - 4, 2, '')]
    texts = [truth[s:e] if i % 2 == 0 else revcomp(truth[s:e]) for i, (s, e) in enumerate(SAMPLE_WINDOWS)]
    texts.append(''.join('ACGT'[i] for i in rng.integers(0, 4, size=260)))
    texts.append(texts[0])
    S = 4 ** k + 1
    steps = np.array([2 * (len(t) - k + 1) for t in texts], dtype=np.int32)
    post = rng.uniform(size=(int(steps.max()), len(texts), S)).astype(np.float32) * np.float32(0.2)
    post[:, :, 0] += 1.0
    for r, t in enumerate(texts):
        st = np.array([sum('ACGT'.index(c) * 4 ** (k - 1 - i) for i, c in enumerate(t[p:p + k])) for p in range(len(t) - k + 1)])
        rows = np.sort(rng.choice(int(steps[r]), size=len(st), replace=False))
        post[rows, r, 0] -= 1.0
        post[rows, r, st + 1] += 1.0
    post /= post.sum(axis=2, keepdims=True)
    return dict(truth=truth, draft=draft, post=post, steps=steps, texts=texts, k=k, fixes=fixes)
