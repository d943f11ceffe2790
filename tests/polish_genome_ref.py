"""CPU model of csrc/polish_genome.hip, plain loops written from design/polish_genome.md section 1: the windows of mapped reads and their
centre lines, the single-letter candidates of a window with their (start, ndel, new) triples, and the sum of the reads' gains on genome
coordinates.  Pure Python and numpy: tests/test_polish_genome_ref.py pins it with no GPU, tests/test_gpu_polish_genome.py compares the
kernels with it integer for integer."""
import numpy as np

DONE, SKIPPED = 0, 1
BAD_SPAN, BAD_COUNT, BAD_SUM, OPS, POSITION, BAD_CODE, CODE_COUNT, PATH, MOVE_ROW, SHORT, FEW_ROWS, CENTER = range(-1, -13, -1)
MAX_LEN = 65535
KIND_BITS = {'sub': 1, 'del': 2, 'ins': 4}
KIND_NAMES = ('sub', 'del', 'ins')
COMP = {'A': 'T', 'C': 'G', 'G': 'C', 'T': 'A'}


def kinds_mask(kinds):
    return sum(KIND_BITS[k] for k in set(kinds))


def revcomp(s):
    return ''.join(COMP.get(c, c) for c in reversed(s))


def window_string(genome, off, w0, w1, minus):
    """The window's own letters: genome[off + w0 : off + w1], reverse-complemented for '-'."""
    s = genome[off + w0:off + w1]
    return revcomp(s) if minus else s


# ---- candidates ----------------------------------------------------------------------------------------------------------------------

def per_position(n, klen, mask):
    return (3 if mask & 1 else 0) + (1 if (mask & 2) and n - 1 >= klen else 0) + (4 if mask & 4 else 0)


def count(n, klen, mask, margin):
    lo, hi = margin, n - margin
    if n < klen or hi < lo:
        return 0
    return (hi - lo) * per_position(n, klen, mask) + (4 if mask & 4 else 0)


def window_edits(s, klen, mask, margin):
    """(kind, u, letter) of every candidate of the window string s in the kernel's order: positions margin .. n - margin - 1 ascending,
    at each the substitutions in alphabet order without the letter that stands there, the deletion (when n - 1 >= klen), the
    insertions in front of it in alphabet order; then the insertions in front of position n - margin."""
    n = len(s)
    lo, hi = margin, n - margin
    out = []
    if n < klen or hi < lo:
        return out
    for u in range(lo, hi + 1):
        if u < hi:
            if mask & 1:
                out.extend(('sub', u, c) for c in 'ACGT' if c != s[u])
            if (mask & 2) and n - 1 >= klen:
                out.append(('del', u, ''))
        if mask & 4:
            out.extend(('ins', u, c) for c in 'ACGT')
    return out


def edited(s, kind, u, c):
    return s[:u] + c + s[u + 1:] if kind == 'sub' else s[:u] + s[u + 1:] if kind == 'del' else s[:u] + c + s[u:]


def triple(s, kind, u, c, klen):
    """(start, ndel, number of new k-mers): common prefix of the k-mer lists, then common suffix of the rest, from the letters alone.
    dF: the first letter at which the two strings differ read from the front; dB: the last letter of s at which they differ read from
    the back; None when they agree as far as the shorter goes.  In a run of equal letters both are found by walking along the run."""
    n = len(s)
    if kind == 'sub':
        dF = dB = u
        n2 = n
    elif kind == 'del':
        x = u
        while x + 1 < n and s[x + 1] == s[u]:
            x += 1
        dF = None if x == n - 1 else x
        x = u
        while x >= 1 and s[x - 1] == s[u]:
            x -= 1
        dB = None if x == 0 else x
        n2 = n - 1
    else:
        x = u
        while x < n and s[x] == c:
            x += 1
        dF = None if x == n else x
        x = u
        while x >= 1 and s[x - 1] == c:
            x -= 1
        dB = None if x == 0 else x - 1
        n2 = n + 1
    nold, nnew = n - klen + 1, n2 - klen + 1
    nmin = min(nold, nnew)
    pre = nmin if dF is None else min(max(dF - klen + 1, 0), nmin)
    rest = nmin - pre
    suf = rest if dB is None else min(max(nold - 1 - dB, 0), rest)
    return pre, nold - pre - suf, nnew - pre - suf


def column(kmer, blank):
    """The posterior column of a k-mer string; -1 when a letter is none of A C G T."""
    s = 0
    for ch in kmer:
        if ch not in 'ACGT':
            return -1
        s = 4 * s + 'ACGT'.index(ch)
    return s + (1 if s >= blank else 0)


def window_columns(s, klen, blank):
    return [column(s[j:j + klen], blank) for j in range(len(s) - klen + 1)]


def forward_edit(n, minus, kind, u, c):
    """(forward position within the window's span, forward letter) of a window edit."""
    if not minus:
        return u, c
    return (n - u if kind == 'ins' else n - 1 - u), COMP.get(c, c)


def slot_of(kind, fletter, fdraft):
    if kind == 'del':
        return 3
    fl = 'ACGT'.index(fletter)
    if kind == 'ins':
        return 4 + fl
    fd = 'ACGT'.index(fdraft) if fdraft in 'ACGT' else -1
    return min(fl - (1 if fd >= 0 and fl > fd else 0), 2)


def letter_edits(genome, windows, klen, blank, mask, margin):
    """windows: [(contig offset, w0, w1, minus)] over the packed genome string.  -> dict of the arrays the kernels write: cand_off,
    pos_off int64 [nwin + 1]; cand_pair, cand_start, cand_ndel int32; cand_new_off int64; cand_new int32; cand_edit int64; seq int32."""
    pair, start, ndel, nnew, new, edit, seq, ncand, nkmer = [], [], [], [], [], [], [], [0], [0]
    for b, (off, w0, w1, minus) in enumerate(windows):
        s = window_string(genome, off, w0, w1, minus)
        n = len(s)
        cands = window_edits(s, klen, mask, margin)
        assert len(cands) == count(n, klen, mask, margin)
        ncand.append(len(cands))
        cols = window_columns(s, klen, blank) if n >= klen else []
        nkmer.append(len(cols))
        seq.extend(cols)
        for kind, u, c in cands:
            a, d, m = triple(s, kind, u, c, klen)
            t = edited(s, kind, u, c)
            fu, fc = forward_edit(n, minus, kind, u, c)
            pair.append(b)
            start.append(a)
            ndel.append(d)
            nnew.append(m)
            new.extend(column(t[a + x:a + x + klen], blank) for x in range(m))
            edit.append(8 * (off + w0 + fu) + slot_of(kind, fc, genome[off + w0 + fu] if kind == 'sub' else ''))
    return dict(cand_off=np.cumsum(ncand).astype(np.int64), pos_off=np.cumsum(nkmer).astype(np.int64),
                cand_pair=np.array(pair, dtype=np.int32), cand_start=np.array(start, dtype=np.int32),
                cand_ndel=np.array(ndel, dtype=np.int32), cand_new_off=np.concatenate([[0], np.cumsum(nnew)]).astype(np.int64),
                cand_new=np.array(new, dtype=np.int32), cand_edit=np.array(edit, dtype=np.int64), seq=np.array(seq, dtype=np.int32))


def edit_of(cand_edit):
    """(packed position, kind, slot) of a cand_edit value."""
    p, slot = divmod(int(cand_edit), 8)
    return p, ('sub' if slot < 3 else 'del' if slot == 3 else 'ins'), slot


# ---- windows -------------------------------------------------------------------------------------------------------------------------

def moves_of_path(path, klen):
    """Letters each called k-mer emits under always_move: klen for the first, then the smallest shift 1 .. klen - 1 whose overlap
    agrees, else klen (csrc/bases.hip)."""
    out = [klen]
    for s1, s2 in zip(path[:-1], path[1:]):
        mv = klen
        for sh in range(1, klen):
            if s1 % 4 ** (klen - sh) == s2 // 4 ** sh:
                mv = sh
                break
        out.append(mv)
    return out


def read_window(path, move_row, nrow, qlen, ldq, row, codes, ops_len, minus, wstart, coff, rlen, G, klen, center_cap, keep=1, tb_status=0):
    """One read.  row: the nine fields of its alignment (window coordinates), codes: its columns in query order, ops_len: the length
    of its slice of the column buffer.  -> (status, (r0, r1), (w0, w1), center) with None for what a refused read does not get."""
    none = (None, None, None)
    if not keep or tb_status != 0:
        return (SKIPPED,) + none
    _, qs, qe, rs, re, nm, nx, ni, nd = [int(v) for v in row]
    if qlen < 0 or qlen > MAX_LEN or qlen > ldq or rlen < 0 or rlen > MAX_LEN or qs < 0 or qe < qs or qe > qlen or rs < 0 or re < rs \
            or re > rlen:
        return (BAD_SPAN,) + none
    if min(nm, nx, ni, nd) < 0:
        return (BAD_COUNT,) + none
    if nm + nx + ni != qe - qs or nm + nx + nd != re - rs:
        return (BAD_SUM,) + none
    ncol = nm + nx + ni + nd
    if ops_len != ncol:
        return (OPS,) + none
    if wstart < 0 or wstart + rlen > G or coff < 0 or coff > wstart:
        return (POSITION,) + none
    codes = [int(c) for c in codes[:ncol]]
    if any(c > 3 for c in codes):
        return (BAD_CODE,) + none
    if [codes.count(k) for k in range(4)] != [nm, nx, ni, nd]:
        return (CODE_COUNT,) + none
    n = len(path)
    if n < 1 or nrow < 1 or any(s < 0 or s >= 4 ** klen for s in path):
        return (PATH,) + none
    bad_row = any(r < 0 or r >= nrow for r in move_row[:n]) or any(a > b for a, b in zip(move_row[:n - 1], move_row[1:n]))
    letter_row = []
    for mv, r in zip(moves_of_path(path, klen), move_row):
        letter_row.extend([r] * mv)
    if len(letter_row) != qlen:
        return (PATH,) + none
    if bad_row:
        return (MOVE_ROW,) + none
    L = re - rs - klen + 1
    if L < 1:
        return (SHORT,) + none
    if qe <= qs:
        return (FEW_ROWS,) + none
    # the row of every window letter: its column's query letter, or the next query letter for a deletion (the last for a trailing one)
    wrow, i = [], qs
    for c in codes:
        if c in (0, 1, 3):
            wrow.append(letter_row[min(i, qe - 1)])
        if c in (0, 1, 2):
            i += 1
    r0 = wrow[klen - 1]                                           # the first k-mer of the window is whole
    r1 = nrow                                                    # the first row above those of the last aligned letter
    for x in range(qe, qlen):
        if letter_row[x] > letter_row[qe - 1]:
            r1 = letter_row[x]
            break
    Tp = r1 - r0
    if Tp < L:
        return (FEW_ROWS,) + none
    if center_cap < Tp + 1:
        return (CENTER,) + none
    center = np.zeros(Tp + 1, dtype=np.int32)
    for j, r in enumerate(wrow):
        if j >= klen - 1 and 1 <= r - r0 + 1 <= Tp:
            center[r - r0 + 1] += 1
    center = np.cumsum(center).astype(np.int32)
    if minus:
        w0, w1 = wstart + (rlen - re) - coff, wstart + (rlen - rs) - coff
    else:
        w0, w1 = wstart + rs - coff, wstart + re - coff
    return DONE, (r0, r1), (w0, w1), center


def band_lo(center, npos, width):
    """decode.band_lo on the host; None when the result is no valid band."""
    lo = np.maximum.accumulate(np.clip(np.asarray(center, dtype=np.int64) - width // 2, 0, max(0, npos + 1 - width)))
    return lo if lo[0] == 0 and lo[-1] + width > npos else None


# ---- sum -----------------------------------------------------------------------------------------------------------------------------

def sum_gains(score, ll_edit, cand_pair, cand_edit, region_start, P, gain=None, support=None):
    """gain [P][8] float64, support [P][8] int32: per cell the candidates in read order (ties: as they come), ll_edit - score added
    one after the other when both are finite; a NaN of either makes the cell NaN.  Continues from gain / support when given."""
    gain = np.zeros((P, 8), dtype=np.float64) if gain is None else gain.copy()
    support = np.zeros((P, 8), dtype=np.int32) if support is None else support.copy()
    order = sorted(range(len(cand_edit)), key=lambda i: (int(cand_edit[i]), int(cand_pair[i])))
    for i in order:
        cell = int(cand_edit[i]) - 8 * region_start
        if cand_edit[i] < 0 or cell < 0 or cell >= 8 * P:
            continue
        l, s = float(ll_edit[i]), float(score[cand_pair[i]])
        p, k = divmod(cell, 8)
        if l != l or s != s:
            gain[p, k] = np.nan
        elif np.isfinite(l) and np.isfinite(s):
            gain[p, k] = gain[p, k] + (l - s)
            support[p, k] += 1
    return gain, support


# ---- a planted read ------------------------------------------------------------------------------------------------------------------

def planted_read(seed, nwin=60, klen=3, clip=(4, 5), rlen_pad=(7, 3), minus=False, wstart=11, coff=5, whole=False):
    """A call planted on a window: the window's letters with one mismatch, one inserted and one deleted letter, `clip` unaligned letters
    at either end (none when `whole`), inside a mapping window with `rlen_pad` more letters at either end.  -> dict with what
    read_window takes, and `planted`: per called k-mer (i >= 0) the window k-mers passed once it is entered, None in the clips."""
    rng = np.random.RandomState(seed)
    win = ''.join('ACGT'[v] for v in rng.randint(0, 4, nwin))
    sub_at, ins_at, del_at = nwin // 4, nwin // 2, (3 * nwin) // 4
    codes, called, wof = [], [], []                              # wof: the window letter a called letter stands for
    for x, ch in enumerate(win):
        if x == del_at:
            codes.append(3)
            continue
        if x == ins_at:
            codes.append(2)
            called.append('ACGT'[rng.randint(0, 4)])
            wof.append(x - 1)
        if x == sub_at:
            codes.append(1)
            called.append('ACGT'[('ACGT'.index(ch) + 1) % 4])
        else:
            codes.append(0)
            called.append(ch)
        wof.append(x)
    front, back = (0, 0) if whole else clip
    head = ['ACGT'[v] for v in rng.randint(0, 4, front)]
    tail = ['ACGT'[v] for v in rng.randint(0, 4, back)]
    letters = ''.join(head + called + tail)
    qs, qe = front, front + len(called)
    path = [sum('ACGT'.index(c) * 4 ** (klen - 1 - d) for d, c in enumerate(letters[i:i + klen])) for i in range(len(letters) - klen + 1)]
    move_row = np.cumsum(rng.randint(1, 4, len(path))).astype(np.int32) - 1
    move_row -= move_row[0] if whole else 0
    nrow = int(move_row[-1]) + 3
    rs, re = rlen_pad[0], rlen_pad[0] + nwin
    rlen = re + rlen_pad[1]
    row = [50, qs, qe, rs, re, codes.count(0), codes.count(1), codes.count(2), codes.count(3)]
    planted = []
    for i in range(len(path)):
        last = i + klen - 1                                       # the call's k-mer i ends with called letter `last`
        planted.append(wof[last - qs] - klen + 2 if qs <= last < qe else None)
    return dict(path=path, move_row=move_row, nrow=nrow, qlen=len(letters), ldq=len(letters) + 3, row=row,
                codes=np.array(codes, dtype=np.uint8), minus=minus, wstart=wstart, coff=coff, rlen=rlen, G=wstart + rlen + 9, klen=klen,
                planted=planted, window=win, letters=letters)


def run_planted(case, **over):
    a = dict(case)
    a.update(over)
    codes = a['codes']
    return read_window(a['path'], a['move_row'], a['nrow'], a['qlen'], a['ldq'], a['row'], codes, a.get('ops_len', len(codes)),
                       a['minus'], a['wstart'], a['coff'], a['rlen'], a['G'], a['klen'], a.get('center_cap', a['nrow'] + 1))


# ---- a planted genome ------------------------------------------------------------------------------------------------------------------

#: the windows of the truth the 12 planted reads spell (start, end), odd reads as the reverse complement
SAMPLE_WINDOWS = ((0, 300), (40, 360), (80, 420), (120, 480), (160, 540), (200, 600), (0, 260), (50, 350), (100, 450), (150, 550),
                  (200, 590), (210, 590))
SAMPLE_SUB, SAMPLE_RUN, SAMPLE_INS = 150, (300, 305), 450


#: shorter windows, fewer than 255 k-mers each: a band of 256 states is then all 0 and the banded bits are the dense ones
SHORT_WINDOWS = ((0, 200), (100, 340), (150, 400), (280, 520), (350, 600), (390, 600), (60, 310), (230, 480))


def planted_genome(seed=3, k=3, nletters=600, windows=SAMPLE_WINDOWS):
    """rescore_ref.planted_case's recipe on genome coordinates: a truth of `nletters` random letters with a homopolymer of 5 at
    SAMPLE_RUN; 12 float32 posteriors that each spell their own window of it (SAMPLE_WINDOWS, the odd ones as the reverse complement)
    over twice as many rows as the window has k-mers; read 12 spells an unrelated string (it maps nowhere) and read 13 the window of
    read 0 again (for keep=).  The draft differs from the truth by a substitution at SAMPLE_SUB, one letter of the run deleted and a
    letter inserted in front of SAMPLE_INS.  -> dict(truth, draft, post [T, 14, 4^k + 1], steps int32 [14], texts: the reads' strings)"""
    rng = np.random.default_rng(seed)
    letters = [('ACGT')[i] for i in rng.integers(0, 4, size=nletters)]
    a, b = SAMPLE_RUN
    letters[a - 1], letters[b] = 'C', 'G'
    letters[a:b] = 'A' * (b - a)
    truth = ''.join(letters)
    other = lambda c: 'ACGT'[('ACGT'.index(c) + 1 + int(rng.integers(0, 3))) % 4]                 # noqa: E731
    ins = next(c for c in 'ACGT' if c not in (truth[SAMPLE_INS - 1], truth[SAMPLE_INS]))          # (the insertion lengthens no run)
    draft = truth[:SAMPLE_SUB] + other(truth[SAMPLE_SUB]) + truth[SAMPLE_SUB + 1:a] + truth[a + 1:SAMPLE_INS] + ins + truth[SAMPLE_INS:]
    texts = [truth[s:e] if i % 2 == 0 else revcomp(truth[s:e]) for i, (s, e) in enumerate(windows)]
    texts.append(''.join('ACGT'[i] for i in rng.integers(0, 4, size=260)))
    texts.append(texts[0])
    S = 4 ** k + 1
    steps = np.array([2 * (len(t) - k + 1) for t in texts], dtype=np.int32)
    post = rng.uniform(size=(int(steps.max()), len(texts), S)).astype(np.float32) * np.float32(0.2)
    post[:, :, 0] += 1.0
    for r, t in enumerate(texts):
        states = np.array([sum('ACGT'.index(c) * 4 ** (k - 1 - i) for i, c in enumerate(t[p:p + k])) for p in range(len(t) - k + 1)])
        rows = np.sort(rng.choice(int(steps[r]), size=len(states), replace=False))
        post[rows, r, 0] -= 1.0
        post[rows, r, states + 1] += 1.0
    post /= post.sum(axis=2, keepdims=True)
    return dict(truth=truth, draft=draft, post=post, steps=steps, texts=texts, k=k)
