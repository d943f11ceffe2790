"""Plain-loop model of design/pileup.md section 1: the forward view of a pair, the left-normalisation of its gaps, the two tables
and the call per position.  Written from that text, not from csrc/pileup.hip; lists, dicts and loops only.

Codes: 0 match, 1 mismatch, 2 insertion, 3 deletion.  Letter classes A C G T = 0..3, any other byte 4; complement swaps 0 with 3
and 1 with 2 and keeps 4."""
import numpy as np

MATCH, MISMATCH, INSERTION, DELETION = 0, 1, 2, 3
INS_READS, SPAN = 6, 7
LOW, CHANGED, INSERTED = 1, 2, 4
DONE, SKIPPED = 0, 1
BAD_SPAN, BAD_COUNT, BAD_SUM, OPS, POSITION, BAD_CODE, CODE_COUNT = -1, -2, -3, -4, -5, -6, -7
LETTERS = b"ACGT"


def as_bytes(s):
    if isinstance(s, str):
        return s.encode('ascii')
    return bytes(bytearray(np.asarray(s, dtype=np.uint8))) if not isinstance(s, (bytes, bytearray)) else bytes(s)


def letter_class(c):
    return {65: 0, 67: 1, 71: 2, 84: 3}.get(int(c), 4)


def complement_class(k):
    return 3 - k if k < 4 else 4


def revcomp(s):
    return as_bytes(s)[::-1].translate(bytes.maketrans(b"ACGT", b"TGCA"))


def forward_view(q, r, row, codes, minus):
    """1.1 -> (codes in forward order, the query's classes Q(0..), the reference's classes R(0..)) of the aligned spans."""
    q, r = as_bytes(q), as_bytes(r)
    codes = [int(c) for c in codes]
    qs, qe, rs, re = (int(row[k]) for k in (1, 2, 3, 4))
    if not minus:
        return codes, [letter_class(c) for c in q[qs:qe]], [letter_class(c) for c in r[rs:re]]
    return (codes[::-1], [complement_class(letter_class(q[qe - 1 - i])) for i in range(qe - qs)],
            [complement_class(letter_class(r[re - 1 - j])) for j in range(re - rs)])


def forward_bytes(q, r, row, minus):
    """The stored bytes behind Q(i) and R(j): what the letter test of 1.2 compares."""
    q, r = as_bytes(q), as_bytes(r)
    qs, qe, rs, re = (int(row[k]) for k in (1, 2, 3, 4))
    if not minus:
        return list(q[qs:qe]), list(r[rs:re])
    return list(q[qs:qe][::-1]), list(r[rs:re][::-1])


def normalise(codes, Q, R):
    """1.2: one pass, front to back.  Q, R: anything indexable whose equality is the letters' (bytes or classes of A C G T ...;
    callers pass the stored bytes)."""
    c = list(codes)
    pos, i, j = 0, 0, 0
    while pos < len(c):
        K = c[pos]
        if K in (MATCH, MISMATCH):
            pos, i, j = pos + 1, i + 1, j + 1
            continue
        L = 0
        while pos + L < len(c) and c[pos + L] == K:
            L += 1
        a, ii, jj = pos, i, j
        while a > 0 and c[a - 1] in (MATCH, MISMATCH):
            if K == DELETION:
                ok = R[jj - 1] == R[jj + L - 1]
            else:
                ok = Q[ii - 1] == Q[ii + L - 1]
            if not ok:
                break
            c[a + L - 1], c[a - 1] = c[a - 1], K
            a, ii, jj = a - 1, ii - 1, jj - 1
        if K == INSERTION:
            i += L
        else:
            j += L
        pos += L                                                 # behind the run's OLD end
    return c


def count(counts, ins, codes, Q, t0, lo, hi):
    """1.3: add one pair's forward-view columns.  counts: list of P lists of 8, ins: list of P lists of S lists of 5 (or arrays)."""
    S = len(ins[0]) if len(ins) else 1
    m = sum(1 for c in codes if c != INSERTION)
    i = j = 0
    k = 0                                                        # insertion columns directly in front of this one
    for c in codes:
        if c == INSERTION:
            p = t0 + j - 1
            if j > 0 and lo <= p < hi:
                if k == 0:
                    counts[p - lo][INS_READS] += 1
                if k < S:
                    ins[p - lo][k][Q[i]] += 1
            i += 1
            k += 1
            continue
        k = 0
        p = t0 + j
        if lo <= p < hi:
            counts[p - lo][5 if c == DELETION else Q[i]] += 1
            if j < m - 1:
                counts[p - lo][SPAN] += 1
        j += 1
        if c != DELETION:
            i += 1


def call_full(cn, ip, ref_byte, min_depth=3):
    """1.4 for one position -> (bytes emitted, flags, winner: None when LOW, 0..3 a letter, 4 the deletion; letters inserted)."""
    depth = sum(int(cn[k]) for k in range(6))
    cand = [int(cn[0]), int(cn[1]), int(cn[2]), int(cn[3]), int(cn[5])]
    if depth < min_depth or not any(cand):
        return bytes([ref_byte]), LOW, None, 0
    best = max(cand)
    tied = [k for k in range(5) if cand[k] == best]
    refc = letter_class(ref_byte)
    w = refc if refc < 4 and refc in tied else tied[0]           # (candidate 4 is the deletion, not the letter class `other`)
    out, flags, nins = b"", 0, 0
    if w < 4:
        out = LETTERS[w:w + 1]
    if w == 4 or w != refc:
        flags |= CHANGED
    for k in range(len(ip)):
        n_k = sum(int(v) for v in ip[k])
        four = [int(v) for v in ip[k][:4]]
        if not (2 * n_k > int(cn[SPAN]) and max(four) > 0):
            break
        am = four.index(max(four))
        out += LETTERS[am:am + 1]
        flags |= INSERTED
        nins += 1
    return out, flags, w, nins


def call(cn, ip, ref_byte, min_depth=3):
    return call_full(cn, ip, ref_byte, min_depth)[:2]


def tables(P, S):
    return [[0] * 8 for _ in range(P)], [[[0] * 5 for _ in range(S)] for _ in range(P)]


def check_pair(row, codes, qlen, rlen, t0, G):
    """The refusals of slk_pileup_columns_u8, in its order."""
    qs, qe, rs, re = (int(row[k]) for k in (1, 2, 3, 4))
    cnt = [int(row[k]) for k in (5, 6, 7, 8)]
    if not (0 <= qs <= qe <= qlen and 0 <= rs <= re <= rlen):
        return BAD_SPAN
    if min(cnt) < 0:
        return BAD_COUNT
    if cnt[0] + cnt[1] + cnt[2] != qe - qs or cnt[0] + cnt[1] + cnt[3] != re - rs:
        return BAD_SUM
    if len(codes) != sum(cnt):
        return OPS
    if t0 < 0 or t0 + re - rs > G:
        return POSITION
    if any(int(c) > 3 for c in codes):
        return BAD_CODE
    if [sum(1 for c in codes if int(c) == k) for k in range(4)] != cnt:
        return CODE_COUNT
    return DONE


def pile(pairs, lo, hi, S, normalised=True):
    """pairs: [(q, r, row, codes, minus, t0)] -> (counts, ins, [forward codes]) over [lo, hi)."""
    counts, ins = tables(hi - lo, S)
    views = []
    for q, r, row, codes, minus, t0 in pairs:
        f, Q, _ = forward_view(q, r, row, codes, minus)
        if normalised:
            f = normalise(f, *forward_bytes(q, r, row, minus))
        count(counts, ins, f, Q, int(t0), lo, hi)
        views.append(f)
    return counts, ins, views


def consensus(counts, ins, genome, lo, min_depth=3):
    """-> (the consensus of the region as bytes, [bytes per position], [flags per position])."""
    genome = as_bytes(genome)
    parts, flags = [], []
    for p in range(len(counts)):
        out, fl = call(counts[p], ins[p], genome[lo + p], min_depth)
        parts.append(out)
        flags.append(fl)
    return b"".join(parts), parts, flags


def variants(counts, ins, genome, lo, contig_offsets, names, min_depth=3):
    """The list Consensus.variants() gives: (contig, pos within the contig, kind, ref, alt, depth, support), in position order, a
    position's substitution or deletion in front of its insertion.  depth / support: for 'sub' and 'del' the position's depth and
    the winner's count; for 'ins' its span entry and the reads with an insertion behind it."""
    genome = as_bytes(genome)
    out = []
    for p in range(len(counts)):
        g = lo + p
        c = max(k for k in range(len(names)) if contig_offsets[k] <= g)
        pos, cn = g - int(contig_offsets[c]), counts[p]
        letters, flags, w, nins = call_full(cn, ins[p], genome[g], min_depth)
        depth = sum(int(cn[k]) for k in range(6))
        ref = genome[g:g + 1].decode('ascii')
        if flags & CHANGED:
            if w < 4:
                out.append((names[c], pos, 'sub', ref, "ACGT"[w], depth, int(cn[w])))
            else:
                out.append((names[c], pos, 'del', ref, '', depth, int(cn[5])))
        if flags & INSERTED:
            out.append((names[c], pos, 'ins', '', letters[len(letters) - nins:].decode('ascii'), int(cn[SPAN]), int(cn[INS_READS])))
    return out
