"""Plain-loop model of design/pileup.md section 9: the weight of a letter and of a column, the Phred-weighted tables beside the plain
ones, the weighted call with a quality per emitted letter, and the variants with a quality.  Written from that text, not from
csrc/pileup.hip; built on tests/pileup_ref.py's forward view and left-normalisation.  Lists and loops only.

A pair here is pileup_ref's with one more value: (q, r, row, codes, minus, t0, qual), qual one byte per letter of q AS STORED."""
from tests import pileup_ref as R

MATCH, MISMATCH, INSERTION, DELETION = R.MATCH, R.MISMATCH, R.INSERTION, R.DELETION
INS_READS, SPAN = R.INS_READS, R.SPAN
LOW, CHANGED, INSERTED = R.LOW, R.CHANGED, R.INSERTED
LETTERS = R.LETTERS


def weights_table(min_qual=0, qmax=60):
    """The 256 weights: 0 below min_qual, else min(v, qmax)."""
    return [0 if v < min_qual else min(v, qmax) for v in range(256)]


def forward_weights(qual, row, minus, weights):
    """W(i) of the aligned query span: the weight of forward letter Q(i), read where Q(i) is read ('-': back to front)."""
    qs, qe = int(row[1]), int(row[2])
    if not minus:
        return [int(weights[int(qual[qs + i])]) for i in range(qe - qs)]
    return [int(weights[int(qual[qe - 1 - i])]) for i in range(qe - qs)]


def deletion_weight(W, i):
    """The smaller of W(i - 1) and W(i), of those of the two indices that lie in [0, n); 0 if neither does."""
    near = [W[k] for k in (i - 1, i) if 0 <= k < len(W)]
    return min(near) if near else 0


def count(counts, ins, wcounts, wins, codes, Q, W, t0, lo, hi):
    """One pair's forward-view columns into the four tables: wherever 1.3 adds 1, the weighted table adds the weight."""
    S = len(ins[0]) if len(ins) else 1
    m = sum(1 for c in codes if c != INSERTION)
    i = j = 0
    k = 0
    for c in codes:
        if c == INSERTION:
            p = t0 + j - 1
            if j > 0 and lo <= p < hi:
                if k == 0:
                    counts[p - lo][INS_READS] += 1
                    wcounts[p - lo][INS_READS] += W[i]
                if k < S:
                    ins[p - lo][k][Q[i]] += 1
                    wins[p - lo][k][Q[i]] += W[i]
            i += 1
            k += 1
            continue
        k = 0
        p = t0 + j
        if lo <= p < hi:
            entry = 5 if c == DELETION else Q[i]
            w = deletion_weight(W, i) if c == DELETION else W[i]
            counts[p - lo][entry] += 1
            wcounts[p - lo][entry] += w
            if j < m - 1:
                counts[p - lo][SPAN] += 1
                wcounts[p - lo][SPAN] += w
        j += 1
        if c != DELETION:
            i += 1


def pile(pairs, lo, hi, S, weights, normalised=True):
    """pairs: [(q, r, row, codes, minus, t0, qual)] -> (counts, ins, wcounts, wins, [forward codes]) over [lo, hi)."""
    counts, ins = R.tables(hi - lo, S)
    wcounts, wins = R.tables(hi - lo, S)
    views = []
    for q, r, row, codes, minus, t0, qual in pairs:
        f, Q, _ = R.forward_view(q, r, row, codes, minus)
        if normalised:
            f = R.normalise(f, *R.forward_bytes(q, r, row, minus))           # codes move, letters (and their weights) do not
        count(counts, ins, wcounts, wins, f, Q, forward_weights(qual, row, minus, weights), int(t0), lo, hi)
        views.append(f)
    return counts, ins, wcounts, wins, views


def call_full(cn, wcn, wip, ref_byte, min_depth=3, qmax=60):
    """The weighted call of one position -> (bytes emitted, flags, winner: None when LOW, 0..3 a letter, 4 the deletion; letters
    inserted, qualities of the emitted bytes, posq)."""
    depth = sum(int(cn[k]) for k in range(6))
    cand = [int(wcn[0]), int(wcn[1]), int(wcn[2]), int(wcn[3]), int(wcn[5])]
    if depth < min_depth or not any(cand):
        return bytes([ref_byte]), LOW, None, 0, [0], 0
    best = max(cand)
    tied = [k for k in range(5) if cand[k] == best]
    refc = R.letter_class(ref_byte)
    w = refc if refc < 4 and refc in tied else tied[0]
    nxt = max([cand[k] for k in range(5) if k != w] + [int(wcn[4])])
    posq = max(0, min(qmax, best - nxt))
    out, quals, flags, nins = b"", [], 0, 0
    if w < 4:
        out = LETTERS[w:w + 1]
        quals.append(posq)
    if w == 4 or w != refc:
        flags |= CHANGED
    span = int(wcn[SPAN])
    for k in range(len(wip)):
        Wn = sum(int(v) for v in wip[k])
        four = [int(v) for v in wip[k][:4]]
        mx = max(four)
        if not (2 * Wn > span and mx > 0):
            break
        am = four.index(mx)
        out += LETTERS[am:am + 1]
        quals.append(max(0, min(qmax, 2 * mx - span)))
        flags |= INSERTED
        nins += 1
    return out, flags, w, nins, quals, posq


def consensus(counts, wcounts, wins, genome, lo, min_depth=3, qmax=60):
    """-> (consensus bytes, [bytes per position], [flags], [qualities per position], [posq])."""
    genome = R.as_bytes(genome)
    parts, flags, quals, posq = [], [], [], []
    for p in range(len(counts)):
        out, fl, _, _, lq, pq = call_full(counts[p], wcounts[p], wins[p], genome[lo + p], min_depth, qmax)
        parts.append(out)
        flags.append(fl)
        quals.append(lq)
        posq.append(pq)
    return b"".join(parts), parts, flags, quals, posq


def variants(counts, wcounts, wins, genome, lo, contig_offsets, names, min_depth=3, qmax=60):
    """pileup_ref.variants' tuples for the WEIGHTED call with one more value: posq for 'sub' / 'del', the smallest inserted-letter
    quality for 'ins'.  depth and support stay the unweighted counts."""
    genome = R.as_bytes(genome)
    out = []
    for p in range(len(counts)):
        g = lo + p
        c = max(k for k in range(len(names)) if contig_offsets[k] <= g)
        pos, cn = g - int(contig_offsets[c]), counts[p]
        letters, flags, w, nins, quals, posq = call_full(cn, wcounts[p], wins[p], genome[g], min_depth, qmax)
        depth = sum(int(cn[k]) for k in range(6))
        ref = genome[g:g + 1].decode('ascii')
        if flags & CHANGED:
            if w < 4:
                out.append((names[c], pos, 'sub', ref, "ACGT"[w], depth, int(cn[w]), posq))
            else:
                out.append((names[c], pos, 'del', ref, '', depth, int(cn[5]), posq))
        if flags & INSERTED:
            out.append((names[c], pos, 'ins', '', letters[len(letters) - nins:].decode('ascii'), int(cn[SPAN]), int(cn[INS_READS]),
                        min(quals[len(quals) - nins:])))
    return out
