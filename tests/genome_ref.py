"""A dict / numpy model of the seed-and-vote stage of csrc/genome_map.hip and of the window and reference-cutting arithmetic of
sloika_amd/genome.py (design/genome_map.md).  Not a test: tests/test_genome_host.py checks it against hand-worked cases, and
tests/test_gpu_genome.py holds the kernels to it, integer for integer.

Letters A C G T are 0..3, any other letter breaks the k-mers that hold it; a k-mer's code is the base-4 number of its letters,
first letter most significant.  A genome is a list of (name, str); positions count through the contigs laid end to end.
"""
import math
from collections import defaultdict

import numpy as np

DIGIT = {'A': 0, 'C': 1, 'G': 2, 'T': 3}
INVALID = 0x7FFFFFFF
OFFSET = 65536
COMPLEMENT = {'A': 'T', 'C': 'G', 'G': 'C', 'T': 'A'}


def revcomp(s):
    return ''.join(COMPLEMENT.get(ch, ch) for ch in reversed(s))


def kmer_code(word):
    """Code of a word, or None when a letter of it is not one of A C G T."""
    code = 0
    for ch in word:
        if ch not in DIGIT:
            return None
        code = code * 4 + DIGIT[ch]
    return code


def packed(contigs):
    """-> (all letters as one str, [start of contig 0, ..., start of the last, total length])."""
    text = ''.join(seq.upper() for _, seq in contigs)
    starts = [0]
    for _, seq in contigs:
        starts.append(starts[-1] + len(seq))
    return text, starts


def genome_keys(contigs, k):
    """-> (int64 array with code << 32 | p for every position p, number of valid k-mers).  A k-mer that holds another letter or
    does not end inside its own contig has the code INVALID."""
    keys = []
    base = 0
    valid = 0
    for _, seq in contigs:
        seq = seq.upper()
        for j in range(len(seq)):
            code = kmer_code(seq[j:j + k]) if j + k <= len(seq) else None
            valid += code is not None
            keys.append(((INVALID if code is None else code) << 32) | (base + j))
        base += len(seq)
    return np.array(keys, dtype=np.int64), valid


def occurrences(contigs, k):
    """dict: code -> ascending list of the packed positions at which it occurs."""
    table = defaultdict(list)
    keys, _ = genome_keys(contigs, k)
    for key in keys.tolist():
        if key >> 32 != INVALID:
            table[key >> 32].append(key & 0xFFFFFFFF)
    return table


def vote(table, seq, k, width, max_occ):
    """One sequence, as it stands, against the table -> (bin, votes, second, nseed).

    Every position i with a valid k-mer that occurs at most max_occ times is a seed; each of its occurrences p casts the diagonal
    p - i + OFFSET into the bins d // width and d // width - 1.  bin: the greatest count, the smallest such bin on a tie (0 when
    nothing was counted); second: the greatest count among bins more than 2 away from it."""
    seq = seq.upper()
    count = defaultdict(int)
    nseed = 0
    for i in range(len(seq) - k + 1):
        code = kmer_code(seq[i:i + k])
        if code is None:
            continue
        places = table.get(code, ())
        if len(places) > max_occ:
            continue
        nseed += 1
        for p in places:
            d = p - i + OFFSET
            count[d // width] += 1
            count[d // width - 1] += 1
    if not count:
        return (0, 0, 0, nseed)
    votes = max(count.values())
    bin_ = min(b for b, c in count.items() if c == votes)
    second = max([c for b, c in count.items() if abs(b - bin_) > 2] + [0])
    return (bin_, votes, second, nseed)


def seed(table, query, k, width, max_occ):
    """Both strands of one query: [[bin, votes, second, nseed] of the query, the same of its reverse complement]."""
    return [list(vote(table, query, k, width, max_occ)), list(vote(table, revcomp(query.upper()), k, width, max_occ))]


def choose_strand(rows, min_votes):
    """rows as `seed` returns them -> ('+' or '-', the chosen row) or None when unmapped.  More votes wins, a tie goes to '+'."""
    which = 1 if rows[1][1] > rows[0][1] else 0
    if rows[which][1] < min_votes or rows[which][1] < 1:
        return None
    return '+-'[which], rows[which]


def window(bin_, n, width, drift, starts):
    """The window (packed coordinates) and contig of a query of n letters whose winning bin is bin_: the bin's diagonals
    [bin_ * width, (bin_ + 2) * width) less OFFSET, the query's n letters behind the last of them, and width + ceil(drift * n)
    letters of slack either side; clipped to the contig in which the midpoint (clamped to the genome) lies."""
    slack = width + int(math.ceil(drift * n))
    lo = bin_ * width - OFFSET - slack
    hi = (bin_ + 2) * width - OFFSET + n + slack
    mid = min(max((lo + hi) // 2, 0), starts[-1] - 1)
    c = max(j for j in range(len(starts) - 1) if starts[j] <= mid)
    return max(lo, starts[c]), min(hi, starts[c + 1]), c


def reference_span(q_start, q_end, r_start, r_end, strand, n, contig_len, pad):
    """get_refs: the part of the contig a read's reference is cut from.  A SAM record of a '-' alignment stores the reverse
    complement of the read, so the unaligned letters in front of the alignment ON THE RECORD are the read's last ones."""
    if strand == '+':
        lead, tail = q_start, n - q_end
    else:
        lead, tail = n - q_end, q_start
    return max(0, r_start - lead - pad), min(contig_len, r_end + tail + pad)


def read_reference(contig_seq, q_start, q_end, r_start, r_end, strand, n, pad):
    lo, hi = reference_span(q_start, q_end, r_start, r_end, strand, n, len(contig_seq), pad)
    piece = contig_seq[lo:hi].upper()
    return piece if strand == '+' else revcomp(piece)
