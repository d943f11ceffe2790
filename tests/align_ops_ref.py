"""The columns of the alignment tests/align_ref.py defines: its three full matrices and its traceback, recording the operation
of every column instead of counting them.  Plus numpy models, written from the contract's text, of the 68-entry error profile,
of the CIGAR run-length encoding and of a SAM record, and a small SAM parser that walks a CIGAR over SEQ and the reference.

Column codes: 0 match, 1 mismatch, 2 insertion (a query letter against a gap), 3 deletion (a reference letter against a gap).
"""
import numpy as np

from tests.align_ref import align, as_bytes, matrices  # noqa: F401  (align: the nine integers these columns must count to)

MATCH, MISMATCH, INSERTION, DELETION = 0, 1, 2, 3


def ops(q, r, A=1, B=2, O=2, X=1):
    """-> (row of nine integers, uint8 array of the columns in query order)."""
    q, r = as_bytes(q), as_bytes(r)
    n, m = len(q), len(r)
    H, E, F = matrices(q, r, A, B, O, X)
    best, bi, bj = 0, 0, 0
    for i in range(1, n + 1):
        Hi = H[i]
        for j in range(1, m + 1):
            if Hi[j] > best:
                best, bi, bj = Hi[j], i, j
    if best == 0:
        return [0] * 9, np.zeros(0, dtype=np.uint8)
    oe = O + X
    i, j, state = bi, bj, 'H'
    out = []
    while True:
        if state == 'H':
            if H[i][j] == 0:
                break
            d = H[i - 1][j - 1] + (A if q[i - 1] == r[j - 1] else -B)
            if H[i][j] == d:
                out.append(MATCH if q[i - 1] == r[j - 1] else MISMATCH)
                i, j = i - 1, j - 1
            elif H[i][j] == E[i][j]:
                state = 'E'
            else:
                assert H[i][j] == F[i][j]
                state = 'F'
        elif state == 'E':
            out.append(DELETION)
            if E[i][j] == H[i][j - 1] - oe:
                state = 'H'
            else:
                assert E[i][j] == E[i][j - 1] - X
            j -= 1
        else:
            out.append(INSERTION)
            if F[i][j] == H[i - 1][j] - oe:
                state = 'H'
            else:
                assert F[i][j] == F[i - 1][j] - X
            i -= 1
    codes = np.array(out[::-1], dtype=np.uint8)
    cnt = [int((codes == k).sum()) for k in range(4)]
    return [best, i, bi, j, bj] + cnt, codes


def banded_ops(q, r, row, A=1, B=2, O=2, X=1):
    """What the device traceback computes, in plain loops: the recurrence over the band -D <= i - j <= I of the rectangle the row
    names, anchored at its start cell (H(0,0) = 0, every other border and everything outside the band -inf, no clamp at 0), then a
    walk back from (n', m') in state H.  -> (value of the end cell, columns in query order)."""
    q, r = as_bytes(q)[row[1]:row[2]], as_bytes(r)[row[3]:row[4]]
    n, m, I, D = len(q), len(r), row[7], row[8]
    NEG = -(1 << 40)
    oe = O + X
    H, E, F = {(0, 0): 0}, {}, {}
    for i in range(1, n + 1):
        for j in range(max(1, i - I), min(m, i + D) + 1):
            e = max(H.get((i, j - 1), NEG) - oe, E.get((i, j - 1), NEG) - X)
            f = max(H.get((i - 1, j), NEG) - oe, F.get((i - 1, j), NEG) - X)
            d = H.get((i - 1, j - 1), NEG) + (A if q[i - 1] == r[j - 1] else -B)
            E[i, j], F[i, j], H[i, j] = max(e, NEG), max(f, NEG), max(d, e, f, NEG)
    i, j, state, out = n, m, 'H', []
    while (i, j) != (0, 0) or state != 'H':
        if state == 'H':
            d = H.get((i - 1, j - 1), NEG) + (A if q[i - 1] == r[j - 1] else -B)
            if H[i, j] == d:
                out.append(MATCH if q[i - 1] == r[j - 1] else MISMATCH)
                i, j = i - 1, j - 1
            elif H[i, j] == E[i, j]:
                state = 'E'
            else:
                state = 'F'
        elif state == 'E':
            out.append(DELETION)
            if E[i, j] == H.get((i, j - 1), NEG) - oe:
                state = 'H'
            j -= 1
        else:
            out.append(INSERTION)
            if F[i, j] == H.get((i - 1, j), NEG) - oe:
                state = 'H'
            i -= 1
    return H[n, m], np.array(out[::-1], dtype=np.uint8)


def diagonal_range(codes):
    """(lowest, highest) value of i - j along the path, relative to its start."""
    d = np.concatenate(([0], np.cumsum(np.where(codes == INSERTION, 1, np.where(codes == DELETION, -1, 0)))))
    return int(d.min()), int(d.max())


def letter_class(c):
    return {65: 0, 67: 1, 71: 2, 84: 3}.get(int(c), 4)


def profile(q, r, row, codes):
    """The 68 entries of one pair: [0, 36) columns by query class * 6 + reference class (classes A C G T other gap), [36, 52)
    maximal insertion runs of length 1..15 and >= 16, [52, 68) the same for deletions."""
    q, r = as_bytes(q), as_bytes(r)
    out = np.zeros(68, dtype=np.int32)
    i, j = row[1], row[3]
    for c in codes:
        qc = rc = 5
        if c != DELETION:
            qc = letter_class(q[i])
            i += 1
        if c != INSERTION:
            rc = letter_class(r[j])
            j += 1
        out[qc * 6 + rc] += 1
    assert (i, j) == (row[2], row[4])
    k = 0
    while k < len(codes):
        e = k
        while e < len(codes) and codes[e] == codes[k]:
            e += 1
        if codes[k] == INSERTION:
            out[36 + min(e - k, 16) - 1] += 1
        elif codes[k] == DELETION:
            out[52 + min(e - k, 16) - 1] += 1
        k = e
    return out


def cigar(codes, extended=True, front=0, back=0):
    """Run-length encoding with '=' 'X' 'I' 'D' (or 'M' 'I' 'D'), soft clips of `front` / `back` letters around it."""
    letters = [("=XID" if extended else "MMID")[int(c)] for c in codes]
    out = ["%dS" % front] if front else []
    k = 0
    while k < len(letters):
        e = k
        while e < len(letters) and letters[e] == letters[k]:
            e += 1
        out.append("%d%s" % (e - k, letters[k]))
        k = e
    if back:
        out.append("%dS" % back)
    return "".join(out)


def revcomp(s):
    return s[::-1].translate(str.maketrans('ACGT', 'TGCA'))


def sam_fields(name, row, strand, codes, query, rname):
    """The fields of the SAM record of an alignment whose row has FORWARD-strand r_start (codes in query order)."""
    if row[0] <= 0:
        return [name, "4", "*", "0", "0", "*", "*", "0", "0", query or "*", "*"]
    front, back = row[1], len(query) - row[2]
    if strand == '-':
        codes, front, back, query = codes[::-1], back, front, revcomp(query)
    return [name, "16" if strand == '-' else "0", rname, str(row[3] + 1), "255", cigar(codes, False, front, back), "*", "0", "0",
            query, "*", "NM:i:%d" % (row[6] + row[7] + row[8]), "AS:i:%d" % row[0]]


def parse_sam_line(line, reference):
    """Walk the record's CIGAR over its SEQ and the forward-strand `reference` -> dict with flag, pos, the clips, the numbers of
    M / I / D letters, `nm` counted from the letters (mismatches under M + I + D), the reference span and the tags."""
    import re
    f = line.split("\t")
    flag, pos, seq = int(f[1]), int(f[3]), f[9]
    tags = dict((t[:2], int(t[5:])) for t in f[11:])
    parts = [(int(n), c) for n, c in re.findall(r"(\d+)([MIDS])", f[5])]
    assert "".join("%d%s" % p for p in parts) == f[5]
    qi, rj, cnt, mism = 0, pos - 1, {"M": 0, "I": 0, "D": 0, "S": 0}, 0
    for n, c in parts:
        cnt[c] += n
        if c == "M":
            mism += sum(1 for k in range(n) if seq[qi + k] != reference[rj + k])
        if c in "MIS":
            qi += n
        if c in "MD":
            rj += n
    assert qi == len(seq)
    return {"flag": flag, "pos": pos, "front": parts[0][0] if parts[0][1] == "S" else 0,
            "back": parts[-1][0] if parts[-1][1] == "S" else 0, "M": cnt["M"], "I": cnt["I"], "D": cnt["D"], "mismatch": mism,
            "nm": mism + cnt["I"] + cnt["D"], "r_start": pos - 1, "r_end": rj, "tags": tags}
