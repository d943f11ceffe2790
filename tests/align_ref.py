"""An independent statement of the local alignment csrc/align.hip computes (design/align.md): the three full matrices of
Smith-Waterman-Gotoh and a REAL traceback under the contract's priorities -- no counts are carried forward, so this and the
kernel's carried words check each other.  Plain loops: meant for pairs of a few hundred thousand cells.

    E[i][j] = max(H[i][j-1] - O - E, E[i][j-1] - E)          consumes r[j]: a deletion
    F[i][j] = max(H[i-1][j] - O - E, F[i-1][j] - E)          consumes q[i]: an insertion
    H[i][j] = max(0, H[i-1][j-1] + (q[i] == r[j] ? A : -B), E[i][j], F[i][j])

Ties: opening beats extension in E and F; diagonal, then E, then F in H; best <= 0 -> empty cell; the end is the cell of
greatest H, smallest i, then smallest j.  `score_only` is a vectorised score-only DP for larger pairs.
"""
import numpy as np

NEG = -(1 << 40)


def as_bytes(s):
    if isinstance(s, str):
        return s.upper().encode('ascii')
    return bytes(bytearray(np.asarray(s, dtype=np.uint8))) if not isinstance(s, (bytes, bytearray)) else bytes(s)


def matrices(q, r, A=1, B=2, O=2, X=1):
    """(H, E, F) as lists of lists, (n + 1) x (m + 1), borders H = 0 and E = F = NEG."""
    q, r = as_bytes(q), as_bytes(r)
    n, m = len(q), len(r)
    H = [[0] * (m + 1) for _ in range(n + 1)]
    E = [[NEG] * (m + 1) for _ in range(n + 1)]
    F = [[NEG] * (m + 1) for _ in range(n + 1)]
    oe = O + X
    for i in range(1, n + 1):
        Hi, Hu, Ei, Fi, Fu = H[i], H[i - 1], E[i], F[i], F[i - 1]
        qc = q[i - 1]
        for j in range(1, m + 1):
            e = max(Hi[j - 1] - oe, Ei[j - 1] - X)
            f = max(Hu[j] - oe, Fu[j] - X)
            d = Hu[j - 1] + (A if qc == r[j - 1] else -B)
            Ei[j], Fi[j] = e, f
            Hi[j] = max(0, d, e, f)
    return H, E, F


def align(q, r, A=1, B=2, O=2, X=1):
    """The nine integers of the contract: score, q_start, q_end, r_start, r_end, match, mismatch, insertion, deletion."""
    q, r = as_bytes(q), as_bytes(r)
    n, m = len(q), len(r)
    H, E, F = matrices(q, r, A, B, O, X)
    best, bi, bj = 0, 0, 0
    for i in range(1, n + 1):                      # row-major scan with a strict test: smallest i, then smallest j
        Hi = H[i]
        for j in range(1, m + 1):
            if Hi[j] > best:
                best, bi, bj = Hi[j], i, j
    if best == 0:
        return [0] * 9
    oe = O + X
    i, j, state = bi, bj, 'H'
    match = mismatch = ins = dele = 0
    while True:
        if state == 'H':
            if H[i][j] == 0:                       # empty cell: the alignment starts behind it
                break
            d = H[i - 1][j - 1] + (A if q[i - 1] == r[j - 1] else -B)
            if H[i][j] == d:                       # diagonal first
                if q[i - 1] == r[j - 1]:
                    match += 1
                else:
                    mismatch += 1
                i, j = i - 1, j - 1
            elif H[i][j] == E[i][j]:               # then the deletion
                state = 'E'
            else:
                assert H[i][j] == F[i][j]
                state = 'F'
        elif state == 'E':
            dele += 1
            if E[i][j] == H[i][j - 1] - oe:        # the opening beats the extension
                state = 'H'
            else:
                assert E[i][j] == E[i][j - 1] - X
            j -= 1
        else:
            ins += 1
            if F[i][j] == H[i - 1][j] - oe:
                state = 'H'
            else:
                assert F[i][j] == F[i - 1][j] - X
            i -= 1
    return [best, i, bi, j, bj, match, mismatch, ins, dele]


def score_only(q, r, A=1, B=2, O=2, X=1):
    """Best local score by a DP vectorised along the reference: the in-row dependency of E is a running maximum,
    E[j] = max_k<j (H[k] - O - (j - k) X), where H may be taken without its own E term (a gap opened from a cell that a
    longer gap reaches is never better than extending that gap, as O >= 0)."""
    q = np.frombuffer(as_bytes(q), dtype=np.uint8)
    r = np.frombuffer(as_bytes(r), dtype=np.uint8)
    m = len(r)
    if len(q) == 0 or m == 0:
        return 0
    Hp = np.zeros(m + 1, dtype=np.int64)
    Fp = np.full(m + 1, NEG, dtype=np.int64)
    ramp = np.arange(m + 1, dtype=np.int64) * X
    best = 0
    for c in q:
        F = np.maximum(Hp - (O + X), Fp - X)
        d = np.empty(m + 1, dtype=np.int64)
        d[0] = 0
        d[1:] = Hp[:-1] + np.where(r == c, A, -B)
        G = np.maximum(np.maximum(d, F), 0)                # H without the E term
        G[0] = 0
        run = np.maximum.accumulate(G + ramp)              # max_k<=j (G[k] + k X)
        E = np.full(m + 1, NEG, dtype=np.int64)
        E[1:] = run[:-1] - ramp[1:] - O                    # max_k<j (G[k] - O - (j - k) X)
        H = np.maximum(G, E)
        H[0] = 0
        best = max(best, int(H.max()))
        Hp, Fp = H, F
    return best
