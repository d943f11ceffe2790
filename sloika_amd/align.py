"""Read accuracy on the device: align called bases to their references (reference: misc/align.py).

The reference's second workflow step runs `bwa mem -A 1 -B 2 -O 2 -E 1` (align.py:22) through a subprocess and turns every
alignment into a `samacc` row through pysam (align.py:70-133).  Neither tool is part of this project: `align_batch` computes
the OPTIMAL local alignment with affine gaps under the same scores on the GPU (csrc/align.hip, C ABI
slk_align_local_batch_u8; design/align.md).  It is the optimum and not bwa's seed-and-extend heuristic, so figures can differ
slightly from a `bwa mem` run (never towards a lower score).

There is no CPU fallback, like the rest of the package.
"""
import numpy as np

from . import _lib

#: the columns of a result row
FIELDS = ("score", "q_start", "q_end", "r_start", "r_end", "match", "mismatch", "insertion", "deletion")
#: longest sequence the kernel's 16-bit carried fields allow
MAX_LEN = 65535
#: largest score parameter (65535 * 16384 stays inside int32)
MAX_SCORE = 16384
QUANTILES = [5, 25, 50, 75, 95]


def __getattr__(name):
    if name == "PASS_WIDTH":                     # reference columns per pass of the kernel, read from the library
        return int(_lib.lib().slk_align_pass_width())
    raise AttributeError(name)


def _as_u8(seq):
    """str (upper-cased), bytes or uint8 array -> 1-D uint8 array."""
    if isinstance(seq, str):
        seq = seq.upper().encode('ascii')
    if isinstance(seq, (bytes, bytearray)):
        return np.frombuffer(bytes(seq), dtype=np.uint8)
    a = np.asarray(seq)
    if a.dtype != np.uint8 or a.ndim != 1:
        raise ValueError("a sequence is a str, bytes or a 1-D uint8 array")
    return a


def _check_scores(match, mismatch, gap_open, gap_extend):
    for name, v, lo in (("match", match, 1), ("mismatch", mismatch, 0), ("gap_open", gap_open, 0), ("gap_extend", gap_extend, 1)):
        if int(v) != v or v < lo or v > MAX_SCORE:
            raise ValueError("align: %s = %r outside %d..%d" % (name, v, lo, MAX_SCORE))


def _check_len(n, what):
    if n > MAX_LEN:
        raise ValueError("align: %s of %d letters exceeds the limit of %d (16-bit carried fields)" % (what, n, MAX_LEN))


def revcomp_packed(ref, roff, max_len):
    """Reverse complement of sequences packed end to end (device uint8 / int64 offsets) -> new device tensor."""
    import torch
    from . import device as D
    out = torch.empty_like(ref)
    _lib.check(_lib.lib().slk_revcomp_u8(ref.data_ptr(), roff.data_ptr(), roff.numel() - 1, int(max_len), out.data_ptr(),
                                         D.stream_ptr()), "revcomp")
    return out


def _pack_references(references):
    refs = [_as_u8(r) for r in references]
    rlens = np.array([len(r) for r in refs], dtype=np.int64)
    if len(refs):
        _check_len(int(rlens.max()), "a reference")
    roff = np.concatenate(([0], np.cumsum(rlens))).astype(np.int64)
    packed = np.concatenate(refs) if len(refs) and roff[-1] else np.zeros(0, dtype=np.uint8)
    return packed, roff, rlens


def _align_device(q, ldq, qlen, max_qlen, ref, roff, rlens, scores, both_strands):
    """q:[B][ldq] uint8, qlen:[B] int32, ref packed uint8, roff:[B+1] int64 -- all on the device; rlens host int64.
    -> (int32 [B, 9] host array, strand array of '+' / '-')."""
    import torch
    from . import device as D
    L = _lib.lib()
    B = int(qlen.numel())
    max_rlen = int(rlens.max()) if B else 0
    _check_len(max_qlen, "a query")
    _check_len(max_rlen, "a reference")
    nbytes = L.slk_align_local_workspace_bytes(B, max_qlen, max_rlen)
    ws = torch.empty(max(nbytes, 8), dtype=torch.uint8, device=qlen.device)
    if ref.numel() == 0:
        ref = torch.zeros(8, dtype=torch.uint8, device=qlen.device)

    def run(r):
        out = torch.empty((B, 9), dtype=torch.int32, device=qlen.device)
        _lib.check(L.slk_align_local_batch_u8(q.data_ptr(), ldq, qlen.data_ptr(), r.data_ptr(), roff.data_ptr(), B, max_qlen,
                                              max_rlen, scores[0], scores[1], scores[2], scores[3], out.data_ptr(),
                                              ws.data_ptr(), nbytes, D.stream_ptr()), "align_local_batch")
        res = out.cpu().numpy()
        if (res[:, 0] < 0).any():
            raise ValueError("align: a sequence on the device is longer than the bound it was launched with")
        return res

    fwd = run(ref)
    strand = np.full(B, '+', dtype='U1')
    if both_strands and B:
        rev = run(revcomp_packed(ref, roff, max_rlen))
        take = rev[:, 0] > fwd[:, 0]                       # a tie goes to '+'
        rs, re = rev[:, 3].copy(), rev[:, 4].copy()        # back to forward-strand coordinates, as a SAM record gives them
        rev[:, 3] = np.where(rev[:, 0] > 0, rlens - re, 0)
        rev[:, 4] = np.where(rev[:, 0] > 0, rlens - rs, 0)
        fwd[take] = rev[take]
        strand[take] = '-'
    return fwd, strand


def align_batch(queries, references, match=1, mismatch=2, gap_open=2, gap_extend=1, both_strands=False):
    """Optimal local alignment of queries[b] against references[b] with affine gaps (a gap of k letters costs
    gap_open + k * gap_extend; the defaults are bwa's -A 1 -B 2 -O 2 -E 1 of align.py:22).

    Sequences are str (upper-cased), bytes or uint8 arrays.  Returns (results, strand): results is an int32 [B, 9] host array
    with the columns FIELDS (0-based half-open coordinates; all 0 for an empty alignment), strand an array of '+' / '-'.
    With both_strands each query is also aligned against the reverse complement of its reference and the higher score kept
    (a tie goes to '+'; this is samacc's `strand` column, align.py:40-41, 120); r_start / r_end of a '-' row are forward-strand
    coordinates, the counts are those of the alignment against the reverse complement."""
    import torch
    queries, references = list(queries), list(references)
    if len(queries) != len(references):
        raise ValueError("align: %d queries but %d references" % (len(queries), len(references)))
    _check_scores(match, mismatch, gap_open, gap_extend)
    qs = [_as_u8(x) for x in queries]
    B = len(qs)
    max_qlen = max([len(x) for x in qs] + [0])
    _check_len(max_qlen, "a query")
    packed, roff, rlens = _pack_references(references)
    _lib.require_gpu()
    from . import device as D
    if B == 0:
        return np.zeros((0, 9), dtype=np.int32), np.zeros(0, dtype='U1')
    ldq = max(max_qlen, 1)
    qh = np.zeros((B, ldq), dtype=np.uint8)
    for b, x in enumerate(qs):
        qh[b, :len(x)] = x
    dev = D.device()
    q = torch.from_numpy(qh).to(dev)
    qlen = torch.tensor([len(x) for x in qs], dtype=torch.int32).to(dev)
    ref = torch.from_numpy(packed.copy()).to(dev)
    return _align_device(q, ldq, qlen, max_qlen, ref, torch.from_numpy(roff).to(dev), rlens,
                         (int(match), int(mismatch), int(gap_open), int(gap_extend)), both_strands)


def accuracy_of_paths(paths, lens, references, kmer_len, alphabet='ACGT', match=1, mismatch=2, gap_open=2, gap_extend=1,
                      both_strands=False):
    """Align decoded paths to their references without the called sequences leaving the device.

    paths:[B, T] int32 device tensor of k-mer states and lens:[B] int32 device tensor, as any `call_*` returns them.  The
    paths become bases on the device (slk_paths_to_bases, always_move=True, what bio.paths_to_bases runs) and that buffer is
    the kernel's query operand as it lies.  Returns (results, strand, query_lengths): as align_batch, plus the number of
    bases called per read (the denominator of samacc's coverage)."""
    import torch
    from . import device as D
    references = list(references)
    _check_scores(match, mismatch, gap_open, gap_extend)
    _lib.require_gpu()
    B, Tmax = paths.shape
    if B != len(references) or lens.numel() != B:
        raise ValueError("align: %d paths but %d references" % (B, len(references)))
    packed, roff, rlens = _pack_references(references)
    if isinstance(alphabet, str):
        alphabet = alphabet.encode('utf-8')
    cap = max(kmer_len * max(Tmax, 1), kmer_len)
    bases = torch.empty((B, cap), dtype=torch.uint8, device=paths.device)
    nb = torch.empty((B,), dtype=torch.int32, device=paths.device)
    _lib.check(_lib.lib().slk_paths_to_bases(paths.data_ptr(), paths.stride(0), lens.data_ptr(), B, kmer_len, len(alphabet), 1,
                                             int.from_bytes(alphabet.ljust(8, b'\0'), 'little'), bases.data_ptr(), cap,
                                             nb.data_ptr(), D.stream_ptr()), "paths_to_bases")
    counts = nb.cpu().numpy()                              # B integers: the lengths only, for the launch bounds and coverage
    max_qlen = int(counts.max()) if B else 0
    ref = torch.from_numpy(packed.copy()).to(paths.device)
    res, strand = _align_device(bases, cap, nb, max_qlen, ref, torch.from_numpy(roff).to(paths.device), rlens,
                                (int(match), int(mismatch), int(gap_open), int(gap_extend)), both_strands)
    return res, strand, counts


def samacc_rows(results, strand, query_lengths, names=None, min_coverage=0.6):
    """Accuracy rows of alignments: the reference's samacc (align.py:97-131) in this project's terms.

    Here `match` counts the aligned pairs whose letters agree (the reference's column of that name is pysam's M count, which is
    match + mismatch in these terms, and its `mismatch` is the NM tag = mismatch + insertion + deletion).  With correct = match:
        coverage    = (q_end - q_start) / query length
        id          = correct / (match + mismatch)
        accuracy    = correct / (match + mismatch + insertion + deletion)
        information = (match + mismatch) * (2 + entropy),   entropy = (1 - perr) log2(1 - perr) + perr log2(perr / 3) [if NM > 0],
                      perr = min(0.75, NM / (match + mismatch + insertion)),  NM = mismatch + insertion + deletion
    Rows below min_coverage are dropped, and so are empty alignments and reads of no letters (nothing to divide by)."""
    results = np.asarray(results)
    rows = []
    for b in range(len(results)):
        score, qs, qe, rs, re, match, mism, ins, dele = (int(v) for v in results[b])
        n = int(query_lengths[b])
        if score <= 0 or n <= 0 or match + mism == 0:
            continue
        coverage = float(qe - qs) / n
        if coverage < min_coverage:
            continue
        nm = mism + ins + dele
        perr = min(0.75, float(nm) / (match + mism + ins))
        pmatch = 1.0 - perr
        entropy = pmatch * np.log2(pmatch)
        if nm > 0:
            entropy += perr * np.log2(perr / 3.0)
        rows.append({
            'query': names[b] if names is not None else b,
            'strand': str(strand[b]),
            'reference_start': rs,
            'reference_end': re,
            'match': match,
            'mismatch': mism,
            'insertion': ins,
            'deletion': dele,
            'coverage': coverage,
            'id': float(match) / (match + mism),
            'accuracy': float(match) / (match + mism + ins + dele),
            'information': (match + mism) * (2.0 + entropy),
        })
    return rows


def summary(rows):
    """The figures of the reference's summary report (align.py:156-204) as a dict: mapped reads, mean accuracy, the 5/25/50/75/95
    percentiles (np.percentile), proportion and count above 0.9 and CIscore in Mbits.  The KDE mode of the accuracies
    (scipy's gaussian_kde) and the histogram plot are left out: neither scipy nor matplotlib is a dependency here."""
    if len(rows) == 0:
        return {'mapped': 0}
    acc = np.array([r['accuracy'] for r in rows], dtype=np.float64)
    info = np.array([r['information'] for r in rows], dtype=np.float64)
    res = {
        'mapped': len(set(r['query'] for r in rows)),
        'mean': float(acc.mean()),
        'quantiles': dict(zip(QUANTILES, (float(v) for v in np.percentile(acc, QUANTILES)))),
        'proportion_gt_90': float((acc > 0.9).mean()),
        'count_gt_90': int((acc > 0.9).sum()),
        'ciscore_mbits': float(info.sum() / 1e6),
    }
    return res
