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


def _align_device(q, ldq, qlen, max_qlen, ref, roff, rlens, scores, both_strands, ops=False, workspace_limit=None, parts_out=None):
    """q:[B][ldq] uint8, qlen:[B] int32, ref packed uint8, roff:[B+1] int64 -- all on the device; rlens host int64.
    -> (int32 [B, 9] host array, strand array of '+' / '-'), and with `ops` the alignments' columns as an Ops (the traceback runs
    right behind the forward launch, on the device rows as they are: in the coordinates of the buffer they were computed against).
    parts_out: a list that receives (reference buffer, roff, device rows, host mask of the pairs it serves) per strand buffer, for a
    caller that runs the traceback itself over several such calls (genome.Index._map_device)."""
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
        return res, out

    fwd, fwd_d = run(ref)
    strand = np.full(B, '+', dtype='U1')
    parts = [(ref, roff, fwd_d, np.ones(B, dtype=bool))]
    buffer_rows = fwd.copy() if (ops or parts_out is not None) else None
    if both_strands and B:
        rc = revcomp_packed(ref, roff, max_rlen)
        rev, rev_d = run(rc)
        take = rev[:, 0] > fwd[:, 0]                       # a tie goes to '+'
        if buffer_rows is not None:                        # which buffer serves which pair: settled BEFORE '-' rows change coordinates
            buffer_rows[take] = rev[take]
            parts = [(ref, roff, fwd_d, ~take), (rc, roff, rev_d, take.copy())]
        rs, re = rev[:, 3].copy(), rev[:, 4].copy()        # back to forward-strand coordinates, as a SAM record gives them
        rev[:, 3] = np.where(rev[:, 0] > 0, rlens - re, 0)
        rev[:, 4] = np.where(rev[:, 0] > 0, rlens - rs, 0)
        fwd[take] = rev[take]
        strand[take] = '-'
    if parts_out is not None:
        parts_out.extend(parts)
    if not ops:
        return fwd, strand
    return fwd, strand, _traceback_device(q, ldq, qlen, parts, buffer_rows, scores, workspace_limit)


# ---- the alignments' columns: traceback, CIGAR, error profile, SAM (csrc/align_traceback.hip, design/align_traceback.md) ------------

#: codes of an alignment column (include/sloika_amd.h: SLK_ALIGN_OP_*)
OP_MATCH, OP_MISMATCH, OP_INSERTION, OP_DELETION = 0, 1, 2, 3
#: letter classes of the error profile; 'gap' is the side an insertion / a deletion has no letter on
LETTER_CLASSES = ("A", "C", "G", "T", "other", "gap")
#: names of the 68 entries of a profile row: "query class/reference class", then the run-length histograms
PROFILE_FIELDS = tuple(["%s/%s" % (a, b) for a in LETTER_CLASSES for b in LETTER_CLASSES] +
                       ["%s_run_%s" % (w, "%d" % k if k < 16 else "16+") for w in ("insertion", "deletion") for k in range(1, 17)])
#: per-pair status of the traceback (include/sloika_amd.h: SLK_ALIGN_TB_*)
TB_DONE, TB_EMPTY = 0, 1
TB_REASONS = {
    -1: "a span of its row lies outside the sequences",
    -2: "its row has a negative count",
    -3: "the spans of its row are not the sums of its counts",
    -4: "insertions + deletions + 1 exceed the widest band the traceback kernel accepts",
    -5: "its slice of the traceback workspace is misaligned, too short or outside the workspace",
    -6: "its slice of the column codes does not have the length of its alignment",
    -7: "the band's DP does not end on the row's score (the row does not belong to these sequences and scores)",
    -8: "the walk did not reach the alignment's start in the announced number of columns",
}


def _traceback_runs(nbytes, limit):
    """Consecutive runs [lo, hi) whose traceback workspace stays within `limit` bytes; a pair above the limit alone is a run of one."""
    n = len(nbytes)
    if limit is None or n == 0:
        return [(0, n)]
    runs, lo, tot = [], 0, 0
    for b in range(n):
        if b > lo and tot + int(nbytes[b]) > limit:
            runs.append((lo, b))
            lo, tot = b, 0
        tot += int(nbytes[b])
    runs.append((lo, n))
    return runs


def _traceback_device(q, ldq, qlen, parts, rows, scores, workspace_limit=None):
    """The columns of the alignments `rows` describes -> Ops.  parts: [(reference buffer, roff, device rows, host mask)], one per
    strand buffer; a buffer's launch sees a zeroed row for every pair it does not serve.  rows: host [B, 9], every pair's row in the
    coordinates of ITS buffer.  Offsets come from the host rows; the launches are split at workspace_limit bytes of workspace, and a
    pair's columns do not depend on the split."""
    import torch
    from . import device as D
    L = _lib.lib()
    B = len(rows)
    dev = qlen.device
    rows = np.ascontiguousarray(rows, dtype=np.int32)
    live = rows[:, 0] > 0
    ncol = np.where(live, rows[:, 5:9].astype(np.int64).sum(axis=1), 0)
    off = np.concatenate(([0], np.cumsum(ncol))).astype(np.int64)
    need = np.array([L.slk_align_traceback_workspace_bytes(int(r[2] - r[1]), int(r[4] - r[3]), int(r[7]), int(r[8])) if r[0] > 0 else 0
                     for r in rows], dtype=np.int64)
    codes = torch.empty(max(int(off[-1]), 8), dtype=torch.uint8, device=dev)
    off_d = torch.from_numpy(off).to(dev)
    status = np.full(B, TB_EMPTY, dtype=np.int32)
    kept = []
    for ref, roff, rows_d, mask in parts:
        if not B:
            break
        mask = np.asarray(mask, dtype=bool)
        rows_m = rows_d if mask.all() else rows_d * torch.from_numpy(mask.astype(np.int32)).to(dev)[:, None]
        rows_m = rows_m.contiguous()
        st_d = torch.empty(B, dtype=torch.int32, device=dev)
        want = np.where(mask, need, 0)
        for lo, hi in _traceback_runs(want, workspace_limit):
            wo = np.concatenate(([0], np.cumsum(want[lo:hi]))).astype(np.int64)
            ws = torch.empty(max(int(wo[-1]), 16), dtype=torch.uint8, device=dev)
            wo_d = torch.from_numpy(wo).to(dev)
            _lib.check(L.slk_align_traceback_batch_u8(q[lo:hi].data_ptr(), ldq, qlen[lo:hi].data_ptr(), ref.data_ptr(),
                                                      roff[lo:hi + 1].data_ptr(), hi - lo, scores[0], scores[1], scores[2], scores[3],
                                                      rows_m[lo:hi].data_ptr(), codes.data_ptr(), off_d[lo:hi + 1].data_ptr(),
                                                      codes.numel(), ws.data_ptr(), wo_d.data_ptr(), ws.numel(),
                                                      st_d[lo:hi].data_ptr(), D.stream_ptr()), "align_traceback_batch")
        status[mask] = st_d.cpu().numpy()[mask]
        kept.append((ref, roff, rows_m, st_d))
    return Ops(q, ldq, qlen, kept, rows, codes, off, off_d, status, int(need.sum()))


class Ops(object):
    """The columns of a batch of alignments, on the device.

    codes_dev: uint8 device tensor, one byte per alignment column (OP_MATCH, OP_MISMATCH, OP_INSERTION: a query letter against a
    gap, OP_DELETION: a reference letter against a gap), pair b's at offsets[b] .. offsets[b + 1] in query order (offsets: host
    int64, offsets_dev: the same on the device).  status: host int32 per pair, TB_DONE, TB_EMPTY (no alignment, no columns) or a
    negative code of TB_REASONS; touching such a pair raises a ValueError that names it.  rows: host [B, 9], every pair's row in
    the coordinates of the buffer its columns index.  q, ldq, qlen: the query buffer; parts: per strand buffer (reference buffer --
    for '-' the reverse-complemented one --, roff, the device rows that buffer's launch saw, its device status).
    workspace_bytes: what the tracebacks needed in all.  qual: None, or a uint8 device tensor [B, ldq] with a quality byte beside
    every letter of q (genome.Index.map(quals=) / map_paths(conf=) set it; a weighted genome.Pileup reads it)."""

    def __init__(self, q, ldq, qlen, parts, rows, codes, offsets, offsets_dev, status, workspace_bytes=0):
        self.q, self.ldq, self.qlen, self.parts, self.rows = q, ldq, qlen, parts, rows
        self.codes_dev, self.offsets, self.offsets_dev, self.status = codes, offsets, offsets_dev, status
        self.workspace_bytes = workspace_bytes
        self.qual = None                                        # [B][ldq] quality bytes beside q, set by genome.Index.map / map_paths
        self._host = None
        self._qlen_host = None

    def __len__(self):
        return len(self.rows)

    def check(self, b):
        if self.status[b] < 0:
            raise ValueError("align: no columns for pair %d: %s" % (b, TB_REASONS.get(int(self.status[b]), "status %d" % self.status[b])))

    def codes(self, b):
        """uint8 host array of pair b's columns in query order (empty for an empty alignment)."""
        self.check(b)
        if self._host is None:
            self._host = self.codes_dev.cpu().numpy()
        if self.status[b] != TB_DONE:
            return np.zeros(0, dtype=np.uint8)
        return self._host[self.offsets[b]:self.offsets[b + 1]]

    def query_lengths(self):
        if self._qlen_host is None:
            self._qlen_host = self.qlen.cpu().numpy()
        return self._qlen_host

    def queries(self):
        """The query letters as a list of bytes, fetched from the device buffer (for a SAM export of calls that never left it)."""
        n = self.query_lengths()
        host = self.q.cpu().numpy() if len(n) else np.zeros((0, 1), dtype=np.uint8)
        return [host[b, :n[b]].tobytes() for b in range(len(n))]

    def cigar(self, b, extended=True, clip=None, reverse=False):
        """Pair b's CIGAR: '=' / 'X' / 'I' / 'D', or 'M' / 'I' / 'D' when not extended ('*' for an empty alignment).  clip: the
        query's length; the unaligned letters in front of and behind the alignment then become soft clips.  reverse: the columns
        back to front, as a SAM record of a '-' alignment gives them."""
        codes = self.codes(b)
        if self.status[b] != TB_DONE:
            return "*"
        front = back = 0
        if clip is not None:
            front, back = int(self.rows[b, 1]), int(clip) - int(self.rows[b, 2])
        if reverse:
            codes, front, back = codes[::-1], back, front
        return cigar_string(codes, extended, front, back)

    def profile(self):
        """int32 host array [B, 68] (PROFILE_FIELDS) from slk_align_error_profile_u8; zeros for a pair without columns."""
        import torch
        from . import device as D
        B = len(self)
        total = np.zeros((B, len(PROFILE_FIELDS)), dtype=np.int32)
        for b in np.flatnonzero(self.status < 0):
            self.check(b)
        for ref, roff, rows_d, st_d in self.parts:
            out = torch.empty((B, len(PROFILE_FIELDS)), dtype=torch.int32, device=self.codes_dev.device)
            _lib.check(_lib.lib().slk_align_error_profile_u8(self.q.data_ptr(), self.ldq, ref.data_ptr(), roff.data_ptr(),
                                                             rows_d.data_ptr(), self.codes_dev.data_ptr(), self.offsets_dev.data_ptr(),
                                                             st_d.data_ptr(), B, out.data_ptr(), D.stream_ptr()), "align_error_profile")
            total += out.cpu().numpy()
        return total


def cigar_string(codes, extended=True, clip_front=0, clip_back=0):
    """Run-length encoding of column codes (host, numpy)."""
    codes = np.asarray(codes, dtype=np.uint8)
    letters = np.frombuffer(b"=XID" if extended else b"MMID", dtype=np.uint8)[codes] if len(codes) else codes
    out = ["%dS" % clip_front] if clip_front > 0 else []
    if len(letters):
        cut = np.flatnonzero(letters[1:] != letters[:-1]) + 1
        starts, ends = np.concatenate(([0], cut)), np.concatenate((cut, [len(letters)]))
        out.extend("%d%s" % (e - s, chr(letters[s])) for s, e in zip(starts, ends))
    if clip_back > 0:
        out.append("%dS" % clip_back)
    return "".join(out)


def error_summary(profile):
    """Figures over all pairs of a profile ([B, 68] or [68]) as a dict: `substitutions` (4 x 4 int array, query letter by reference
    letter over A C G T; the diagonal are the matches), `insertions` / `deletions` by letter (A C G T other), `insertion_runs` /
    `deletion_runs` (16 bins: lengths 1..15 and >= 16), `reference_letters` (aligned reference letters: match + mismatch + deletion)
    and the rates per aligned reference letter: `mismatch_rate` (aligned pairs that are not a match of two of A C G T),
    `insertion_rate`, `deletion_rate`."""
    p = np.asarray(profile, dtype=np.int64).reshape(-1, len(PROFILE_FIELDS)).sum(axis=0)
    m = p[:36].reshape(6, 6)
    pairs, matches = int(m[:5, :5].sum()), int(np.trace(m[:4, :4]))
    ins, dele = int(m[:5, 5].sum()), int(m[5, :5].sum())
    ref = pairs + dele
    rate = (lambda v: float(v) / ref) if ref else (lambda v: float('nan'))
    return {'substitutions': m[:4, :4].copy(), 'insertions': m[:5, 5].copy(), 'deletions': m[5, :5].copy(),
            'insertion_runs': p[36:52].copy(), 'deletion_runs': p[52:68].copy(), 'reference_letters': ref,
            'mismatch_rate': rate(pairs - matches), 'insertion_rate': rate(ins), 'deletion_rate': rate(dele)}


_COMPLEMENT = bytes.maketrans(b"ACGT", b"TGCA")


def sam_record(name, row, strand, codes, query_length, rname, seq=None, qual=None):
    """One SAM line (no newline) of an alignment: row = FIELDS with forward-strand r_start, codes = its columns in query order.
    See sam_records for the field rules.  qual: None ('*'), or the QUAL string of `seq` (Phred + 33, one character per letter, in the
    query's own direction: reversed with SEQ for a '-' alignment)."""
    score, qs, qe, rs = int(row[0]), int(row[1]), int(row[2]), int(row[3])
    if seq is not None and not isinstance(seq, str):
        seq = bytes(bytearray(_as_u8(seq))).decode('ascii')
    if qual is not None:
        if not seq or len(qual) != len(seq):
            raise ValueError("align: QUAL needs a SEQ of the same length")
        qual = str(qual)
    if score <= 0:
        return "\t".join([str(name), "4", "*", "0", "0", "*", "*", "0", "0", seq if seq else "*", qual if qual else "*"])
    front, back = qs, int(query_length) - qe
    if strand == '-':
        codes, front, back = np.asarray(codes)[::-1], back, front
        if seq is not None:
            seq = seq.encode('ascii').translate(_COMPLEMENT)[::-1].decode('ascii')
        if qual is not None:
            qual = qual[::-1]
    nm = int(row[6]) + int(row[7]) + int(row[8])
    return "\t".join([str(name), "16" if strand == '-' else "0", str(rname), str(rs + 1), "255",
                      cigar_string(codes, False, front, back), "*", "0", "0", seq if seq else "*", qual if qual else "*",
                      "NM:i:%d" % nm, "AS:i:%d" % score])


# ---- are the qualities of calls calibrated?  (design/lattice_marginals.md) ----------------------------------------------------------

def calibration_counts(columns, starts, quals, qmax=60):
    """Right and wrong letters per Phred value, from plain arrays: columns[b] the codes of pair b's alignment in query order (OP_*),
    starts[b] the query letter its first column lies at, quals[b] the Phred values of the query's letters.  The j-th column that
    consumes a query letter (match, mismatch, insertion) is letter starts[b] + j: OP_MATCH counts right, OP_MISMATCH and OP_INSERTION
    wrong; deletions have no letter and the clipped letters outside the alignment count nowhere.  -> int64 [qmax + 1][2]."""
    qmax = int(qmax)
    counts = np.zeros((qmax + 1, 2), dtype=np.int64)
    if not len(columns) == len(starts) == len(quals):
        raise ValueError("calibration_counts needs one start and one quality array per alignment")
    for b, (codes, start, q) in enumerate(zip(columns, starts, quals)):
        codes = np.asarray(codes, dtype=np.uint8).reshape(-1)
        q = np.asarray(q).reshape(-1)
        letters = codes[codes != OP_DELETION]
        if letters.size == 0:
            continue
        if (letters > OP_DELETION).any():
            raise ValueError("alignment %d holds a code that is no column" % b)
        start = int(start)
        if start < 0 or start + letters.size > q.size:
            raise ValueError("alignment %d covers letters %d .. %d of a query with %d qualities" % (b, start, start + letters.size, q.size))
        mine = q[start:start + letters.size].astype(np.int64)
        if mine.min() < 0 or mine.max() > qmax:
            raise ValueError("alignment %d: qualities must lie in 0 .. %d" % (b, qmax))
        np.add.at(counts, (mine, (letters != OP_MATCH).astype(np.int64)), 1)
    return counts


def quality_calibration(ops, quals, qmax=60):
    """calibration_counts over the alignments of an Ops (align_batch / accuracy_of_paths with ops=True): quals[b] the Phred values of
    query b's letters (bio.paths_to_bases_qual).  A pair without an alignment counts nowhere.  -> int64 [qmax + 1][2], the right and
    the wrong letters per Phred value."""
    if len(quals) != len(ops):
        raise ValueError("quality_calibration needs one quality array per pair")
    return calibration_counts([ops.codes(b) for b in range(len(ops))], [int(ops.rows[b, 1]) for b in range(len(ops))], quals, qmax)


def calibration_table(counts):
    """The empirical Phred value of every bin of quality_calibration's counts: -10 log10(wrong / (right + wrong)) as float64
    [qmax + 1]; NaN for a bin without letters, inf for one without a wrong letter."""
    counts = np.asarray(counts, dtype=np.float64)
    total = counts.sum(axis=1)
    with np.errstate(divide='ignore', invalid='ignore'):
        return np.where(total > 0, -10.0 * np.log10(counts[:, 1] / total), np.nan)


def sam_records(res, strand, ops, names, ref_names, ref_lengths, queries=None):
    """SAM lines of the alignments of align_batch / accuracy_of_paths (ops=True), one per pair (misc/align.py:46-67 leaves a SAM
    file behind; this is its content for the optimal alignment).  ref_names[b] / ref_lengths[b]: pair b's reference.

    FLAG 0 ('+'), 16 ('-') or 4 (no alignment: RNAME '*', POS 0, MAPQ 0, CIGAR '*'); POS = r_start + 1 on the forward strand; MAPQ
    255, which the SAM specification reserves for "not available" (no mapping quality is computed); CIGAR with M / I / D and soft
    clips for the unaligned ends of the query; tags NM:i = mismatch + insertion + deletion and AS:i = score.  For '-' the columns
    are reversed and SEQ is the reverse complement of the query.  SEQ is '*' without `queries` (ops.queries() fetches calls that
    never left the device); QUAL is '*'.  No secondary or supplementary records."""
    n = ops.query_lengths()
    out = []
    for b in range(len(res)):
        if res[b][0] > 0 and int(res[b][4]) > int(ref_lengths[b]):
            raise ValueError("align: pair %d ends at %d on a reference of %d letters" % (b, res[b][4], ref_lengths[b]))
        out.append(sam_record(names[b], res[b], str(strand[b]), ops.codes(b), n[b], ref_names[b],
                              None if queries is None else queries[b]))
    return out


def sam_text(header_refs, records):
    """A SAM file's text: @HD, one @SQ per (name, length) of header_refs, then the records."""
    head = ["@HD\tVN:1.6\tSO:unknown"] + ["@SQ\tSN:%s\tLN:%d" % (name, int(length)) for name, length in header_refs]
    return "\n".join(head + list(records)) + "\n"


def align_batch(queries, references, match=1, mismatch=2, gap_open=2, gap_extend=1, both_strands=False, ops=False,
                workspace_limit=None):
    """Optimal local alignment of queries[b] against references[b] with affine gaps (a gap of k letters costs
    gap_open + k * gap_extend; the defaults are bwa's -A 1 -B 2 -O 2 -E 1 of align.py:22).

    Sequences are str (upper-cased), bytes or uint8 arrays.  Returns (results, strand): results is an int32 [B, 9] host array
    with the columns FIELDS (0-based half-open coordinates; all 0 for an empty alignment), strand an array of '+' / '-'.
    With both_strands each query is also aligned against the reverse complement of its reference and the higher score kept
    (a tie goes to '+'; this is samacc's `strand` column, align.py:40-41, 120); r_start / r_end of a '-' row are forward-strand
    coordinates, the counts are those of the alignment against the reverse complement.

    ops=True: one more value, the alignments' columns as an Ops (for a '-' pair: columns against the reverse complement of the
    reference, in query order); workspace_limit: bytes of traceback workspace per launch (None: one launch)."""
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
    if B == 0 and not ops:
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
                         (int(match), int(mismatch), int(gap_open), int(gap_extend)), both_strands, ops, workspace_limit)


def accuracy_of_paths(paths, lens, references, kmer_len, alphabet='ACGT', match=1, mismatch=2, gap_open=2, gap_extend=1,
                      both_strands=False, ops=False, workspace_limit=None):
    """Align decoded paths to their references without the called sequences leaving the device.

    paths:[B, T] int32 device tensor of k-mer states and lens:[B] int32 device tensor, as any `call_*` returns them.  The
    paths become bases on the device (slk_paths_to_bases, always_move=True, what bio.paths_to_bases runs) and that buffer is
    the kernel's query operand as it lies.  Returns (results, strand, query_lengths): as align_batch, plus the number of
    bases called per read (the denominator of samacc's coverage).  ops=True: one more value, the alignments' columns as an Ops,
    made from the same device buffer (workspace_limit as for align_batch)."""
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
    got = _align_device(bases, cap, nb, max_qlen, ref, torch.from_numpy(roff).to(paths.device), rlens,
                        (int(match), int(mismatch), int(gap_open), int(gap_extend)), both_strands, ops, workspace_limit)
    return (got[0], got[1], counts) + tuple(got[2:])


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
