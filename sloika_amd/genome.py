"""Locate calls on a genome on the device and cut per-read references (reference: misc/align.py:46-67, the genome that
`bwa mem -k14` is handed, and misc/get_refs_from_sam.py:40-68).

`align.align_batch` needs one reference per read, already cut to the read's locus; a user with a run of reads and a genome FASTA
has neither bwa nor pysam here.  `Index` holds the genome and its sorted k-mer keys on the device; `Index.map` chooses per read and
strand a window of the genome by seed and vote (csrc/genome_map.hip) and aligns the read inside it with csrc/align.hip, unchanged.

What is guaranteed (design/genome_map.md): the result is the OPTIMAL local alignment within the chosen window, and equals the
optimum over the genome whenever that alignment lies inside the window.  It is neither bwa's heuristic nor a proof of global
optimality: `second` (the best vote elsewhere) and `edge` (the alignment ran into a window end) are what to filter on.  Repeats
longer than a read are ambiguous, as for any mapper; supplementary or chimeric placements are not reported.

There is no CPU fallback, like the rest of the package.
"""
import os

import numpy as np

from . import _lib, align, transducer, util

#: added to every diagonal p - i: keeps it positive and makes the bins independent of the batch (csrc/genome_map.hip)
DIAG0 = 65536
MIN_K, MAX_K = 8, 15
MAX_GENOME = 1 << 31
MAX_OCC = 4096
MAX_BIN_WIDTH = 32768
#: the columns of a row of Index.seed's result
SEED_FIELDS = ("bin", "votes", "second", "nseed")


def trim_fast5_extension(fn):
    """get_refs_from_sam.py:34-37."""
    base, ext = os.path.splitext(fn)
    return base if ext == ".fast5" else fn


def fasta(records):
    """The ">name\\nseq\\n" text of a list of (name, sequence) (get_refs_from_sam.py:66)."""
    return ''.join(">{}\n{}\n".format(name, seq if isinstance(seq, str) else bytes(seq).decode('ascii')) for name, seq in records)


def window_of(bin_, n, bin_width, drift):
    """The window of the packed genome that the winning bin of a query of n letters gives, before it is clipped to a contig:
    bin b covers the diagonals [b W, (b + 2) W), a query on diagonal d lies at [d, d + n), and either end gets W + ceil(drift * n)
    letters of slack for the indels that move an alignment off its seeds' diagonal."""
    slack = bin_width + int(np.ceil(drift * n))
    return bin_ * bin_width - DIAG0 - slack, (bin_ + 2) * bin_width - DIAG0 + n + slack


def align_runs(qlens, wlens, limit):
    """Cut a batch into consecutive runs [lo, hi) whose aligner workspace (slk_align_local_workspace_bytes: 24 bytes per row of
    the longest query for every pair of a launch whose longest window is wider than one pass) stays within `limit` bytes; a pair
    above the limit on its own is a run of one.  None: one run."""
    n = len(qlens)
    if limit is None or n == 0:
        return [(0, n)]
    P = align.PASS_WIDTH
    runs, lo, mq, mw = [], 0, 0, 0
    for r in range(n):
        q2, w2 = max(mq, int(qlens[r])), max(mw, int(wlens[r]))
        if r > lo and w2 > P and (r - lo + 1) * 24 * q2 > limit:
            runs.append((lo, r))
            lo, q2, w2 = r, int(qlens[r]), int(wlens[r])
        mq, mw = q2, w2
    runs.append((lo, n))
    return runs


class Index(object):
    """A genome on the device with the sorted keys of its k-mers.

    contigs: a dict name -> sequence or a list of (name, sequence); sequences are str (upper-cased), bytes or uint8 arrays.
    k: seed length, 8..15 (14 is bwa's -k14 of align.py:22).  bin_width: W, a power of two; the vote counts diagonals in half
    overlapping bins of 2 W.  max_occ: a k-mer with more occurrences in the genome casts no vote."""

    def __init__(self, contigs, k=14, bin_width=256, max_occ=64):
        items = list(contigs.items()) if isinstance(contigs, dict) else [(n, s) for n, s in contigs]
        if int(k) != k or k < MIN_K or k > MAX_K:
            raise ValueError("genome: k = %r outside %d..%d" % (k, MIN_K, MAX_K))
        if int(bin_width) != bin_width or bin_width < 2 or bin_width > MAX_BIN_WIDTH or bin_width & (bin_width - 1):
            raise ValueError("genome: bin_width = %r is not a power of two in 2..%d" % (bin_width, MAX_BIN_WIDTH))
        if int(max_occ) != max_occ or max_occ < 1 or max_occ > MAX_OCC:
            raise ValueError("genome: max_occ = %r outside 1..%d" % (max_occ, MAX_OCC))
        seqs = [align._as_u8(s) for _, s in items]
        self.names = [n for n, _ in items]
        self.lengths = np.array([len(s) for s in seqs], dtype=np.int64)
        self.offsets = np.concatenate(([0], np.cumsum(self.lengths))).astype(np.int64)
        self.G = int(self.offsets[-1])
        if self.G == 0:
            raise ValueError("genome: the genome is empty")
        if self.G >= MAX_GENOME:
            raise ValueError("genome: %d letters; the limit is 2^31 - 1 (positions are the low half of a 64-bit key)" % self.G)
        self.k, self.bin_width, self.max_occ = int(k), int(bin_width), int(max_occ)
        _lib.require_gpu()
        import torch
        from . import device as D
        dev = D.device()
        self.genome = torch.from_numpy(np.concatenate(seqs)).to(dev)
        self.offsets_dev = torch.from_numpy(self.offsets).to(dev)
        keys = torch.empty(self.G, dtype=torch.int64, device=dev)
        count = torch.zeros(1, dtype=torch.int32, device=dev)
        _lib.check(_lib.lib().slk_genome_kmer_keys_u8(self.genome.data_ptr(), self.offsets_dev.data_ptr(), len(seqs), self.G, self.k,
                                                      keys.data_ptr(), count.data_ptr(), D.stream_ptr()), "genome_kmer_keys")
        self.keys = torch.sort(keys).values                     # distinct keys: the order is unique, positions ascend within a code
        self.nvalid = int(count.item())

    @classmethod
    def from_fasta(cls, path, **kw):
        """An index of every record of a FASTA file, in file order (lower case is upper-cased; an 'N' only breaks its k-mers)."""
        return cls(util.fasta_records(path), **kw)

    def contig_of(self, pos):
        """Index of the contig that holds position `pos` of the packed genome."""
        return int(np.searchsorted(self.offsets, pos, side='right')) - 1

    # ---- seed and vote ---------------------------------------------------------------------------------------------------------

    def _upload(self, queries):
        import torch
        from . import device as D
        qs = [align._as_u8(x) for x in queries]
        B = len(qs)
        lens = np.array([len(x) for x in qs], dtype=np.int32)
        max_qlen = int(lens.max()) if B else 0
        align._check_len(max_qlen, "a query")
        ldq = max(max_qlen, 1)
        qh = np.zeros((B, ldq), dtype=np.uint8)
        for b, x in enumerate(qs):
            qh[b, :len(x)] = x
        dev = D.device()
        return torch.from_numpy(qh).to(dev), ldq, torch.from_numpy(lens).to(dev), lens, max_qlen

    def _seed_device(self, q, ldq, qlen, max_qlen):
        """q:[B][ldq] uint8 and qlen:[B] int32 on the device -> host int32 [B, 2, 4]."""
        import torch
        from . import device as D
        L = _lib.lib()
        B = int(qlen.numel())
        if max_qlen + self.bin_width > DIAG0:
            raise ValueError("genome: a query of %d letters with bin_width %d: their sum may not exceed %d"
                             % (max_qlen, self.bin_width, DIAG0))
        if B == 0:
            return np.zeros((0, 2, 4), dtype=np.int32)
        nbytes = L.slk_genome_seed_workspace_bytes(B, max_qlen, self.G, self.bin_width)
        ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=qlen.device)
        out = torch.empty((B, 2, 4), dtype=torch.int32, device=qlen.device)
        _lib.check(L.slk_genome_seed_votes_u8(q.data_ptr(), ldq, qlen.data_ptr(), B, max_qlen, self.keys.data_ptr(), self.nvalid,
                                              self.G, self.k, self.bin_width, self.max_occ, out.data_ptr(), ws.data_ptr(), nbytes,
                                              D.stream_ptr()), "genome_seed_votes")
        res = out.cpu().numpy()
        if (res[:, :, 0] < 0).any():
            raise ValueError("genome: a query on the device is longer than the bound it was launched with")
        return res

    def seed(self, queries):
        """The seed stage alone: host int32 [B, 2, 4], per query and strand (0 '+', 1 '-') the columns SEED_FIELDS as the kernel
        writes them: the bin of diagonals with the greatest count (ties to the smallest bin; 0 without a vote), that count, the
        greatest count among bins further than 2 from it, and the number of valid k-mers not skipped for max_occ."""
        q, ldq, qlen, _, max_qlen = self._upload(list(queries))
        return self._seed_device(q, ldq, qlen, max_qlen)

    # ---- cut ---------------------------------------------------------------------------------------------------------------------

    def cut(self, start, end, minus):
        """Spans [start[b], end[b]) of the PACKED genome, reverse-complemented where minus[b], end to end on the device
        (slk_genome_windows_u8) -> (uint8 device tensor, host int64 offsets [B + 1], device tensor of the offsets)."""
        import torch
        from . import device as D
        start, end = np.asarray(start, dtype=np.int64), np.asarray(end, dtype=np.int64)
        if ((start < 0) | (end < start) | (end > self.G)).any():
            raise ValueError("genome: a span outside the genome")
        lens = end - start
        off = np.concatenate(([0], np.cumsum(lens))).astype(np.int64)
        dev = self.genome.device
        out = torch.empty(max(int(off[-1]), 8), dtype=torch.uint8, device=dev)
        off_d = torch.from_numpy(off).to(dev)
        if len(lens) and off[-1]:
            start_d, end_d = torch.from_numpy(start).to(dev), torch.from_numpy(end).to(dev)
            minus_d = torch.from_numpy(np.ascontiguousarray(minus, dtype=np.int32)).to(dev)
            _lib.check(_lib.lib().slk_genome_windows_u8(self.genome.data_ptr(), self.G, start_d.data_ptr(), end_d.data_ptr(),
                                                        minus_d.data_ptr(), off_d.data_ptr(), len(lens), int(lens.max()),
                                                        out.data_ptr(), D.stream_ptr()), "genome_windows")
        return out, off, off_d

    # ---- map ---------------------------------------------------------------------------------------------------------------------

    def _map_device(self, q, ldq, qlen, lens, max_qlen, names, drift, min_votes, scores, workspace_limit, ops=False, qual=None):
        B = len(lens)
        seeds = self._seed_device(q, ldq, qlen, max_qlen)
        W = self.bin_width
        minus = seeds[:, 1, 1] > seeds[:, 0, 1]                 # more votes wins; a tie goes to '+'
        pick = np.where(minus[:, None], seeds[:, 1, :], seeds[:, 0, :]) if B else np.zeros((0, 4), dtype=np.int32)
        mapped = pick[:, 1] >= max(int(min_votes), 1)
        ws, we = np.zeros(B, dtype=np.int64), np.zeros(B, dtype=np.int64)
        contig = np.full(B, -1, dtype=np.int32)
        for b in np.flatnonzero(mapped):
            s, e = window_of(int(pick[b, 0]), int(lens[b]), W, drift)
            c = self.contig_of(min(max((s + e) // 2, 0), self.G - 1))
            s, e = max(s, int(self.offsets[c])), min(e, int(self.offsets[c + 1]))
            if e - s > align.MAX_LEN:
                raise ValueError("genome: the window of read %s is %d letters long; the aligner's limit is %d (a smaller drift, or "
                                 "shorter reads)" % (names[b] if names is not None else b, e - s, align.MAX_LEN))
            if e <= s:
                mapped[b] = False
                continue
            ws[b], we[b], contig[b] = s, e, c
        strand = np.where(minus & mapped, '-', '+').astype('U1')
        wlens = we - ws
        ref, roff, roff_d = self.cut(ws, we, strand == '-')
        res = np.zeros((B, 9), dtype=np.int32)
        device_rows = []
        for lo, hi in align_runs(lens, wlens, workspace_limit):
            if hi > lo:
                parts = [] if ops else None
                res[lo:hi], _ = align._align_device(q[lo:hi], ldq, qlen[lo:hi], int(lens[lo:hi].max()), ref, roff_d[lo:hi + 1],
                                                    wlens[lo:hi], scores, False, parts_out=parts)
                if ops:
                    device_rows.append(parts[0][2])
        columns = None
        if ops:                                                 # on the rows as the windows' launches left them: window coordinates
            import torch
            rows_d = torch.cat(device_rows) if device_rows else torch.zeros((0, 9), dtype=torch.int32, device=qlen.device)
            columns = align._traceback_device(q, ldq, qlen, [(ref, roff_d, rows_d, np.ones(B, dtype=bool))], res.copy(), scores,
                                              workspace_limit)
            columns.qual = qual                                 # [B][ldq] bytes beside the letters, or None; never fetched here
        edge = np.zeros(B, dtype=np.int32)
        for b in np.flatnonzero(res[:, 0] > 0):
            rs, re = int(res[b, 3]), int(res[b, 4])
            head, tail = res[b, 1] > 0, res[b, 2] < lens[b]     # unaligned query letters in front of / behind the alignment
            if strand[b] == '-':                                # window coordinates back to the forward strand
                rs, re = int(wlens[b]) - re, int(wlens[b]) - rs
                head, tail = tail, head
            c0, c1 = int(self.offsets[contig[b]]), int(self.offsets[contig[b] + 1])
            edge[b] = int((rs == 0 and ws[b] > c0 and head) or (re == wlens[b] and we[b] < c1 and tail))
            res[b, 3], res[b, 4] = rs + ws[b] - c0, re + ws[b] - c0
        contig[res[:, 0] <= 0] = -1                              # (a window in which nothing aligns: unmapped as well)
        strand[contig < 0] = '+'
        info = {'contig': contig, 'votes': pick[:, 1].astype(np.int32), 'second': pick[:, 2].astype(np.int32), 'edge': edge,
                'window_start': ws, 'window_end': we, 'seeds': seeds}
        return (res, strand, info, columns) if ops else (res, strand, info)

    def map(self, queries, drift=1.0 / 16, min_votes=3, match=1, mismatch=2, gap_open=2, gap_extend=1, workspace_limit=None,
            names=None, ops=False, quals=None):
        """Place every query on the genome and align it there.  -> (res, strand, info).

        The strand with more votes wins (a tie goes to '+'); a query with fewer than min_votes is unmapped: its row of `res` is all
        0 and info['contig'] = -1.  The window of a query of n letters whose winning bin is b is, with slack = W + ceil(drift * n),
        [b W - 65536 - slack, (b + 2) W - 65536 + n + slack) clipped to the contig that holds its midpoint; a window longer than
        65535 letters raises a ValueError that names the read.  The windows are cut on the device ('-' ones reverse-complemented)
        and ONE slk_align_local_batch_u8 launch aligns the queries as they are against them (workspace_limit: bytes of aligner
        workspace per launch; the batch is then split into consecutive launches, with the same rows).

        res:[B, 9] int32 has align.FIELDS; r_start / r_end are forward-strand coordinates WITHIN THE CONTIG, as a SAM record gives
        them, the counts of a '-' row those of the alignment against the reverse complement.  info: dict of arrays -- `contig`
        (index into Index.names, -1 unmapped), `votes`, `second` (the best count among bins further than 2 from the winner: a
        second locus), `edge` (1: the alignment touches a window end that is not a contig end while the query has unaligned letters
        on that side -- rerun with a larger drift; nothing is widened silently), `window_start` / `window_end` (packed-genome
        coordinates) and `seeds`, the kernel's rows.

        ops=True: one more value, the alignments' columns as an align.Ops (slk_align_traceback_batch_u8 on the windows: its rows
        are in window coordinates, for '-' against the reverse-complemented window; workspace_limit bounds the traceback's
        workspace per launch as well).  sam_records turns them into SAM lines.

        quals: one uint8 array per query, a quality per letter (FASTQ input; bio.fastq_records gives them).  They are uploaded
        beside the letters, with the same pitch, and kept on the returned Ops as `ops.qual` for a weighted Pileup; they take no part
        in the mapping.  An array whose length is not its query's raises a ValueError that names the read."""
        align._check_scores(match, mismatch, gap_open, gap_extend)
        queries = list(queries)
        _lib.require_gpu()
        q, ldq, qlen, lens, max_qlen = self._upload(queries)
        qual = None
        if quals is not None:
            import torch
            quals = list(quals)
            if len(quals) != len(queries):
                raise ValueError("genome: quals= holds %d arrays for %d queries" % (len(quals), len(queries)))
            vh = np.zeros((len(queries), ldq), dtype=np.uint8)
            for b, v in enumerate(quals):
                v = np.asarray(v)
                if v.ndim != 1 or len(v) != lens[b]:
                    raise ValueError("genome: quals= of read %s has %d values for %d letters"
                                     % (names[b] if names is not None else b, v.size, lens[b]))
                vh[b, :len(v)] = v
            qual = torch.from_numpy(vh).to(q.device)
        return self._map_device(q, ldq, qlen, lens, max_qlen, names, drift, min_votes,
                                (int(match), int(mismatch), int(gap_open), int(gap_extend)), workspace_limit, ops, qual)

    def map_paths(self, paths, lens, kmer_len, alphabet='ACGT', drift=1.0 / 16, min_votes=3, match=1, mismatch=2, gap_open=2,
                  gap_extend=1, workspace_limit=None, names=None, ops=False, conf=None, qmax=60):
        """`map` of decoded paths without the called sequences leaving the device: paths:[B, T] int32 device tensor of k-mer states
        and lens:[B] int32 device tensor, as any `call_*` returns them, become bases through slk_paths_to_bases(always_move=True)
        and that buffer is the query operand of the seed stage and of the aligner as it lies.  Only the base counts come to the
        host.  -> (res, strand, info, nbases), with ops=True one more value, the align.Ops of `map`.

        conf: the float64 [B, T] device tensor of call_chunks_qual / decode.viterbi_marginals_batch.  The bases then come from
        slk_paths_to_bases_qual (the same letters) and its quality buffer, Phred values capped at qmax with the pitch of the bases,
        stays on the device as `ops.qual` for a weighted Pileup.  The rows do not depend on it."""
        import torch
        from . import device as D
        align._check_scores(match, mismatch, gap_open, gap_extend)
        _lib.require_gpu()
        B, Tmax = paths.shape
        if lens.numel() != B:
            raise ValueError("genome: %d paths but %d lengths" % (B, lens.numel()))
        if isinstance(alphabet, str):
            alphabet = alphabet.encode('utf-8')
        cap = max(kmer_len * max(Tmax, 1), kmer_len)
        bases = torch.empty((B, cap), dtype=torch.uint8, device=paths.device)
        nb = torch.empty((B,), dtype=torch.int32, device=paths.device)
        qual = None
        if conf is None:
            _lib.check(_lib.lib().slk_paths_to_bases(paths.data_ptr(), paths.stride(0), lens.data_ptr(), B, kmer_len, len(alphabet), 1,
                                                     int.from_bytes(alphabet.ljust(8, b'\0'), 'little'), bases.data_ptr(), cap,
                                                     nb.data_ptr(), D.stream_ptr()), "paths_to_bases")
        else:
            from . import bio
            if conf.dtype != torch.float64 or conf.shape[0] != B or conf.shape[1] < Tmax or conf.stride(1) != 1:
                raise ValueError("genome: conf= must be a float64 device tensor with one row per path and one entry per position")
            table = torch.from_numpy(bio.phred_thresholds(qmax)).to(paths.device)
            qual = torch.zeros((B, cap), dtype=torch.uint8, device=paths.device)
            _lib.check(_lib.lib().slk_paths_to_bases_qual(paths.data_ptr(), paths.stride(0), lens.data_ptr(), conf.data_ptr(),
                                                          conf.stride(0), table.data_ptr(), int(qmax), B, kmer_len, len(alphabet), 1,
                                                          int.from_bytes(alphabet.ljust(8, b'\0'), 'little'), bases.data_ptr(),
                                                          qual.data_ptr(), cap, nb.data_ptr(), D.stream_ptr()), "paths_to_bases_qual")
        counts = nb.cpu().numpy()
        max_qlen = int(counts.max()) if B else 0
        align._check_len(max_qlen, "a query")
        got = self._map_device(bases, cap, nb, counts, max_qlen, names, drift, min_votes,
                               (int(match), int(mismatch), int(gap_open), int(gap_extend)), workspace_limit, ops, qual)
        return got[:3] + (counts,) + got[3:]


def sam_records(index, res, strand, info, ops, names, queries=None):
    """SAM lines of the rows of Index.map / map_paths (ops=True), one per read, by align.sam_records' field rules: RNAME is the
    contig's name and POS the 1-based forward-strand position WITHIN the contig; a read without a contig gets FLAG 4.
    align.sam_text(zip(index.names, index.lengths), records) adds the header.  queries: the reads' letters, or None for SEQ '*'
    (ops.queries() fetches calls that never left the device: that is what this export is for)."""
    n = ops.query_lengths()
    out = []
    for b in range(len(res)):
        c = int(info['contig'][b])
        row = res[b] if c >= 0 else np.zeros(9, dtype=np.int32)
        out.append(align.sam_record(names[b] if names is not None else b, row, str(strand[b]), ops.codes(b), n[b],
                                    index.names[c] if c >= 0 else '*', None if queries is None else queries[b]))
    return out


def samacc_rows(index, res, strand, info, query_lengths, names=None, min_coverage=0.6):
    """align.samacc_rows on the rows of Index.map, with the reference's leading 'reference' column (the contig's name,
    align.py:118).  align.summary applies to the result unchanged."""
    rows = []
    for row in align.samacc_rows(res, strand, query_lengths, names=None, min_coverage=min_coverage):
        b = row['query']
        out = {'reference': index.names[int(info['contig'][b])], 'query': names[b] if names is not None else b}
        out.update((key, val) for key, val in row.items() if key != 'query')
        rows.append(out)
    return rows


def reference_span(res_row, strand, n, contig_len, pad=50):
    """get_refs_from_sam.py:57-58 in this project's terms: pysam's query_alignment_start / _end are on the sequence as stored in
    the SAM record, which for '-' is the reverse complement of the read, so lead = q_start, tail = n - q_end for '+' and
    lead = n - q_end, tail = q_start for '-'.  -> (start, end) within the contig."""
    qs, qe, rs, re = (int(res_row[j]) for j in (1, 2, 3, 4))
    lead, tail = (qs, n - qe) if strand == '+' else (n - qe, qs)
    return max(0, rs - lead - pad), min(int(contig_len), re + tail + pad)


def reference_spans(contig_lengths, contig_offsets, res, strand, contig, query_lengths, min_coverage=0.6, pad=50):
    """The host half of read_references: which reads get a reference (get_refs_from_sam.py:46-55) and the span of the PACKED genome
    each is cut from -> (indices of the reads kept, starts, ends)."""
    res = np.asarray(res)
    keep, start, end = [], [], []
    for b in range(len(res)):
        n, c = int(query_lengths[b]), int(contig[b])
        if c < 0 or res[b, 0] <= 0 or n <= 0 or float(res[b, 2] - res[b, 1]) / n < min_coverage:
            continue
        s, e = reference_span(res[b], strand[b], n, contig_lengths[c], pad)
        keep.append(b)
        start.append(s + int(contig_offsets[c]))
        end.append(e + int(contig_offsets[c]))
    return keep, start, end


def read_references(index, res, strand, info, query_lengths, names, min_coverage=0.6, pad=50):
    """One padded, strand-corrected reference per mapped read: get_refs (get_refs_from_sam.py:40-68) on the rows of Index.map.
    -> ([(name, sequence str)], [strand-list names]).  Unmapped reads and reads whose aligned part is under min_coverage of their
    length are dropped; the sequence is contig[start:end] (reference_span), reverse-complemented for '-', cut on the device by
    slk_genome_windows_u8; the record's name has a '.fast5' extension trimmed, the strand-list name is name + '.fast5'."""
    keep, start, end = reference_spans(index.lengths, index.offsets, res, strand, info['contig'], query_lengths, min_coverage, pad)
    if not keep:
        return [], []
    out, off, _ = index.cut(start, end, [strand[b] == '-' for b in keep])
    text = out.cpu().numpy().tobytes().decode('ascii')
    records = [(trim_fast5_extension(names[b]), text[off[j]:off[j + 1]]) for j, b in enumerate(keep)]
    return records, [names[b] + ".fast5" for b in keep]


# ---- pileup and consensus (csrc/pileup.hip, design/pileup.md) ----------------------------------------------------------------------

#: entries of a row of Pileup.counts(): query letters by class, deletions, reads with an insertion behind the position, and `span`,
#: the reads whose alignment covers this reference letter and the next one
PILEUP_FIELDS = ("A", "C", "G", "T", "other", "deletion", "insertion_reads", "span")
MAX_INS = 16
#: bits of Consensus.flags (include/sloika_amd.h: SLK_PILEUP_FLAG_*)
FLAG_LOW, FLAG_CHANGED, FLAG_INSERTED = 1, 2, 4
#: per-pair status of Pileup.add (include/sloika_amd.h: SLK_PILEUP_*)
PILEUP_DONE, PILEUP_SKIPPED = 0, 1
PILEUP_REASONS = {
    -1: "a span of its row lies outside the sequences",
    -2: "its row has a negative count",
    -3: "the spans of its row are not the sums of its counts",
    -4: "its slice of the column codes does not have the length of its alignment",
    -5: "its alignment does not lie inside the packed genome",
    -6: "a byte of its columns is no column code",
    -7: "its columns of a kind are not as many as its row says",
}
#: the largest qmax of a weighted Pileup (bio.PHRED_MAX: Phred + 33 stays printable)
QMAX_LIMIT = 93


def quality_weights(min_qual=0, qmax=60):
    """uint8 [256], the weight of a letter by its quality byte (design/pileup.md section 9): 0 below min_qual, else min(v, qmax)."""
    v = np.arange(256)
    return np.where(v < min_qual, 0, np.minimum(v, qmax)).astype(np.uint8)


def region_span(index, region):
    """region=(contig name or index, start, end) within that contig, or None for the whole genome -> (first packed position, number of
    positions), as Pileup reads it."""
    if region is None:
        return 0, index.G
    c, start, end = region
    if not isinstance(c, (int, np.integer)):
        if c not in index.names:
            raise ValueError("genome: region= names the contig %r, which the index does not hold" % (c,))
        c = index.names.index(c)
    if c < 0 or c >= len(index.names) or start < 0 or end < start or end > index.lengths[c]:
        raise ValueError("genome: region=%r lies outside the contig" % (region,))
    return int(index.offsets[c]) + int(start), int(end) - int(start)


class Pileup(object):
    """Zeroed count tables on the device for a span of the packed genome of `index`, to which batches of mapped reads are added
    (design/pileup.md section 1 defines every quantity).

    region: (contig name or index, start, end) within that contig, or None for the whole genome.  max_ins: S, the insertion
    letters kept per position, 1..16.  The tables take (8 + 5 S) * 4 bytes per position; a span that needs more than memory_limit
    raises a ValueError: pile such a genome region by region.

    weighted=True: a second pair of tables of the same shapes (wcounts_dev, wins_dev) holds sums of per-letter weights beside the
    counts (design/pileup.md section 9), the memory check counts both pairs, and `add` needs the reads' qualities.  The weight of
    a letter whose quality byte is v is weights[v]: 0 below min_qual, else min(v, qmax) (qmax 1..93); weights= passes a table of
    256 bytes of the caller's own instead.  The decoder's Phred values order letters and are not calibrated error probabilities
    (design/lattice_marginals.md section 6): a sum of them is a definition, not a likelihood."""

    def __init__(self, index, region=None, max_ins=4, memory_limit=transducer.WORKSPACE_LIMIT, weighted=False, min_qual=0, qmax=60,
                 weights=None):
        import torch
        if int(max_ins) != max_ins or max_ins < 1 or max_ins > MAX_INS:
            raise ValueError("genome: max_ins = %r outside 1..%d" % (max_ins, MAX_INS))
        if int(qmax) != qmax or qmax < 1 or qmax > QMAX_LIMIT:
            raise ValueError("genome: qmax = %r outside 1..%d" % (qmax, QMAX_LIMIT))
        self.index, self.S = index, int(max_ins)
        self.weighted, self.qmax = bool(weighted), int(qmax)
        if weights is None:
            weights = quality_weights(min_qual, qmax)
        weights = np.asarray(weights)
        if weights.shape != (256,) or weights.min() < 0 or weights.max() > 255:
            raise ValueError("genome: weights= is a table of 256 values in 0..255")
        self.weights = weights.astype(np.uint8)
        if region is None:
            self.lo, self.hi = 0, index.G
        else:
            c, start, end = region
            if not isinstance(c, (int, np.integer)):
                if c not in index.names:
                    raise ValueError("genome: region= names the contig %r, which the index does not hold" % (c,))
                c = index.names.index(c)
            if c < 0 or c >= len(index.names) or start < 0 or end < start or end > index.lengths[c]:
                raise ValueError("genome: region=%r lies outside the contig" % (region,))
            self.lo, self.hi = int(index.offsets[c]) + int(start), int(index.offsets[c]) + int(end)
        self.P = self.hi - self.lo
        nbytes = self.P * (8 + 5 * self.S) * 4 * (2 if self.weighted else 1)
        if nbytes > memory_limit:
            raise ValueError("genome: the %stables of %d positions take %d bytes, above the limit of %d: pile it in pieces with region="
                             % ("two pairs of " if self.weighted else "", self.P, nbytes, memory_limit))
        dev = index.genome.device
        self.counts_dev = torch.zeros((max(self.P, 1), 8), dtype=torch.int32, device=dev)
        self.ins_dev = torch.zeros((max(self.P, 1), self.S, 5), dtype=torch.int32, device=dev)
        self.wcounts_dev = self.wins_dev = self.weights_dev = None
        if self.weighted:
            self.wcounts_dev, self.wins_dev = torch.zeros_like(self.counts_dev), torch.zeros_like(self.ins_dev)
            self.weights_dev = torch.from_numpy(self.weights).to(dev)
        self.status = np.zeros(0, dtype=np.int32)
        self._fcodes = self._offsets = None
        self._names = None

    def add(self, res, strand, info, ops, keep=None, normalise=True, names=None, qual=None):
        """Add the alignments of one batch: the values Index.map / map_paths return with ops=True.  keep: bool mask of the reads to
        add (info['edge'] == 0 is the usual filter: an alignment cut by its window's end says nothing about the letters behind
        it); unmapped reads and empty alignments are skipped anyway.  normalise: move every gap as far to the front of the forward
        strand as its letters allow, so that both strands vote for the same place; off only to study the aligner's own placement.
        -> host int32 status per read: PILEUP_DONE, PILEUP_SKIPPED or a negative code of PILEUP_REASONS (then nothing of the read
        was added; `check` / `columns` raise a ValueError that names it).  May be called any number of times.

        A weighted Pileup also needs a quality byte per query letter: `ops.qual`, as Index.map(quals=) and map_paths(conf=) leave
        it, or qual=, a uint8 device tensor [B, ops.ldq]; without either it raises a ValueError.  An unweighted Pileup looks at
        neither."""
        import torch
        from . import device as D
        B = len(ops)
        if self.weighted:
            if qual is None:
                qual = getattr(ops, 'qual', None)
            if qual is None:
                raise ValueError("genome: a weighted pileup needs the reads' qualities: map with quals= / conf= (ops.qual) or pass "
                                 "qual=")
            if qual.dtype != torch.uint8 or tuple(qual.shape) != (B, ops.ldq) or not qual.is_contiguous() or \
                    qual.device != ops.codes_dev.device:
                raise ValueError("genome: qual= must be a contiguous uint8 device tensor of shape (%d, %d), the pitch of the queries"
                                 % (B, ops.ldq))
        if len(res) != B or len(strand) != B:
            raise ValueError("genome: %d rows but the columns of %d reads" % (len(res), B))
        keep = np.ones(B, dtype=bool) if keep is None else np.asarray(keep, dtype=bool)
        if keep.shape != (B,):
            raise ValueError("genome: keep= is a mask of %d reads, not of %d" % (keep.size, B))
        self._names = names
        self._fcodes, self._offsets = None, ops.offsets
        self.status = np.zeros(B, dtype=np.int32)
        if B == 0:
            return self.status
        if len(ops.parts) != 1:
            raise ValueError("genome: a pileup takes the columns of Index.map / map_paths (one reference buffer)")
        ref, roff, rows_d, tb_d = ops.parts[0]
        dev = ops.codes_dev.device
        minus = np.asarray(strand) == '-'
        rows = np.asarray(ops.rows)
        t0 = np.where(minus, np.asarray(info['window_end'], dtype=np.int64) - rows[:, 4],
                      np.asarray(info['window_start'], dtype=np.int64) + rows[:, 3]).astype(np.int64)
        minus_d = torch.from_numpy(minus.astype(np.int32)).to(dev)
        keep_d = torch.from_numpy(keep.astype(np.uint8)).to(dev)
        t0_d = torch.from_numpy(t0).to(dev)
        fcodes = torch.zeros_like(ops.codes_dev)
        st_d = torch.empty(B, dtype=torch.int32, device=dev)
        L = _lib.lib()
        _lib.check(L.slk_pileup_columns_u8(ops.q.data_ptr(), ops.ldq, ops.qlen.data_ptr(), ref.data_ptr(), roff.data_ptr(),
                                           rows_d.data_ptr(), ops.codes_dev.data_ptr(), ops.offsets_dev.data_ptr(),
                                           ops.codes_dev.numel(), tb_d.data_ptr(), minus_d.data_ptr(), keep_d.data_ptr(),
                                           t0_d.data_ptr(), self.index.G, B, int(bool(normalise)), fcodes.data_ptr(),
                                           st_d.data_ptr(), D.stream_ptr()), "pileup_columns")
        if self.weighted:
            _lib.check(L.slk_pileup_count_qual_u8(ops.q.data_ptr(), ops.ldq, ops.qlen.data_ptr(), qual.data_ptr(), roff.data_ptr(),
                                                  rows_d.data_ptr(), fcodes.data_ptr(), ops.offsets_dev.data_ptr(), fcodes.numel(),
                                                  st_d.data_ptr(), minus_d.data_ptr(), t0_d.data_ptr(), self.index.G, B, self.lo,
                                                  self.hi, self.S, self.weights_dev.data_ptr(), self.counts_dev.data_ptr(),
                                                  self.ins_dev.data_ptr(), self.wcounts_dev.data_ptr(), self.wins_dev.data_ptr(),
                                                  D.stream_ptr()), "pileup_count_qual")
        else:
            _lib.check(L.slk_pileup_count_u8(ops.q.data_ptr(), ops.ldq, ops.qlen.data_ptr(), roff.data_ptr(), rows_d.data_ptr(),
                                             fcodes.data_ptr(), ops.offsets_dev.data_ptr(), fcodes.numel(), st_d.data_ptr(),
                                             minus_d.data_ptr(), t0_d.data_ptr(), self.index.G, B, self.lo, self.hi, self.S,
                                             self.counts_dev.data_ptr(), self.ins_dev.data_ptr(), D.stream_ptr()), "pileup_count")
        self.status = st_d.cpu().numpy()
        self._fcodes = fcodes
        return self.status

    def check(self, b):
        if self.status[b] < 0:
            raise ValueError("genome: read %s was not piled: %s"
                             % (self._names[b] if self._names is not None else b,
                                PILEUP_REASONS.get(int(self.status[b]), "status %d" % self.status[b])))

    def columns(self, b):
        """uint8 host array: the forward-view codes of read b of the last `add` (empty for a read that was skipped)."""
        self.check(b)
        if self.status[b] != PILEUP_DONE or self._fcodes is None:
            return np.zeros(0, dtype=np.uint8)
        if not isinstance(self._fcodes, np.ndarray):
            self._fcodes = self._fcodes.cpu().numpy()
        return self._fcodes[self._offsets[b]:self._offsets[b + 1]]

    def counts(self):
        """Host int32 [P, 8] (PILEUP_FIELDS)."""
        return self.counts_dev[:self.P].cpu().numpy()

    def insertions(self):
        """Host int32 [P, max_ins, 5]: classes A C G T other of the k-th letter of an insertion behind the position."""
        return self.ins_dev[:self.P].cpu().numpy()

    def _need_weighted(self, what):
        if not self.weighted:
            raise ValueError("genome: %s needs a Pileup made with weighted=True" % what)

    def weighted_counts(self):
        """Host int32 [P, 8]: the sums of weights at the entries of `counts()`."""
        self._need_weighted("weighted_counts()")
        return self.wcounts_dev[:self.P].cpu().numpy()

    def weighted_insertions(self):
        """Host int32 [P, max_ins, 5]: the sums of weights at the entries of `insertions()`."""
        self._need_weighted("weighted_insertions()")
        return self.wins_dev[:self.P].cpu().numpy()

    def consensus(self, min_depth=3, weighted=None):
        """The call of every position -> Consensus.  weighted: None for the Pileup's own mode; True the weighted call of
        slk_pileup_call_qual_u8 (a ValueError on a Pileup without weighted tables), whose Consensus has a quality per letter; False
        the majority call of slk_pileup_call_u8 from the plain tables, which a weighted Pileup holds as well."""
        import torch
        from . import device as D
        weighted = self.weighted if weighted is None else bool(weighted)
        if weighted:
            self._need_weighted("consensus(weighted=True)")
        dev = self.counts_dev.device
        n = max(self.P, 1)
        letters = torch.zeros((n, 1 + self.S), dtype=torch.uint8, device=dev)
        nlet = torch.zeros(n, dtype=torch.uint8, device=dev)
        flags = torch.zeros(n, dtype=torch.uint8, device=dev)
        if weighted:
            letq = torch.zeros((n, 1 + self.S), dtype=torch.uint8, device=dev)
            posq = torch.zeros(n, dtype=torch.uint8, device=dev)
            _lib.check(_lib.lib().slk_pileup_call_qual_u8(self.counts_dev.data_ptr(), self.ins_dev.data_ptr(),
                                                          self.wcounts_dev.data_ptr(), self.wins_dev.data_ptr(),
                                                          self.index.genome.data_ptr(), self.index.G, self.lo, self.hi, self.S,
                                                          int(min_depth), self.qmax, letters.data_ptr(), nlet.data_ptr(),
                                                          flags.data_ptr(), letq.data_ptr(), posq.data_ptr(), D.stream_ptr()),
                       "pileup_call_qual")
            return Consensus(self, letters[:self.P], nlet[:self.P], flags[:self.P], int(min_depth), letq[:self.P], posq[:self.P])
        _lib.check(_lib.lib().slk_pileup_call_u8(self.counts_dev.data_ptr(), self.ins_dev.data_ptr(), self.index.genome.data_ptr(),
                                                 self.index.G, self.lo, self.hi, self.S, int(min_depth), letters.data_ptr(),
                                                 nlet.data_ptr(), flags.data_ptr(), D.stream_ptr()), "pileup_call")
        return Consensus(self, letters[:self.P], nlet[:self.P], flags[:self.P], int(min_depth))

    def alleles(self, kmer_len, min_count=2, min_fraction=0.2, min_depth=3, max_del=8):
        """The variants the pileup's own disagreeing reads propose (slk_pileup_alleles_count / _emit; design/genotypes.md 1.1), the
        minority ones too: at every position whose reference letter is one of A C G T, the insertion in front of it, the
        substitutions and the deletion run that starts there whose counts n pass n >= min_count, 1000 n >= permille x depth and
        depth >= min_depth (permille = round(1000 min_fraction); depth the position's own, an insertion's the `span` of the
        position in front).  An insertion of more than polish.max_alt(kmer_len) letters and a deletion run of more than max_del
        are not proposed and counted in `skipped`.  Runs and insertions are cut at the Pileup's span.  Each variant stands against
        the reference alone; overlapping alleles are separate variants.
        -> polish.VariantSet, sorted as it comes, with `skipped` = {'insertion': positions, 'deletion': runs} and `skipped_dev`,
        int32 [P] on the device (bit 1: the insertion in front, bit 2: the run that starts there)."""
        import torch
        from . import device as D, polish
        permille = int(round(1000.0 * float(min_fraction)))
        if min(int(min_count), int(min_depth), int(max_del)) < 1 or not 1 <= permille <= 1000 or int(max_del) > 1 << 20:
            raise ValueError("genome: alleles needs min_count, min_depth >= 1, max_del 1 .. 2^20 and min_fraction in (0, 1], not %r"
                             % ((min_count, min_depth, max_del, min_fraction),))
        polish._check_kmer_len(kmer_len)
        ix, P = self.index, self.P
        dev = self.counts_dev.device
        coff = polish._contig_offsets(ix, dev)
        L, st = _lib.lib(), D.stream_ptr()
        head = (self.counts_dev.data_ptr(), self.ins_dev.data_ptr(), ix.genome.data_ptr(), int(ix.G), coff.data_ptr(), len(ix.names),
                self.lo, P, self.S, int(kmer_len), int(min_depth), int(min_count), permille, int(max_del))
        offs = torch.zeros((2, P + 1), dtype=torch.int64, device=dev)
        skipped = torch.zeros(max(P, 1), dtype=torch.int32, device=dev)
        _lib.check(L.slk_pileup_alleles_count(*head, offs[0].data_ptr(), offs[1].data_ptr(), skipped.data_ptr(), st),
                   "pileup_alleles_count")
        offs = torch.cumsum(offs, 1)
        V, A = (int(v) for v in offs[:, -1].cpu().numpy())
        var_off = torch.zeros(V, dtype=torch.int64, device=dev)
        var_pos, var_ndel = torch.zeros_like(var_off), torch.zeros(V, dtype=torch.int32, device=dev)
        var_alt_off, var_alt = torch.zeros(V + 1, dtype=torch.int64, device=dev), torch.zeros(A, dtype=torch.uint8, device=dev)
        _lib.check(L.slk_pileup_alleles_emit(*head, offs[0].data_ptr(), offs[1].data_ptr(), V, A, var_off.data_ptr(), var_pos.data_ptr(),
                                             var_ndel.data_ptr(), var_alt_off.data_ptr(), var_alt.data_ptr(), st), "pileup_alleles_emit")
        out = polish.VariantSet(ix, var_off, var_pos, var_ndel, var_alt_off, var_alt, coff)
        out.skipped_dev = skipped[:P]
        out.prop_off, out.alt_off = offs[0], offs[1]
        out.skipped = {'insertion': int((out.skipped_dev & 1).ne(0).sum()), 'deletion': int((out.skipped_dev & 2).ne(0).sum())}
        return out


class Consensus(object):
    """The calls of a Pileup.  letters_dev:[P, 1 + max_ins] uint8, nlet_dev:[P], flags_dev:[P] on the device; `flags` the host copy
    (FLAG_LOW: too little depth, the genome's letter was kept; FLAG_CHANGED: a substitution or a deletion; FLAG_INSERTED).

    A weighted call (Pileup.consensus(weighted=True)) also has letq_dev:[P, 1 + max_ins], the quality of every emitted letter, and
    posq_dev:[P], the winner's lead over the runner-up per position (design/pileup.md section 9); `weighted` says which it is."""

    def __init__(self, pileup, letters, nlet, flags, min_depth, letq=None, posq=None):
        self.pileup, self.letters_dev, self.nlet_dev, self.flags_dev, self.min_depth = pileup, letters, nlet, flags, min_depth
        self.letq_dev, self.posq_dev, self.weighted = letq, posq, letq is not None
        self.flags = flags.cpu().numpy()

    def _selected(self, slots):
        """The first nlet[p] entries of every row of `slots` in order, cut per contig -> [(contig name, uint8 host array)]."""
        import torch
        pl, ix = self.pileup, self.pileup.index
        if pl.P == 0:
            return []
        width = slots.shape[1]
        mask = torch.arange(width, device=self.nlet_dev.device)[None, :] < self.nlet_dev[:, None]
        flat = slots[mask].cpu().numpy()
        ends = torch.cumsum(self.nlet_dev.to(torch.int64), 0).cpu().numpy()
        out = []
        for c in range(ix.contig_of(pl.lo), ix.contig_of(pl.hi - 1) + 1):
            s, e = max(int(ix.offsets[c]), pl.lo) - pl.lo, min(int(ix.offsets[c + 1]), pl.hi) - pl.lo
            if e > s:
                out.append((ix.names[c], flat[int(ends[s - 1]) if s else 0:int(ends[e - 1])]))
        return out

    def sequences(self):
        """[(contig name, str)]: the region's part of every contig it touches, in genome order: the selected letters in order
        (a mask and a cumulative sum on the device)."""
        return [(name, text.tobytes().decode('ascii')) for name, text in self._selected(self.letters_dev)]

    def qualities(self):
        """[(contig name, uint8 array)] of a weighted call, aligned letter for letter with `sequences()` (the same mask and
        cumulative sum on the device)."""
        if not self.weighted:
            raise ValueError("genome: qualities() needs a weighted call: Pileup(weighted=True).consensus()")
        return self._selected(self.letq_dev)

    def fastq(self):
        """FASTQ text of a weighted call, one record per contig (bio.fastq_text)."""
        from . import bio
        seqs, quals = self.sequences(), self.qualities()
        return bio.fastq_text([name for name, _ in seqs], [text for _, text in seqs], [v for _, v in quals])

    def variants(self, with_qual=False):
        """Host list of (contig name, position within the contig, kind, ref, alt, depth, support), in position order.  kind 'sub':
        ref and alt are letters, depth the position's depth (query letters + deletions) and support the winner's count; 'del': alt
        is '', support the deletions; 'ins': ref is '', alt the letters inserted BEHIND the position, depth its `span` entry and
        support the reads with an insertion there.  Gaps are left-normalised: one in a repeat is reported at the repeat's front.

        with_qual=True (a weighted call only) appends one value: the position's posq for 'sub' / 'del', the smallest quality among
        the inserted letters for 'ins'.  depth and support stay the unweighted counts; in a weighted call the winner is the one by
        weight."""
        if with_qual and not self.weighted:
            raise ValueError("genome: variants(with_qual=True) needs a weighted call: Pileup(weighted=True).consensus()")
        pl, ix = self.pileup, self.pileup.index
        hit = np.flatnonzero(self.flags & (FLAG_CHANGED | FLAG_INSERTED))
        if not len(hit):
            return []
        import torch
        hit_d = torch.from_numpy(hit).to(self.letters_dev.device)
        letters, nlet = self.letters_dev[hit_d].cpu().numpy(), self.nlet_dev[hit_d].cpu().numpy()
        counts, ref = pl.counts_dev[hit_d].cpu().numpy(), ix.genome[hit_d + pl.lo].cpu().numpy()
        votes = pl.wcounts_dev[hit_d].cpu().numpy() if self.weighted else counts       # what the winner was chosen by
        if with_qual:
            letq, posq = self.letq_dev[hit_d].cpu().numpy(), self.posq_dev[hit_d].cpu().numpy()
        out = []
        for k, p in enumerate(hit):
            c = ix.contig_of(pl.lo + int(p))
            pos, cn, text = pl.lo + int(p) - int(ix.offsets[c]), counts[k], letters[k, :nlet[k]].tobytes().decode('ascii')
            depth = int(cn[:6].sum())
            deleted = _deletion_wins(votes[k], chr(ref[k]))
            nins = len(text) - (0 if deleted else 1)
            if deleted:
                out.append((ix.names[c], pos, 'del', chr(ref[k]), '', depth, int(cn[5])) + ((int(posq[k]),) if with_qual else ()))
            elif self.flags[p] & FLAG_CHANGED:
                out.append((ix.names[c], pos, 'sub', chr(ref[k]), text[0], depth, int(cn["ACGT".index(text[0])]))
                           + ((int(posq[k]),) if with_qual else ()))
            if self.flags[p] & FLAG_INSERTED:
                out.append((ix.names[c], pos, 'ins', '', text[len(text) - nins:], int(cn[7]), int(cn[6]))
                           + ((int(letq[k, len(text) - nins:len(text)].min()),) if with_qual else ()))
        return out

    def polish_variants(self, rescored):
        """The rows of variants() with what the reads' signal says about exactly that edit beside them (the join of
        design/polish_genome.md): `rescored` a polish.GenomeRescored of reads mapped to the SAME index, the reference the pileup was
        made on.  Each row gets three more values: gain (float), support (int) and single (bool).  A substitution, a deletion and an
        insertion of one letter are one of the 8 cells of their position -- an insertion BEHIND position p is the insertion in front
        of p + 1 --; an insertion of more letters is not a single-letter edit: gain None, support 0, single False.  A variant outside
        the rescored region has gain None and support 0 as well, with single True.

        `rescored` may also be a polish.GenomeVariantsRescored of the variants `proposals()` returns, in that order
        (design/polish_variants.md): every row then gets the gain and support of its own variant -- an insertion of several letters
        too, and every row of a run of deleted positions those of the run's one deletion --, with `single` as above."""
        import torch
        if hasattr(rescored, 'variants'):
            return self._join_proposals(rescored)
        ix = self.pileup.index
        if rescored.index is not ix:
            raise ValueError("genome: polish_variants needs reads rescored against the index the pileup was made on")
        rows = self.variants()
        cells = []
        for name, pos, kind, ref, alt, _, _ in rows:
            cell = None
            if kind != 'ins' or len(alt) == 1:
                try:
                    p, slot = rescored.cell_of(name, pos + 1 if kind == 'ins' else pos, kind, alt)
                    cell = 8 * p + slot
                except ValueError:
                    cell = None
            cells.append(cell)
        have = [c for c in cells if c is not None]
        gain = support = []
        if have:
            at = torch.as_tensor(have, dtype=torch.int64, device=rescored.gain.device)
            gain, support = rescored.gain.reshape(-1)[at].cpu().numpy(), rescored.support.reshape(-1)[at].cpu().numpy()
        out, k = [], 0
        for row, cell in zip(rows, cells):
            single = row[2] != 'ins' or len(row[4]) == 1
            if cell is None:
                out.append(row + (None, 0, single))
            else:
                out.append(row + (float(gain[k]), int(support[k]), True))
                k += 1
        return out

    def proposals(self, max_alt=None):
        """The rows of variants() as variants (contig, pos, ndel, alt) for polish.rescore_variants (proposals_of): a substitution is
        (pos, 1, alt), a run of consecutive 'del' rows of one contig one (pos, run, ''), an 'ins' BEHIND p is (p + 1, 0, alt).
        max_alt: leave out insertions of more letters (polish.max_alt(kmer_len) is what an edit may bring)."""
        return proposals_of(self.variants(), max_alt)[0]

    def _join_proposals(self, rescored):
        if rescored.index is not self.pileup.index:
            raise ValueError("genome: polish_variants needs reads rescored against the index the pileup was made on")
        rows = self.variants()
        mine, which = proposals_of(rows)
        number = dict((v, i) for i, v in reversed(list(enumerate(rescored.variants.rows()))))
        gain, support = rescored.gain.cpu().numpy(), rescored.support.cpu().numpy()
        out = []
        for row, w in zip(rows, which):
            single = row[2] != 'ins' or len(row[4]) == 1
            v = None if w is None else number.get(mine[w])
            out.append(row + ((None, 0, single) if v is None else (float(gain[v]), int(support[v]), single)))
        return out

    def summary(self):
        """dict: `covered` (positions called, i.e. not FLAG_LOW), `substitutions`, `deleted` and `inserted` letters against the
        genome, and `identity` = 1 - their sum / covered (nan without a covered position)."""
        covered = int((self.flags & FLAG_LOW == 0).sum())
        sub = dele = ins = 0
        for _, _, kind, _, alt, _, _ in self.variants():
            if kind == 'sub':
                sub += 1
            elif kind == 'del':
                dele += 1
            else:
                ins += len(alt)
        return {'covered': covered, 'substitutions': sub, 'deleted': dele, 'inserted': ins,
                'identity': 1.0 - float(sub + dele + ins) / covered if covered else float('nan')}


def proposals_of(rows, max_alt=None):
    """Rows of Consensus.variants() -> (variants [(contig, pos, ndel, alt)] in row order, per row the number of its variant or None).
    'sub' at p: (p, 1, alt); 'del' rows that follow one another in the list at consecutive positions of one contig: one (first
    position, run, ''); 'ins' BEHIND p: (p + 1, 0, alt), left out (None) when it has more than max_alt letters."""
    out, which = [], []
    run = None                                                       # (contig, next position) of the deletion being gathered
    for row in rows:
        name, pos, kind, alt = row[0], int(row[1]), row[2], row[4]
        if kind == 'del' and run == (name, pos):
            out[-1] = (name, out[-1][1], out[-1][2] + 1, '')
            which.append(len(out) - 1)
            run = (name, pos + 1)
            continue
        run = None
        if kind == 'ins' and max_alt is not None and len(alt) > max_alt:
            which.append(None)
            continue
        if kind == 'del':
            out.append((name, pos, 1, ''))
            run = (name, pos + 1)
        elif kind == 'sub':
            out.append((name, pos, 1, alt))
        elif kind == 'ins':
            out.append((name, pos + 1, 0, alt))
        else:
            raise ValueError("genome: unknown kind of variant %r" % (kind,))
        which.append(len(out) - 1)
    return out, which


def _deletion_wins(cn, ref):
    """Whether the winner of a position's counts is the deletion (design/pileup.md 1.4: the greatest of A C G T deletion; a tie to
    the reference letter's class, else to the first in that order)."""
    cand = [int(cn[0]), int(cn[1]), int(cn[2]), int(cn[3]), int(cn[5])]
    best = max(cand)
    r = "ACGT".find(ref)
    return cand[4] == best and not (r >= 0 and cand[r] == best) and cand.index(best) == 4


def pileup(index, res, strand, info, ops, region=None, max_ins=4, keep=None, normalise=True, min_depth=3,
           memory_limit=transducer.WORKSPACE_LIMIT, weighted=False, min_qual=0, qmax=60, weights=None, qual=None):
    """The one-call form: Pileup(index, region, max_ins, ...).add(res, strand, info, ops, keep, normalise) and its consensus.
    -> (Pileup, Consensus).  weighted, min_qual, qmax, weights: as Pileup takes them; qual: as Pileup.add."""
    p = Pileup(index, region=region, max_ins=max_ins, memory_limit=memory_limit, weighted=weighted, min_qual=min_qual, qmax=qmax,
               weights=weights)
    p.add(res, strand, info, ops, keep=keep, normalise=normalise, qual=qual)
    return p, p.consensus(min_depth=min_depth)


# ---- VCF text (design/genotypes.md 1.4) ----------------------------------------------------------------------------------------------

VCF_FORMAT = "GT:GQ:DP:AD:PL"


def vcf_record(contig, pos, ndel, alt):
    """(POS, REF, ALT) of replacing contig[pos:pos + ndel] by alt.  ndel == len(alt) == 1: a SNV at pos + 1; both sides non-empty:
    POS = pos + 1, REF the replaced letters; a pure insertion or deletion takes the base in front (POS = pos), at pos 0 the base
    behind (POS = 1, REF = contig[0:ndel + 1], ALT = alt + contig[ndel])."""
    pos, ndel = int(pos), int(ndel)
    if pos < 0 or ndel < 0 or pos + ndel > len(contig) or ndel + len(alt) < 1:
        raise ValueError("genome: (%d, %d, %r) is no variant of a contig of %d letters" % (pos, ndel, alt, len(contig)))
    if ndel and alt:
        return pos + 1, contig[pos:pos + ndel], alt
    if pos > 0:
        return pos, contig[pos - 1:pos + ndel], contig[pos - 1] + alt
    if ndel >= len(contig):
        raise ValueError("genome: VCF has no anchor for a variant that deletes or fills a whole contig")
    return 1, contig[0:ndel + 1], alt + contig[ndel]


def vcf_text(index, rows, sample='sample', min_gq=20):
    """VCFv4.2 text of called variants.  rows: polish.VariantCall (contig, pos, ndel, alt, gt, gq, dp, ad, pl, qual), as
    polish.VariantCalls.rows() gives them.  The header names every contig of `index` in its order; the records come in contig
    order, then by POS, and as they were given beyond that; FILTER is PASS, or LowGQ below min_gq; one sample column,
    GT:GQ:DP:AD:PL with DP the reads that scored the variant and AD those that do not prefer it and those that do."""
    names = list(index.names)
    host = index.genome.cpu().numpy().tobytes().decode('ascii')
    text = dict((n, host[int(a):int(b)]) for n, a, b in zip(names, index.offsets[:-1], index.offsets[1:]))
    head = ["##fileformat=VCFv4.2", "##source=sloika_amd"]
    head += ["##contig=<ID=%s,length=%d>" % (n, len(text[n])) for n in names]
    head += ['##FILTER=<ID=LowGQ,Description="Genotype quality below %d">' % int(min_gq),
             '##FORMAT=<ID=GT,Number=1,Type=String,Description="Genotype">',
             '##FORMAT=<ID=GQ,Number=1,Type=Integer,Description="Genotype quality">',
             '##FORMAT=<ID=DP,Number=1,Type=Integer,Description="Reads whose signal scored the variant">',
             '##FORMAT=<ID=AD,Number=R,Type=Integer,Description="Reads whose signal prefers the reference, the variant">',
             '##FORMAT=<ID=PL,Number=G,Type=Integer,Description="Phred-scaled genotype likelihoods, not calibrated">',
             "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t%s" % sample]
    recs = []
    for row in rows:
        name = row[0] if not isinstance(row[0], (int, np.integer)) else names[int(row[0])]
        if name not in text:
            raise ValueError("genome: a call names the contig %r, which the index does not hold" % (row[0],))
        pos, ref, alt = vcf_record(text[name], row[1], row[2], row[3])
        gt, gq, dp, ad, pl, qual = row[4:10]
        call = "%s:%d:%d:%d,%d:%d,%d,%d" % ("./." if gt < 0 else ("0/0", "0/1", "1/1")[gt], gq, dp, ad[0], ad[1], pl[0], pl[1], pl[2])
        recs.append((names.index(name), pos, "\t".join([name, str(pos), ".", ref, alt, "%.1f" % qual, "PASS" if gq >= min_gq else "LowGQ",
                                                         ".", VCF_FORMAT, call])))
    recs.sort(key=lambda r: r[:2])                                   # (stable)
    return "\n".join(head + [r[2] for r in recs]) + "\n"
