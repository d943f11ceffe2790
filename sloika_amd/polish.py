"""Signal-level polishing: turn the forward likelihood back on the sequence (design/rescore_edits.md).

Given draft base strings and the posteriors of the reads that cover them, score every single-letter edit of every draft under every
read (decode.rescore_edits_batch: one lattice per read, T x (m + 1) cells per candidate) and apply the edits the signal prefers.

    rescore_drafts(post, drafts, kmer_len, group=None, ...)   -> per group the edit table, the gains and the summed score
    polish(post, drafts, kmer_len, group=None, ...)           -> per group the polished string, the applied edits, rounds and score

On genome coordinates (design/polish_genome.md, design/polish_variants.md):

    rescore_genome(...) / polish_genome(...)                   every single-letter edit of a genome under the reads mapped to it
    rescore_variants(..., variants)                            proposed variants of any length, each ONE hypothesis, per read and strand

A posterior column is a k-mer state with the blank's column skipped: state s sits in column s + (s >= blank), which is s + 1 for this
project's transducers (blank 0) and s for the reference's (blank last).
"""
import collections

import numpy as np

from . import bio, decode

#: per group: `edits` the rows of bio.single_letter_edits, `gain` device float64 [len(edits)], the sum over the group's pairs of
#: ll_edit - score; `score` device float64 scalar, the sum of the pairs' scores of the draft itself; `draft`; `pairs` the group's pairs
Rescored = collections.namedtuple("Rescored", "name draft pairs edits gain score")

#: per group: `sequence` the polished string; `applied` rows (round, kind, letter_pos, letter, gain), positions in the string of that
#: round; `rounds` the rounds that applied something; `score` the summed score of `sequence` (float)
Polished = collections.namedtuple("Polished", "name sequence applied rounds score")


def groups_of(drafts, group):
    """-> [(name, draft, [pairs])] in the order of each group's first pair; without `group` every pair is its own group."""
    names = list(range(len(drafts))) if group is None else list(group)
    if len(names) != len(drafts):
        raise ValueError("group needs one entry per draft (%d for %d)" % (len(names), len(drafts)))
    out = collections.OrderedDict()
    for b, (g, d) in enumerate(zip(names, drafts)):
        d = d.decode('utf-8') if isinstance(d, bytes) else d
        if g not in out:
            out[g] = (d, [])
        elif out[g][0] != d:
            raise ValueError("the pairs of group %r carry different drafts" % (g,))
        out[g][1].append(b)
    return [(g, d, pairs) for g, (d, pairs) in out.items()]


def state_columns(states, blank, nstate):
    """The posterior columns of k-mer states: the blank's column is skipped."""
    blank = blank + nstate if blank < 0 else blank
    states = np.asarray(states, dtype=np.int64)
    return states + (states >= blank)


def draft_edits(draft, kmer_len, kinds, alphabet, blank, nstate):
    """-> (columns of the draft, rows of bio.single_letter_edits, their decode.EditSet on the draft's columns)."""
    old = bio.seq_to_states(draft, kmer_len, alphabet)
    if not len(old):
        raise ValueError("a draft of %d letters has no %d-mer" % (len(draft), kmer_len))
    rows = bio.single_letter_edits(draft, kinds, alphabet)
    rows = [r for r in rows if len(r[3]) >= kmer_len]
    trip = [bio.edit_states(old, bio.seq_to_states(r[3], kmer_len, alphabet)) for r in rows]
    trip = [(a, d, state_columns(n, blank, nstate)) for a, d, n in trip]
    return state_columns(old, blank, nstate), rows, decode.EditSet.from_list(trip)


def rescore_drafts(post, drafts, kmer_len, group=None, kinds=bio.EDIT_KINDS, alphabet='ACGT', blank=-1, band=None, **kwargs):
    """Score every single-letter edit of each group's draft under each of the group's posteriors.

    post and kwargs (lengths, min_prob, row_off, workspace_limit): as decode.rescore_edits_batch.  drafts: one base string per pair;
    group[b] names the draft pair b is a read of (pairs of one group carry the same string; None: every pair is its own group).
    kinds: per group a tuple of kinds when given as a dict {name: kinds}, else the same for all.
    band: None for the dense lattices, or (centers, width) for banded ones (decode.rescore_edits_banded_batch, whole reads): per
    pair the k-mer of its draft each row index 0 .. rows sits at (decode.band_center_from_path / band_center_from_moves); the
    band of `width` states is laid round it by decode.band_lo.  score and gain are then the banded ones.
    -> [Rescored] in the order of each group's first pair."""
    import torch
    shape = tuple(post.shape)
    nstate = shape[-1]
    if nstate != len(alphabet) ** kmer_len + 1:
        raise ValueError("a posterior of %d columns is no transducer over %d-mers of %r" % (nstate, kmer_len, alphabet))
    groups = groups_of(drafts, group)
    seqs, edits = [None] * len(drafts), [None] * len(drafts)
    tables = []
    for name, draft, pairs in groups:
        k = kinds.get(name, ()) if isinstance(kinds, dict) else kinds
        cols, rows, eset = draft_edits(draft, kmer_len, k, alphabet, blank, nstate)
        tables.append(rows)
        for b in pairs:
            seqs[b], edits[b] = cols, eset
    if band is None:
        score, ll = decode.rescore_edits_batch(post, seqs, edits, blank=blank, **kwargs)
    else:
        centers, width = band
        if len(centers) != len(drafts):
            raise ValueError("band needs one centre line per pair (%d for %d)" % (len(centers), len(drafts)))
        los = [decode.band_lo(c, len(q), width) for c, q in zip(centers, seqs)]
        score, ll = decode.rescore_edits_banded_batch(post, seqs, edits, los, width, blank=blank, **kwargs)
    out = []
    for (name, draft, pairs), rows in zip(groups, tables):
        idx = torch.as_tensor(pairs, device=score.device)
        sc = score[idx]
        if rows:
            gain = (torch.stack([ll[b] for b in pairs]) - sc[:, None]).sum(0)
        else:
            gain = torch.zeros(0, dtype=torch.float64, device=score.device)
        out.append(Rescored(name, draft, pairs, rows, gain, sc.sum()))
    return out


def accept_edits(rows, gain, kmer_len, min_gain=0.0):
    """One round's choice: the candidates with gain > min_gain by (-gain, letter_pos, kind, letter), taken greedily when at least
    kmer_len letters from every edit already taken, so that the k-mer windows of the taken edits are disjoint and their gains,
    each computed against the unedited draft, do not interact through a shared state.  A candidate that spells a string an earlier
    candidate of the round has spelled is that edit again (removing any letter of a homopolymer run gives one string, and in a run
    longer than kmer_len two such candidates lie kmer_len apart): it is passed over.  -> [(kind, letter_pos, letter, gain)]"""
    gain = np.asarray(gain, dtype=np.float64)
    rank = dict((k, i) for i, k in enumerate(bio.EDIT_KINDS))
    good = [i for i in range(len(rows)) if gain[i] > min_gain]
    good.sort(key=lambda i: (-gain[i], rows[i][1], rank[rows[i][0]], rows[i][2]))
    taken, seen = [], set()
    for i in good:
        if rows[i][3] in seen:
            continue
        seen.add(rows[i][3])
        if all(abs(rows[i][1] - t[1]) >= kmer_len for t in taken):
            taken.append((rows[i][0], rows[i][1], rows[i][2], float(gain[i])))
    return taken


def shifted_centers(centers, draft, taken, kmer_len, alphabet='ACGT'):
    """The centre lines of a draft's pairs after `taken` (rows of accept_edits) were applied to it: each edit moves the values above
    its first changed k-mer by the k-mers it adds or removes (decode.shift_center).  The rows keep their place: no re-alignment."""
    old = bio.seq_to_states(draft, kmer_len, alphabet)
    trip = []
    for t in taken:
        a, d, new = bio.edit_states(old, bio.seq_to_states(bio.apply_letter_edits(draft, [t[:3]]), kmer_len, alphabet))
        trip.append((a, d, len(new)))
    return [decode.shift_center(c, trip) for c in centers]


def polish(post, drafts, kmer_len, group=None, min_gain=0.0, max_rounds=8, kinds=bio.EDIT_KINDS, alphabet='ACGT', blank=-1, band=None,
           **kwargs):
    """Greedy polishing of draft strings against the posteriors of their reads.  Per round every group still running is rescored
    (rescore_drafts), accept_edits picks its edits, they are applied, and the group stops when none is picked; after max_rounds the
    strings are scored once more without candidates.  post, drafts, group, kinds, blank, band, kwargs: as rescore_drafts; with a
    band the centre lines follow the applied edits from round to round (shifted_centers).
    -> [Polished] in the order of each group's first pair."""
    groups = groups_of(drafts, group)
    names = [g for g, _, _ in groups]
    text = dict((g, d) for g, d, _ in groups)
    member = [None] * len(drafts)
    for g, _, pairs in groups:
        for b in pairs:
            member[b] = g
    running = dict((g, True) for g in names)
    applied = dict((g, []) for g in names)
    rounds = dict((g, 0) for g in names)
    score = {}
    centers = None if band is None else list(band[0])
    for r in range(max_rounds + 1):
        want = dict((g, tuple(kinds) if running[g] and r < max_rounds else ()) for g in names)
        res = rescore_drafts(post, [text[g] for g in member], kmer_len, group=member, kinds=want, alphabet=alphabet, blank=blank,
                             band=None if band is None else (centers, band[1]), **kwargs)
        for x in res:
            score[x.name] = float(x.score.item())
            taken = accept_edits(x.edits, x.gain.cpu().numpy(), kmer_len, min_gain) if want[x.name] else []
            if not taken:
                running[x.name] = False
                continue
            text[x.name] = bio.apply_letter_edits(x.draft, [t[:3] for t in taken])
            if band is not None:
                for b, c in zip(x.pairs, shifted_centers([centers[b] for b in x.pairs], x.draft, taken, kmer_len, alphabet)):
                    centers[b] = c
            applied[x.name].extend((r,) + t for t in taken)
            rounds[x.name] += 1
        if not any(running.values()):
            break
    return [Polished(g, text[g], applied[g], rounds[g], score[g]) for g in names]


# ---- on genome coordinates (csrc/polish_genome.hip, design/polish_genome.md) ----------------------------------------------------------

#: status of a read in rescore_genome (include/sloika_amd.h: SLK_POLISH_*); READ_UNMAPPED and READ_NOT_KEPT are the host's
READ_DONE, READ_SKIPPED, READ_UNMAPPED, READ_NOT_KEPT = 0, 1, 2, 3
READ_REASONS = {
    1: "no columns (an empty alignment, or a traceback that failed)", 2: "unmapped", 3: "left out by keep=",
    -1: "a span of its row lies outside the sequences", -2: "its row has a negative count",
    -3: "the spans of its row are not the sums of its counts", -4: "its slice of the column codes does not have the length of its alignment",
    -5: "its mapping window is not inside the genome", -6: "a column code that is no op", -7: "the columns of a kind are not as many as its row says",
    -8: "its call is empty, holds a state that is no k-mer or spells other letters than were aligned", -9: "a move_row outside its rows, or one that decreases",
    -10: "its aligned window has no k-mer", -11: "its aligned part has fewer rows than the window has k-mers", -12: "no room for its centre line",
}
KIND_BITS = {'sub': 1, 'del': 2, 'ins': 4}


def kinds_mask(kinds):
    unknown = [k for k in kinds if k not in KIND_BITS]
    if unknown:
        raise ValueError("unknown kind of edit %r (known: %s)" % (unknown[0], ', '.join(bio.EDIT_KINDS)))
    return sum(KIND_BITS[k] for k in set(kinds))


def _check_kmer_len(kmer_len):
    if int(kmer_len) != kmer_len or not 3 <= kmer_len <= decode.rescore_max_new() - 1:
        raise ValueError("kmer_len = %r outside 3 .. %d (an edit may bring kmer_len + 1 new symbols)" % (kmer_len, decode.rescore_max_new() - 1))


def _candidate_list(who, genome, win_off, w0, w1, minus, kmer_len, blank, margin, extra, extra_dtype, max_new, count, emit, new):
    """What letter_edits and variant_edits share: the candidates of a batch of windows laid out as the rescoring entries read them.
    count(L, ncand, nkmer, st), emit(L, c, new_off, st), new(L, c, cap, st) call the caller's three entries (pointers but `c`, the
    namespace so far); `extra` names the caller's own column of the list, of `extra_dtype`; a candidate has at most max_new new
    symbols.  One round trip, for the totals."""
    import types
    import torch
    from . import _lib, device as D
    nwin, G = int(win_off.numel()), int(genome.numel())
    if margin < 0 or blank < 0:
        raise ValueError("margin and blank are not negative")
    dev = genome.device
    for name, t, dt in (("win_off", win_off, torch.int64), ("w0", w0, torch.int64), ("w1", w1, torch.int64), ("minus", minus, torch.int32)):
        if t.dtype != dt or t.device != dev or t.numel() != nwin or not t.is_contiguous():
            raise ValueError("%s: %s must be a contiguous %s device tensor with one entry per window" % (who, name, dt))
    L, st = _lib.lib(), D.stream_ptr()
    offs = torch.empty((2, nwin + 1), dtype=torch.int64, device=dev)
    _lib.check(count(L, offs[0].data_ptr(), offs[1].data_ptr(), st), who + "_count")
    offs = torch.cumsum(offs, 1)
    host = offs.cpu().numpy()                                     # the round trip: the totals (and the per-window counts with them)
    ncand, npos = int(host[0, -1]), int(host[1, -1])
    c = types.SimpleNamespace(cand_off=offs[0], pos_off=offs[1], cand_off_host=host[0].copy(), pos_off_host=host[1].copy(), ncand=ncand,
                              npos=npos)
    c.cand_pair = torch.empty(max(ncand, 1), dtype=torch.int32, device=dev)
    c.cand_start, c.cand_ndel = torch.empty_like(c.cand_pair), torch.empty_like(c.cand_pair)
    setattr(c, extra, torch.empty(max(ncand, 1), dtype=extra_dtype, device=dev))
    new_off = torch.zeros(ncand + 1, dtype=torch.int64, device=dev)
    _lib.check(emit(L, c, new_off.data_ptr(), st), who + "_emit")
    c.cand_new_off = torch.cumsum(new_off, 0)
    cap = max(ncand * max_new, 1)                                 # (no second round trip for the exact total)
    c.cand_new = torch.full((cap,), -1, dtype=torch.int32, device=dev)
    _lib.check(new(L, c, cap, st), who + "_new")
    c.seq = torch.empty(max(npos, 1), dtype=torch.int32, device=dev)
    _lib.check(L.slk_polish_window_kmers(genome.data_ptr(), G, win_off.data_ptr(), w0.data_ptr(), w1.data_ptr(), minus.data_ptr(), nwin,
                                         kmer_len, int(blank), c.pos_off.data_ptr(), npos, c.seq.data_ptr(), st), "polish_window_kmers")
    for name in ("cand_pair", "cand_start", "cand_ndel", extra):
        setattr(c, name, getattr(c, name)[:ncand])
    return c


def letter_edits(genome, win_off, w0, w1, minus, kmer_len, blank=0, kinds=bio.EDIT_KINDS, margin=0):
    """Every single-letter edit of a batch of windows of the packed genome, made on the device in the layout the rescoring entries read
    (slk_letter_edits_count / _emit / _new, slk_polish_window_kmers).  genome: uint8 device tensor (Index.genome); win_off, w0, w1:
    int64 device tensors [nwin], the packed position of each window's contig and the window [w0, w1) within it; minus: int32 device
    tensor, non-zero where the window is the reverse complement of its span.  Edits lie `margin` letters from either end.
    -> namespace: cand_off, pos_off (device int64 [nwin + 1]) and their host copies cand_off_host, pos_off_host (the one round trip);
    cand_pair, cand_start, cand_ndel (int32), cand_new_off (int64), cand_new (int32), cand_edit (int64 = 8 * packed forward position
    + slot: 0-2 substitutions in alphabet order without the draft's letter, 3 deletion, 4-7 insertions in front); seq (int32)."""
    import torch
    _check_kmer_len(kmer_len)
    mask, margin, nwin, G = kinds_mask(kinds), int(margin), int(win_off.numel()), int(genome.numel())
    wins = (win_off.data_ptr(), w0.data_ptr(), w1.data_ptr())
    head = (genome.data_ptr(), G) + wins + (minus.data_ptr(), nwin, kmer_len)
    return _candidate_list(
        "letter_edits", genome, win_off, w0, w1, minus, kmer_len, blank, margin, "cand_edit", torch.int64, kmer_len + 1,
        lambda L, ncand, nkmer, st: L.slk_letter_edits_count(*wins, nwin, G, kmer_len, mask, margin, ncand, nkmer, st),
        lambda L, c, new_off, st: L.slk_letter_edits_emit(*head, mask, margin, c.cand_off.data_ptr(), c.ncand, c.cand_pair.data_ptr(),
                                                          c.cand_start.data_ptr(), c.cand_ndel.data_ptr(), new_off, c.cand_edit.data_ptr(), st),
        lambda L, c, cap, st: L.slk_letter_edits_new(*head, int(blank), mask, margin, c.cand_off.data_ptr(), c.ncand, c.cand_start.data_ptr(),
                                                     c.cand_new_off.data_ptr(), cap, c.cand_new.data_ptr(), st))


def sum_gains(score, ll_edit, cand_read, cand_edit, region_start, P, gain=None, support=None):
    """The reads' gains on genome coordinates (slk_polish_sum_gains_f64): per cell (position, slot) of the packed positions
    [region_start, region_start + P) the sum of ll_edit - score[cand_read] over the candidates of that edit, taken one after the
    other in read order (the sort by (edit, read) is torch's, the walk the kernel's), and the number of reads counted.  Only
    candidates whose two values are finite count; a NaN of either makes the cell NaN.  gain, support: tables to go on from (added to
    in place) -- batches that come in read order give the bits of one call.  -> (gain float64 [P, 8], support int32 [P, 8])."""
    import torch
    from . import _lib, device as D
    dev = score.device
    P, ncand = int(P), int(ll_edit.numel())
    if gain is None:
        gain = torch.zeros((max(P, 1), 8), dtype=torch.float64, device=dev)
        support = torch.zeros((max(P, 1), 8), dtype=torch.int32, device=dev)
    if cand_read.numel() != ncand or cand_edit.numel() != ncand or cand_read.dtype != torch.int32 or cand_edit.dtype != torch.int64 or \
            score.dtype != torch.float64 or ll_edit.dtype != torch.float64:
        raise ValueError("sum_gains needs one int32 read, one int64 edit and one float64 value per candidate, and float64 scores")
    if ncand and P:
        by_read = torch.sort(cand_read, stable=True).indices
        order = by_read[torch.sort(cand_edit[by_read], stable=True).indices].contiguous()
        _lib.check(_lib.lib().slk_polish_sum_gains_f64(score.data_ptr(), int(score.numel()), ll_edit.contiguous().data_ptr(),
                                                       cand_read.contiguous().data_ptr(), cand_edit.contiguous().data_ptr(),
                                                       order.data_ptr(), ncand, int(region_start), P, gain.data_ptr(),
                                                       support.data_ptr(), D.stream_ptr()), "polish_sum_gains")
    return gain[:P], support[:P]


def read_windows(paths, lens, move_row, steps, ops, strand, info, index, kmer_len, keep=None):
    """Each mapped read's alignment and its call's moves put together (slk_polish_read_windows; design/polish_genome.md 1): paths, lens,
    move_row as decode.viterbi_marginals_batch / call_reads_qual return them, steps the int32 device tensor of the reads' posterior
    rows, ops / strand / info what Index.map_paths(ops=True) returned for those calls.  keep: bool mask of the reads to use.
    -> namespace of host arrays status int32 [B] (READ_REASONS), span int32 [B, 2] (the posterior rows [r0, r1) of the aligned part),
    window int64 [B, 2] ([w0, w1) in contig coordinates), contig, and the device tensors center (int32) and center_off (int64
    [B + 1]): read b's r1 - r0 + 1 centre values start at center_off[b].  A read that is unmapped, not kept or refused has its
    status and nothing else."""
    import types
    import torch
    from . import _lib, device as D
    _check_kmer_len(kmer_len)
    B = len(ops)
    if paths.shape[0] != B or lens.numel() != B or move_row.shape[0] != B or steps.numel() != B or len(strand) != B:
        raise ValueError("read_windows: %d alignments but %d calls" % (B, paths.shape[0]))
    if len(ops.parts) != 1:
        raise ValueError("read_windows takes the columns of Index.map_paths (one reference buffer)")
    if paths.dtype != torch.int32 or move_row.dtype != torch.int32 or paths.stride(1) != 1 or move_row.stride(1) != 1:
        raise ValueError("read_windows: paths and move_row are int32 device tensors [reads, positions]")
    dev = ops.codes_dev.device
    contig = np.asarray(info['contig'], dtype=np.int64)
    mapped = contig >= 0
    kept = np.ones(B, dtype=bool) if keep is None else np.asarray(keep, dtype=bool)
    if kept.shape != (B,):
        raise ValueError("read_windows: keep= is a mask of %d reads, not of %d" % (kept.size, B))
    ref, roff, rows_d, tb_d = ops.parts[0]
    minus = np.asarray(strand) == '-'
    coff = np.where(mapped, index.offsets[np.where(mapped, contig, 0)], 0).astype(np.int64)
    wstart = np.where(mapped, np.asarray(info['window_start'], dtype=np.int64), 0)
    steps_h = steps.cpu().numpy().astype(np.int64)
    coff_h = np.concatenate([[0], np.cumsum(steps_h + 1)]).astype(np.int64)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    out = types.SimpleNamespace(contig=contig, center_off=up(coff_h), center_off_host=coff_h, steps_host=steps_h)
    out.center = torch.zeros(int(coff_h[-1]), dtype=torch.int32, device=dev)
    st_d = torch.zeros(B, dtype=torch.int32, device=dev)
    span_d = torch.zeros((B, 2), dtype=torch.int32, device=dev)
    win_d = torch.zeros((B, 2), dtype=torch.int64, device=dev)
    lrow = torch.empty((max(B, 1), max(int(ops.ldq), 1)), dtype=torch.int32, device=dev)
    T = min(int(paths.shape[1]), int(move_row.shape[1]))
    if B:
        minus_d, keep_d, ws_d, co_d = up(minus.astype(np.int32)), up((kept & mapped).astype(np.uint8)), up(wstart), up(coff)
        steps_d = steps.to(dev).to(torch.int32).contiguous()
        _lib.check(_lib.lib().slk_polish_read_windows(
            paths.data_ptr(), paths.stride(0), lens.data_ptr(), move_row.data_ptr(), move_row.stride(0), T, steps_d.data_ptr(),
            ops.qlen.data_ptr(), ops.ldq, roff.data_ptr(), rows_d.data_ptr(), ops.codes_dev.data_ptr(), ops.offsets_dev.data_ptr(),
            ops.codes_dev.numel(), tb_d.data_ptr(), minus_d.data_ptr(), keep_d.data_ptr(), ws_d.data_ptr(), co_d.data_ptr(), index.G, B,
            int(kmer_len), out.center_off.data_ptr(), lrow.data_ptr(), st_d.data_ptr(), span_d.data_ptr(), win_d.data_ptr(),
            out.center.data_ptr(), D.stream_ptr()), "polish_read_windows")
    out.status = st_d.cpu().numpy()
    out.status[~mapped] = READ_UNMAPPED
    out.status[mapped & ~kept] = READ_NOT_KEPT
    out.span, out.window, out.minus = span_d.cpu().numpy(), win_d.cpu().numpy(), minus
    out.contig_off = coff
    return out


class GenomeRescored(object):
    """What the signal of the mapped reads says about every single-letter edit of a genome (rescore_genome).

    gain float64, support int32: device tensors [P, 8], the cells of the packed positions lo .. lo + P - 1: slots 0-2 the substitutions
    in alphabet order without the draft's letter, 3 the deletion, 4-7 the insertions of A C G T in FRONT of the position.  gain is
    the sum over the reads that scored the edit of (log-likelihood of the edited window - that of the window), support their number;
    NaN where a read's candidate was refused.  status: host int32 per read, READ_DONE or why it was left out (READ_REASONS); score:
    device float64 per read, its window's banded score (NaN for a read left out); span, window: host arrays per read, the rows
    [r0, r1) it was scored on and its window [w0, w1) in contig coordinates.  cand_read (int32), cand_edit (int64), ll_edit
    (float64): the candidates behind the sums, on the device."""

    def __init__(self, index, lo, P, kmer_len, gain, support, status, score, span, window, cand_read, cand_edit, ll_edit):
        self.index, self.lo, self.P, self.kmer_len, self.gain, self.support = index, int(lo), int(P), int(kmer_len), gain, support
        self.status, self.score, self.span, self.window = status, score, span, window
        self.cand_read, self.cand_edit, self.ll_edit = cand_read, cand_edit, ll_edit
        self._genome = None

    def cell_of(self, contig, pos, kind, letter=''):
        """(row of gain / support, slot) of an edit: kind 'sub' puts `letter` at pos, 'del' removes the letter there, 'ins' puts
        `letter` in front of pos (pos = the contig's length: behind its end).  ValueError outside the region."""
        ix = self.index
        c = ix.names.index(contig) if not isinstance(contig, (int, np.integer)) else int(contig)
        p = int(ix.offsets[c]) + int(pos)
        if not self.lo <= p < self.lo + self.P or pos < 0 or p > int(ix.offsets[c + 1]):
            raise ValueError("position %r of contig %r lies outside the rescored region" % (pos, contig))
        if kind == 'del':
            return p - self.lo, 3
        a = 'ACGT'.index(letter)
        if kind == 'ins':
            return p - self.lo, 4 + a
        if kind != 'sub':
            raise ValueError("unknown kind of edit %r" % (kind,))
        d = 'ACGT'.find(self._letters()[p - self.lo])
        if a == d:
            raise ValueError("a substitution by the letter that stands there is no edit")
        return p - self.lo, a - (1 if d >= 0 and a > d else 0)

    def _letters(self):
        if self._genome is None:
            self._genome = self.index.genome[self.lo:self.lo + self.P].cpu().numpy().tobytes().decode('ascii')
        return self._genome

    def edit_of(self, position, slot):
        """(contig name, position within the contig, kind, letter) of a cell: position a row of gain / support."""
        ix = self.index
        p = self.lo + int(position)
        c = ix.contig_of(p) if p < ix.G else len(ix.names) - 1
        pos = p - int(ix.offsets[c])
        if slot == 3:
            return ix.names[c], pos, 'del', ''
        if slot > 3:
            return ix.names[c], pos, 'ins', 'ACGT'[slot - 4]
        d = 'ACGT'.find(self._letters()[int(position)])
        return ix.names[c], pos, 'sub', [x for i, x in enumerate('ACGT') if i != d][slot]

    def cells(self, min_gain=None, min_support=0):
        """The cells with support >= min_support and, when given, gain > min_gain, chosen on the device and fetched alone:
        -> [(contig, pos, kind, letter, gain, support)] in cell order."""
        import torch
        mask = self.support >= max(int(min_support), 0)
        if min_gain is not None:
            mask = mask & (self.gain > float(min_gain))            # (a NaN cell compares false)
        hit = mask.reshape(-1).nonzero().reshape(-1)
        g, s = self.gain.reshape(-1)[hit].cpu().numpy(), self.support.reshape(-1)[hit].cpu().numpy()
        return [self.edit_of(int(h) // 8, int(h) % 8) + (float(gv), int(sv)) for h, gv, sv in zip(hit.cpu().numpy(), g, s)]

    def edits(self):
        """Every cell a read scored: rows (contig, pos, kind, letter, gain, support)."""
        return self.cells(None, 1)

    def top(self, n=10):
        """The n cells of largest gain among those a read scored."""
        return sorted((r for r in self.edits() if r[4] == r[4]), key=lambda r: (-r[4], r[0], r[1]))[:int(n)]


def _window_tensors(w, reads, dev):
    """(win_off, w0, w1, minus) of the reads `reads` of a read_windows result, as the candidate kernels take them."""
    import torch
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return up(w.contig_off[reads]), up(w.window[reads, 0]), up(w.window[reads, 1]), up(w.minus[reads].astype(np.int32))


def _read_bands(w, reads, npos, width, B, dev):
    """The lattices of the reads `reads` of a read_windows result whose windows have npos k-mers: (nrow int64 host, band_lo int32
    device, row_off int64 host).  The bands: centre - width / 2 clamped to [0, max(0, L + 1 - width)]; the centre does not decrease,
    so neither does the band."""
    import torch
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    nrow = (w.span[reads, 1] - w.span[reads, 0]).astype(np.int64)
    src = up(np.repeat(w.center_off_host[reads] - np.concatenate([[0], np.cumsum(nrow + 1)])[:-1], nrow + 1)) + \
        torch.arange(int((nrow + 1).sum()), device=dev)
    top = up(np.repeat(np.maximum(npos + 1 - int(width), 0), nrow + 1))
    band = torch.minimum(torch.clamp(w.center[src].to(torch.int64) - int(width) // 2, min=0), top).to(torch.int32)
    row_off = reads.astype(np.int64) + w.span[reads, 0].astype(np.int64) * B
    return nrow, band, row_off


def _rescore_windows(who, post, steps, paths, lens, move_row, index, res, strand, info, ops, kmer_len, width, margin, keep, blank,
                     min_prob, workspace_limit, candidates):
    """What rescore_genome and rescore_variants share: the reads' windows (read_windows), the candidates of those that have one --
    candidates(win_off, w0, w1, minus, margin=) -> letter_edits' or variant_edits' namespace --, their bands and the banded entry.
    -> (w the read_windows result, score float64 [B], NaN for a read left out, c, cand_read int32, ll_edit float64); without a read
    to score the candidates of no window and no values."""
    import torch
    _check_kmer_len(kmer_len)
    if post.dim() != 3 or int(post.shape[2]) != 4 ** kmer_len + 1:
        raise ValueError("%s takes a [rows, reads, %d] transducer posterior of %d-mers" % (who, 4 ** kmer_len + 1, kmer_len))
    B = int(post.shape[1])
    if len(ops) != B or len(res) != B:
        raise ValueError("%s: %d reads in the posterior, %d alignments" % (who, B, len(ops)))
    margin = 2 * int(kmer_len) if margin is None else int(margin)
    pd = post if post.is_contiguous() else post.contiguous()
    dev = pd.device
    w = read_windows(paths, lens, move_row, steps, ops, strand, info, index, kmer_len, keep)
    reads = np.flatnonzero(w.status == READ_DONE)
    score = torch.full((B,), float('nan'), dtype=torch.float64, device=dev)
    c = candidates(*_window_tensors(w, reads, dev), margin=margin)
    if not len(reads):
        return w, score, c, torch.zeros(0, dtype=torch.int32, device=dev), torch.zeros(0, dtype=torch.float64, device=dev)
    reads_d = torch.from_numpy(np.ascontiguousarray(reads.astype(np.int64))).to(dev)
    nrow, band, row_off = _read_bands(w, reads, np.diff(c.pos_off_host), width, B, dev)
    sc, ll = decode.rescore_edits_banded_device(pd, row_off, B, nrow.astype(np.int32), c.seq, c.pos_off, band, width, c.cand_off_host,
                                                c.cand_pair, c.cand_start, c.cand_ndel, c.cand_new_off, c.cand_new, blank=blank,
                                                min_prob=min_prob, workspace_limit=workspace_limit)
    score[reads_d] = sc
    return w, score, c, reads_d[c.cand_pair.to(torch.int64)].to(torch.int32), ll


def rescore_genome(post, steps, paths, lens, move_row, index, res, strand, info, ops, kmer_len, width=512, margin=None,
                   kinds=bio.EDIT_KINDS, keep=None, region=None, blank=0, min_prob=None, workspace_limit=None):
    """Score every single-letter edit of a genome under the signal of the reads mapped to it, and sum on genome coordinates.

    post: the reads' posterior [T', B, states] on the device (float32 or float64), steps: int32 device tensor of each read's rows;
    paths, lens, move_row: the reads' calls (decode.viterbi_marginals_batch); index: the genome.Index the calls were mapped to, and
    res, strand, info, ops what index.map_paths(paths, lens, kmer_len, ops=True) returned.  Each read's draft is the window of its
    contig that its alignment covers, on its own strand, its rows those of the aligned part, its band `width` states round the
    centre line taken through the alignment (read_windows); its candidates are made on the device (letter_edits) at least `margin`
    letters (default 2 kmer_len: both ends of a window are pinned by the global recursion, so edits near them are not that read's to
    judge) from the window's ends, scored by the banded entry as it is (decode.rescore_edits_banded_device) and summed in read order
    (sum_gains).  keep: bool mask of the reads to use (info['edge'] == 0 is the usual filter).  region: (contig, start, end) or None
    for the whole genome: the cells to sum; a slice gives the slice of the whole.  A read that is unmapped, fails keep or whose band
    cannot be laid is reported in `status`, never raised.  -> GenomeRescored."""
    from . import genome as G
    lo, P = G.region_span(index, region)
    w, score, c, cand_read, ll = _rescore_windows(
        "rescore_genome", post, steps, paths, lens, move_row, index, res, strand, info, ops, kmer_len, width, margin, keep, blank, min_prob,
        workspace_limit, lambda *wins, margin: letter_edits(index.genome, *wins, kmer_len, blank, kinds, margin))
    gain, support = sum_gains(score, ll, cand_read, c.cand_edit, lo, P)
    return GenomeRescored(index, lo, P, kmer_len, gain, support, w.status, score, w.span, w.window, cand_read, c.cand_edit, ll)


#: per contig: `sequence` the polished string; `applied` rows (round, pos, kind, letter, gain, support), positions in the contig's
#: string of that round; `rounds` the rounds that applied something to it
GenomePolished = collections.namedtuple("GenomePolished", "name sequence applied rounds")


def letter_triple(seq, kind, pos, letter, kmer_len):
    """(start, ndel, new k-mer states) of a single-letter edit of a base string, as bio.edit_states gives it for the spelled-out
    strings, from the letters round the edit alone: two edits that spell the same string have the same triple."""
    return variant_triple(seq, *_as_replacement(kind, pos, letter), kmer_len)


def accept_genome_edits(cells, text, kmer_len):
    """One round's choice among the fetched cells (contig, pos, kind, letter, gain, support): accept_edits' order, (-gain, pos, kind,
    letter), and its spacing, at least kmer_len letters from every edit already taken on the same contig; a cell whose triple
    (letter_triple on the contig's string) an earlier cell of the round had is that edit again and is passed over."""
    return accept_genome_variants(cells, [], text, kmer_len)


def polish_genome(post, steps, paths, lens, move_row, index, kmer_len, width=512, margin=None, kinds=bio.EDIT_KINDS, keep=None,
                  min_gain=0.0, min_support=2, max_rounds=4, blank=0, min_prob=None, workspace_limit=None, map_kwargs=None,
                  proposals=None):
    """Greedy polishing of a genome against the signal of the reads mapped to it.  Per round: the calls are mapped onto the current
    strings (index.map_paths(ops=True, **map_kwargs); the first round on `index` itself), rescore_genome sums the gains, the cells
    with gain > min_gain and support >= min_support are chosen on the device and fetched alone, accept_genome_edits takes them
    greedily, they are applied, and the next round's Index is built from the new strings (same k, bin_width, max_occ).  The
    posterior is computed once by the caller; nothing shifts windows arithmetically.  It stops when a round takes nothing.
    keep: None, a bool mask of the reads, or a function (res, strand, info) -> mask evaluated on every round's mapping.
    -> ([GenomePolished] in the index's contig order, the last round's GenomeRescored).

    proposals: None, or variants of any length to put to the signal beside the single-letter cells (design/polish_variants.md):
    'repeats' (repeat_variants of every round's index), a list of (contig, pos, ndel, alt) or a VariantSet on `index` (put in the
    first round, whose coordinates they are), or a function index -> variants evaluated on every round's index.  Each round then also runs
    rescore_variants on the same mapping and accept_genome_variants chooses over cells and variants together; `kinds=()` leaves the
    variants alone.  Applied variants are rows (round, pos, 'var', (ndel, alt), gain, support).
    -> ([GenomePolished], the last round's GenomeRescored or None without kinds, the last round's GenomeVariantsRescored)."""
    from . import genome as G
    kw = dict(map_kwargs or {})
    host = index.genome.cpu().numpy().tobytes().decode('ascii')
    text = collections.OrderedDict((n, host[int(a):int(b)]) for n, a, b in zip(index.names, index.offsets[:-1], index.offsets[1:]))
    applied = dict((n, []) for n in text)
    rounds = dict((n, 0) for n in text)
    ix, last, lastv = index, None, None
    for r in range(int(max_rounds)):
        got = ix.map_paths(paths, lens, kmer_len, ops=True, **kw)
        res, strand, info, ops = got[0], got[1], got[2], got[4]
        mask = keep(res, strand, info) if callable(keep) else keep
        common = dict(width=width, margin=margin, keep=mask, blank=blank, min_prob=min_prob, workspace_limit=workspace_limit)
        cells, rows = [], []
        if proposals is None or len(kinds):
            last = rescore_genome(post, steps, paths, lens, move_row, ix, res, strand, info, ops, kmer_len, kinds=kinds, **common)
            cells = last.cells(min_gain, min_support)
        if proposals is not None:
            asked = proposals(ix) if callable(proposals) else proposals if isinstance(proposals, str) or r == 0 else []
            lastv = rescore_variants(post, steps, paths, lens, move_row, ix, res, strand, info, ops, kmer_len, asked, **common)
            rows = lastv.rows(min_gain, min_support)
        taken = accept_genome_variants(cells, rows, text, kmer_len)
        if not taken:
            break
        for name in text:
            mine = [t for t in taken if t[0] == name]
            if mine:
                s = text[name]
                for t in sorted(mine, key=lambda t: t[1], reverse=True):    # (from the back: the positions in front stay)
                    pos, ndel, alt = (t[1],) + tuple(t[3]) if t[2] == 'var' else _as_replacement(t[2], t[1], t[3])
                    s = s[:pos] + alt + s[pos + ndel:]
                text[name] = s
                if proposals is not None:                          # (rows by position there, in the order taken here: as ever)
                    mine.sort(key=lambda t: t[1])
                applied[name].extend((r, t[1], t[2], t[3], t[4], t[5]) for t in mine)
                rounds[name] += 1
        ix = G.Index(list(text.items()), k=index.k, bin_width=index.bin_width, max_occ=index.max_occ)
    out = [GenomePolished(n, text[n], applied[n], rounds[n]) for n in text]
    return (out, last) if proposals is None else (out, last, lastv)


# ---- proposed variants of any length (csrc/polish_variants.hip, design/polish_variants.md) --------------------------------------------

#: var_status of a variant (include/sloika_amd.h: SLK_VARIANT_*)
VARIANT_REASONS = {
    -1: "its contig is none of the index's", -2: "its span is not inside its contig", -3: "a negative number of deleted letters",
    -4: "its alt has more letters than an edit may bring, or its slice of the letters is not one", -5: "it deletes nothing and puts nothing in",
    -6: "its alt is the letters that stand there",
}


def max_alt(kmer_len):
    """The most letters a variant's alt may have: its edit then has at most SLK_RESCORE_MAX_NEW new symbols."""
    return decode.rescore_max_new() - int(kmer_len) + 1


def variant_triple(seq, pos, ndel, alt, kmer_len):
    """(start, ndel, new k-mer states) of replacing seq[pos:pos + ndel] by alt, as bio.edit_states gives it for the spelled-out strings,
    from the letters alone (design/polish_variants.md 1.3): two variants that spell the same string have the same triple.  For a
    single-letter edit it is letter_triple."""
    pos, ndel, k = int(pos), int(ndel), int(kmer_len)
    text = seq[:pos] + alt + seq[pos + ndel:]
    n, n2 = len(seq), len(text)
    m = min(n, n2)
    front = next((i for i in range(pos, m) if seq[i] != text[i]), None)
    back = next((n - 1 - t for t in range(n - pos - ndel, m) if seq[n - 1 - t] != text[n2 - 1 - t]), None)
    nold, nnew = n - k + 1, n2 - k + 1
    nmin = min(nold, nnew)
    pre = nmin if front is None else min(max(front - k + 1, 0), nmin)
    rest = nmin - pre
    suf = rest if back is None else min(max(nold - 1 - back, 0), rest)
    new = bio.seq_to_states(text[pre:nnew - suf + k - 1], k) if nnew - suf > pre else np.zeros(0, dtype=np.int64)
    return pre, nold - pre - suf, tuple(int(v) for v in new)


class VariantSet(object):
    """Variants on the device in the layout the kernels read, sorted by (contig, pos): var_off, var_pos (int64), var_ndel (int32),
    var_alt_off (int64 [V + 1]), var_alt (uint8), contig_off (int64, the index's offsets).  order: host int64 [V], order[s] the
    caller's number of sorted entry s (order_dev the same on the device); every result of the functions that take the set is in the
    caller's order."""

    def __init__(self, index, var_off, var_pos, var_ndel, var_alt_off, var_alt, contig_off, order=None):
        import torch
        self.index, self.V, self.A = index, int(var_off.numel()), int(var_alt.numel())
        self.var_off, self.var_pos, self.var_ndel, self.var_alt_off, self.var_alt = var_off, var_pos, var_ndel, var_alt_off, var_alt
        self.contig_off = contig_off
        self.order = np.arange(self.V, dtype=np.int64) if order is None else np.asarray(order, dtype=np.int64)
        self.order_dev = torch.from_numpy(self.order).to(var_off.device)
        self._rows = None

    def __len__(self):
        return self.V

    def rows(self):
        """[(contig name, pos, ndel, alt)] in the caller's order (one fetch, kept)."""
        if self._rows is None:
            ix = self.index
            off, pos, nd = self.var_off.cpu().numpy(), self.var_pos.cpu().numpy(), self.var_ndel.cpu().numpy()
            ao, al = self.var_alt_off.cpu().numpy(), self.var_alt.cpu().numpy().tobytes().decode('ascii')
            starts = dict((int(o), n) for n, o in zip(ix.names, ix.offsets[:-1]))
            out = [None] * self.V
            for s in range(self.V):
                out[int(self.order[s])] = (starts.get(int(off[s])), int(pos[s]), int(nd[s]), al[int(ao[s]):int(ao[s + 1])])
            self._rows = out
        return list(self._rows)


def _contig_offsets(index, dev):
    import torch
    have = getattr(index, 'offsets_dev', None)
    return have if have is not None else torch.from_numpy(np.ascontiguousarray(index.offsets, dtype=np.int64)).to(dev)


def upload_variants(index, variants, kmer_len=None):
    """Rows (contig name or number, pos, ndel, alt) checked on the host, sorted by (contig, pos) stably and put on the device.
    ValueError naming the row for: an unknown contig, a span outside it, a negative ndel, an alt with a letter that is none of ACGT or
    with more than max_alt(kmer_len) letters (kmer_len None: of the shortest k-mers, 3), an empty edit, an alt that is the letters
    that stand there.  -> VariantSet."""
    import torch
    rows = list(variants)
    cap = max_alt(3 if kmer_len is None else kmer_len)
    host = None
    key, nd_h, alts = [], [], []
    for i, row in enumerate(rows):
        bad = lambda why: ValueError("variant %d %r: %s" % (i, tuple(row), why))               # noqa: E731
        if len(row) != 4:
            raise bad("a variant is (contig, pos, ndel, alt)")
        c, pos, ndel, alt = row
        if not isinstance(c, (int, np.integer)):
            if c not in index.names:
                raise bad(VARIANT_REASONS[-1])
            c = index.names.index(c)
        if not 0 <= c < len(index.names):
            raise bad(VARIANT_REASONS[-1])
        if int(ndel) < 0:
            raise bad(VARIANT_REASONS[-3])
        if int(pos) < 0 or int(pos) + int(ndel) > int(index.lengths[c]):
            raise bad(VARIANT_REASONS[-2])
        if any(ch not in 'ACGT' for ch in alt):
            raise bad("its alt has a letter that is none of A C G T")
        if len(alt) > cap:
            raise bad(VARIANT_REASONS[-4])
        if int(ndel) + len(alt) < 1:
            raise bad(VARIANT_REASONS[-5])
        if int(ndel) == len(alt):
            if host is None:
                host = index.genome.cpu().numpy().tobytes().decode('ascii')
            p = int(index.offsets[c]) + int(pos)
            if host[p:p + int(ndel)] == alt:
                raise bad(VARIANT_REASONS[-6])
        key.append((int(index.offsets[c]), int(pos)))
        nd_h.append(int(ndel))
        alts.append(alt)
    order = np.array(sorted(range(len(rows)), key=lambda i: key[i]), dtype=np.int64)           # (sorted is stable)
    dev = index.genome.device
    up = lambda a, dt: torch.from_numpy(np.array(a, dtype=dt)).to(dev)                         # noqa: E731
    text = ''.join(alts[i] for i in order)
    return VariantSet(index, up([key[i][0] for i in order], np.int64), up([key[i][1] for i in order], np.int64),
                      up([nd_h[i] for i in order], np.int32), up(np.concatenate([[0], np.cumsum([len(alts[i]) for i in order])]), np.int64),
                      up(np.frombuffer(text.encode('ascii'), dtype=np.uint8), np.uint8), _contig_offsets(index, dev), order)


def repeat_variants(index, kmer_len, region=None, max_unit=4, max_change=2, min_copies=2):
    """The repeat-unit family proposed on the device (slk_repeat_variants_count / _emit; design/polish_variants.md 1.5): for every
    leftmost tract of a primitive unit of 1 .. max_unit letters with at least min_copies copies that starts inside `region`, the
    deletions of 1 .. max_change copies (one copy stays) and the insertions of as many (up to max_alt(kmer_len) letters), but the
    single-letter ones.  One round trip for the totals.  -> VariantSet, sorted as it comes."""
    import torch
    from . import _lib, device as D, genome as G
    _check_kmer_len(kmer_len)
    if not 1 <= int(max_unit) <= 4 or not 1 <= int(max_change) <= 8 or int(min_copies) < 2:
        raise ValueError("repeat_variants: max_unit 1 .. 4, max_change 1 .. 8, min_copies >= 2")
    lo, P = G.region_span(index, region)
    dev = index.genome.device
    coff = _contig_offsets(index, dev)
    L, st = _lib.lib(), D.stream_ptr()
    head = (index.genome.data_ptr(), int(index.G), coff.data_ptr(), len(index.names), int(lo), int(P), int(kmer_len), int(max_unit),
            int(max_change), int(min_copies))
    offs = torch.zeros((2, P + 1), dtype=torch.int64, device=dev)
    _lib.check(L.slk_repeat_variants_count(*head, offs[0].data_ptr(), offs[1].data_ptr(), st), "repeat_variants_count")
    offs = torch.cumsum(offs, 1)
    V, A = (int(v) for v in offs[:, -1].cpu().numpy())
    var_off = torch.zeros(V, dtype=torch.int64, device=dev)
    var_pos, var_ndel = torch.zeros_like(var_off), torch.zeros(V, dtype=torch.int32, device=dev)
    var_alt_off, var_alt = torch.zeros(V + 1, dtype=torch.int64, device=dev), torch.zeros(A, dtype=torch.uint8, device=dev)
    _lib.check(L.slk_repeat_variants_emit(*head, offs[0].data_ptr(), offs[1].data_ptr(), V, A, var_off.data_ptr(), var_pos.data_ptr(),
                                          var_ndel.data_ptr(), var_alt_off.data_ptr(), var_alt.data_ptr(), st), "repeat_variants_emit")
    return VariantSet(index, var_off, var_pos, var_ndel, var_alt_off, var_alt, coff)


def variant_edits(genome, contig_offsets, win_off, w0, w1, minus, variants_on_device, kmer_len, blank=0, margin=0):
    """The candidates a batch of windows of the packed genome has among a variant set, made on the device in the layout the rescoring
    entries read (slk_variant_edits_count / _emit / _new, slk_polish_window_kmers).  genome, win_off, w0, w1, minus: as letter_edits
    takes them; contig_offsets: int64 device tensor, the contigs' packed starts and the genome's length; variants_on_device: a
    VariantSet.  A window's candidates are the variants of its contig that lie `margin` letters inside it.
    -> the namespace letter_edits returns with cand_var (int32, the variant in the caller's order) in place of cand_edit, and
    var_status (int32 device [V], caller's order: 0 or a key of VARIANT_REASONS)."""
    import torch
    _check_kmer_len(kmer_len)
    vs, margin, nwin, G = variants_on_device, int(margin), int(win_off.numel()), int(genome.numel())
    dev = genome.device
    if contig_offsets.dtype != torch.int64 or contig_offsets.device != dev or contig_offsets.numel() < 2 or not contig_offsets.is_contiguous():
        raise ValueError("variant_edits: contig_offsets must be a contiguous int64 device tensor of the contigs' starts and the genome's length")
    lst = (vs.var_off.data_ptr(), vs.var_pos.data_ptr(), vs.var_ndel.data_ptr(), vs.var_alt_off.data_ptr(), vs.var_alt.data_ptr(), vs.V, vs.A)
    wins = (win_off.data_ptr(), w0.data_ptr(), w1.data_ptr())
    status = torch.zeros(max(vs.V, 1), dtype=torch.int32, device=dev)
    head = (genome.data_ptr(), G) + lst + (status.data_ptr(),) + wins + (minus.data_ptr(), nwin, kmer_len)
    c = _candidate_list(
        "variant_edits", genome, win_off, w0, w1, minus, kmer_len, blank, margin, "cand_var_sorted", torch.int32, decode.rescore_max_new(),
        lambda L, ncand, nkmer, st: L.slk_variant_edits_count(genome.data_ptr(), G, contig_offsets.data_ptr(), int(contig_offsets.numel()) - 1,
                                                              *lst, *wins, nwin, kmer_len, margin, status.data_ptr(), ncand, nkmer, st),
        lambda L, c, new_off, st: L.slk_variant_edits_emit(*head, margin, c.cand_off.data_ptr(), c.ncand, c.cand_pair.data_ptr(),
                                                           c.cand_start.data_ptr(), c.cand_ndel.data_ptr(), c.cand_var_sorted.data_ptr(),
                                                           new_off, st),
        lambda L, c, cap, st: L.slk_variant_edits_new(*head, int(blank), margin, c.ncand, c.cand_pair.data_ptr(), c.cand_start.data_ptr(),
                                                      c.cand_var_sorted.data_ptr(), c.cand_new_off.data_ptr(), cap, c.cand_new.data_ptr(), st))
    c.cand_var = vs.order_dev[c.cand_var_sorted.to(torch.int64)].to(torch.int32) if c.ncand else c.cand_var_sorted
    c.var_status = torch.zeros(vs.V, dtype=torch.int32, device=dev)
    if vs.V:
        c.var_status[vs.order_dev] = status[:vs.V]
    return c


VARIANT_TABLES = ("gain", "support", "pro", "gain_strand", "support_strand", "pro_strand")


def sum_variant_gains(score, ll_edit, cand_read, cand_var, read_minus, V, tables=None):
    """The reads' gains per variant and strand (slk_polish_sum_variant_gains_f64): per variant the sum of ll_edit - score[cand_read] over
    its candidates, taken one after the other in read order (the sort by (variant, read) is torch's, the walk the kernel's), the
    number of reads counted and how many of them gained; the same over the '+' reads and the '-' reads alone (read_minus: int32
    device tensor per read).  Only candidates whose two values are finite count; a NaN of either makes the cells NaN.  tables: the six
    tables of an earlier call to go on from (added to in place) -- batches that come in read order give the bits of one call.
    -> (gain float64 [V], support int32 [V], pro int32 [V], gain_strand float64 [V, 2], support_strand, pro_strand int32 [V, 2])."""
    import torch
    from . import _lib, device as D
    dev = score.device
    V, ncand = int(V), int(ll_edit.numel())
    if tables is None:
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)                          # noqa: E731
        tables = (z(V, torch.float64), z(V, torch.int32), z(V, torch.int32), z((V, 2), torch.float64), z((V, 2), torch.int32),
                  z((V, 2), torch.int32))
    if cand_read.numel() != ncand or cand_var.numel() != ncand or cand_read.dtype != torch.int32 or cand_var.dtype != torch.int32 or \
            score.dtype != torch.float64 or ll_edit.dtype != torch.float64 or read_minus.dtype != torch.int32 or \
            read_minus.numel() != score.numel():
        raise ValueError("sum_variant_gains needs one int32 read, one int32 variant and one float64 value per candidate, and a float64 "
                         "score and an int32 strand per read")
    for t, dt in zip(tables, (torch.float64, torch.int32, torch.int32, torch.float64, torch.int32, torch.int32)):
        if t.dtype != dt or t.shape[0] != V or not t.is_contiguous():
            raise ValueError("sum_variant_gains: tables= are the six tables of an earlier call on the same variants")
    if ncand and V:
        by_read = torch.sort(cand_read, stable=True).indices
        order = by_read[torch.sort(cand_var[by_read], stable=True).indices].contiguous()
        _lib.check(_lib.lib().slk_polish_sum_variant_gains_f64(
            score.data_ptr(), read_minus.contiguous().data_ptr(), int(score.numel()), ll_edit.contiguous().data_ptr(),
            cand_read.contiguous().data_ptr(), cand_var.contiguous().data_ptr(), order.data_ptr(), ncand, V,
            *[t.data_ptr() for t in tables], D.stream_ptr()), "polish_sum_variant_gains")
    return tuple(tables)


class GenomeVariantsRescored(object):
    """What the signal of the mapped reads says about proposed variants of a genome (rescore_variants).

    variants: the VariantSet; every table is in the caller's order.  gain float64, support, pro int32: device tensors [V]: the sum
    over the reads that scored the variant of (log-likelihood of the edited window - that of the window), their number, and how
    many of them prefer the variant; gain_strand, support_strand, pro_strand [V, 2]: the same over the '+' (0) and the '-' (1)
    reads alone.  NaN where a read's candidate was refused.  var_status: device int32 [V] (VARIANT_REASONS).  status, score, span,
    window: per read, as GenomeRescored.  cand_read, cand_var (int32), ll_edit (float64): the candidates behind the sums."""

    def __init__(self, variants, kmer_len, tables, var_status, status, score, span, window, cand_read, cand_var, ll_edit):
        self.variants, self.index, self.kmer_len = variants, variants.index, int(kmer_len)
        self.gain, self.support, self.pro, self.gain_strand, self.support_strand, self.pro_strand = tables
        self.var_status, self.status, self.score, self.span, self.window = var_status, status, score, span, window
        self.cand_read, self.cand_var, self.ll_edit = cand_read, cand_var, ll_edit

    def rows(self, min_gain=None, min_support=0):
        """The variants with support >= min_support and, when given, gain > min_gain, chosen on the device:
        -> [(contig, pos, ndel, alt, gain, support, pro)] in the caller's order."""
        mask = self.support >= max(int(min_support), 0)
        if min_gain is not None:
            mask = mask & (self.gain > float(min_gain))            # (a NaN cell compares false)
        hit = mask.nonzero().reshape(-1)
        g, s, p = self.gain[hit].cpu().numpy(), self.support[hit].cpu().numpy(), self.pro[hit].cpu().numpy()
        rows = self.variants.rows()
        return [rows[int(h)] + (float(gv), int(sv), int(pv)) for h, gv, sv, pv in zip(hit.cpu().numpy(), g, s, p)]

    def top(self, n=10):
        """The n variants of largest gain among those a read scored."""
        return sorted((r for r in self.rows(None, 1) if r[4] == r[4]), key=lambda r: (-r[4], r[0], r[1]))[:int(n)]

    def read_gains(self, v):
        """(reads int array, gains float64 array): the per-read log-likelihood ratios of variant v (caller's number), in read order."""
        hit = (self.cand_var == int(v)).nonzero().reshape(-1)
        reads = self.cand_read[hit].to(self.score.device)
        gains = self.ll_edit[hit] - self.score[reads.to(hit.dtype)]
        order = np.argsort(reads.cpu().numpy(), kind='stable')
        return reads.cpu().numpy()[order], gains.cpu().numpy()[order]


def _as_variant_set(index, variants, kmer_len):
    if isinstance(variants, VariantSet):
        if variants.index is not index:
            raise ValueError("rescore_variants: the variant set was made for another index")
        return variants
    if isinstance(variants, str):
        if variants != 'repeats':
            raise ValueError("unknown family of variants %r (known: 'repeats')" % (variants,))
        return repeat_variants(index, kmer_len)
    return upload_variants(index, variants, kmer_len)


def rescore_variants(post, steps, paths, lens, move_row, index, res, strand, info, ops, kmer_len, variants, width=512, margin=None,
                     keep=None, blank=0, min_prob=None, workspace_limit=None):
    """Put proposed variants of any length to the signal of the reads mapped to a genome (design/polish_variants.md).

    Everything but `variants` as rescore_genome takes it, and the reads' windows, rows, centre lines and bands are rescore_genome's.
    variants: a list of (contig, pos, ndel, alt) -- replace the ndel letters from pos on by alt; ndel 0 an insertion in front of pos
    --, a VariantSet (upload_variants, repeat_variants) or 'repeats'.  A read scores the variants of its contig that lie `margin`
    letters inside its window (variant_edits), each as ONE candidate of the banded entry as it is
    (decode.rescore_edits_banded_device), and the answers are summed per variant and strand in read order (sum_variant_gains).
    A variant the device refuses raises ValueError.  -> GenomeVariantsRescored."""
    import torch
    _check_kmer_len(kmer_len)
    vs = _as_variant_set(index, variants, kmer_len)
    w, score, c, cand_read, ll = _rescore_windows(
        "rescore_variants", post, steps, paths, lens, move_row, index, res, strand, info, ops, kmer_len, width, margin, keep, blank,
        min_prob, workspace_limit, lambda *wins, margin: variant_edits(index.genome, vs.contig_off, *wins, vs, kmer_len, blank, margin))
    minus_d = torch.from_numpy(np.ascontiguousarray(w.minus.astype(np.int32))).to(score.device)
    bad = c.var_status.nonzero().reshape(-1)
    if bad.numel():
        v = int(bad[0])
        raise ValueError("variant %d %r: %s" % (v, vs.rows()[v], VARIANT_REASONS.get(int(c.var_status[v]), "refused")))
    tables = sum_variant_gains(score, ll, cand_read, c.cand_var, minus_d, vs.V)
    return GenomeVariantsRescored(vs, kmer_len, tables, c.var_status, w.status, score, w.span, w.window, cand_read, c.cand_var, ll)


def _as_replacement(kind, pos, letter):
    """(pos, ndel, alt) of a single-letter cell."""
    return (pos, 1, letter) if kind == 'sub' else (pos, 1, '') if kind == 'del' else (pos, 0, letter)


def accept_genome_variants(cells, variants, text, kmer_len):
    """One round's choice among the fetched cells (contig, pos, kind, letter, gain, support) and variants (contig, pos, ndel, alt, gain,
    support, ...) together: by (-gain, contig, pos, kind -- cells before variants --, letter); an edit spans its first to its last
    touched letter (an insertion touches pos alone) and is taken when at least kmer_len letters lie between it and every edit already
    taken on its contig -- for two cells accept_genome_edits' spacing --; an edit whose variant_triple on the contig's string an
    earlier one of the round had is that edit again and is passed over.
    -> rows (contig, pos, kind, letter, gain, support), a variant with kind 'var' and (ndel, alt) for its letter."""
    rank = dict((k, i) for i, k in enumerate(bio.EDIT_KINDS))
    items = [(-r[4], r[0], r[1], rank[r[2]], r[3], _as_replacement(r[2], r[1], r[3]), tuple(r[:6])) for r in cells]
    items += [(-r[4], r[0], r[1], len(rank), (r[2], r[3]), (r[1], r[2], r[3]), (r[0], r[1], 'var', (r[2], r[3]), r[4], r[5])) for r in variants]
    taken, spans, seen = [], [], set()
    for it in sorted(items, key=lambda it: it[:5]):
        pos, ndel, alt = it[5]
        key = (it[1],) + variant_triple(text[it[1]], pos, ndel, alt, kmer_len)
        if key in seen:
            continue
        seen.add(key)
        first, last = pos, pos + max(ndel, 1) - 1
        if all(c != it[1] or first - b >= kmer_len or a - last >= kmer_len for c, a, b in spans):
            taken.append(it[6])
            spans.append((it[1], first, last))
    return taken


# ---- genotypes of proposed variants (csrc/genotype.hip, design/genotypes.md) -----------------------------------------------------------

GENOTYPES = ("0/0", "0/1", "1/1")
GQ_CAP, PL_CAP, QUAL_CAP = 99, 999, 999.0

#: one called variant: the variant, gt -1 (./.) or an index of GENOTYPES, gq, dp (the reads that scored it), ad (reads that do not
#: prefer it, reads that do), pl (three values) and qual
VariantCall = collections.namedtuple("VariantCall", "contig pos ndel alt gt gq dp ad pl qual")


def variant_genotype_likelihoods(score, ll_edit, cand_read, cand_var, V, scale=1.0):
    """The genotype log-likelihoods of V variants from their candidates (slk_variant_genotypes_f64; design/genotypes.md 1.2): score
    float64 per read, ll_edit float64, cand_read and cand_var int32 per candidate, as sum_variant_gains takes them, sorted the same
    way.  Per variant, over its candidates in read order with both values finite, d = scale * (ll_edit - score[read]):
    gl = (0, sum of log(1/2 + 1/2 e^d), sum of d), the log-likelihoods of 0/0, 0/1 and 1/1 against 0/0, and n their number.  A NaN
    of either value makes the three NaN.  -> (gl float64 [V, 3], n int32 [V]) on the device."""
    import torch
    from . import _lib, device as D
    dev = score.device
    V, ncand, scale = int(V), int(ll_edit.numel()), float(scale)
    if not scale > 0.0 or scale in (float('inf'),):
        raise ValueError("genotype likelihoods: scale = %r is no positive finite number" % (scale,))
    if cand_read.numel() != ncand or cand_var.numel() != ncand or cand_read.dtype != torch.int32 or cand_var.dtype != torch.int32 or \
            score.dtype != torch.float64 or ll_edit.dtype != torch.float64:
        raise ValueError("genotype likelihoods need one int32 read, one int32 variant and one float64 value per candidate, and a "
                         "float64 score per read")
    gl = torch.zeros((V, 3), dtype=torch.float64, device=dev)
    n = torch.zeros(V, dtype=torch.int32, device=dev)
    if ncand and V:
        by_read = torch.sort(cand_read, stable=True).indices
        order = by_read[torch.sort(cand_var[by_read], stable=True).indices].contiguous()
        _lib.check(_lib.lib().slk_variant_genotypes_f64(
            score.contiguous().data_ptr(), int(score.numel()), ll_edit.contiguous().data_ptr(), cand_read.contiguous().data_ptr(),
            cand_var.contiguous().data_ptr(), order.data_ptr(), ncand, V, scale, gl.data_ptr(), n.data_ptr(), D.stream_ptr()),
            "variant_genotypes")
    return gl, n


def genotype_likelihoods(rescored, scale=1.0):
    """variant_genotype_likelihoods of a GenomeVariantsRescored: -> (gl [V, 3], n [V]) on the device, in the caller's order.  At scale
    1.0 gl[:, 2] has the bits of rescored.gain and n is rescored.support."""
    return variant_genotype_likelihoods(rescored.score, rescored.ll_edit, rescored.cand_read, rescored.cand_var, len(rescored.variants),
                                        scale)


def genotype_prior(het=1e-3, prior=None):
    """(p00, p01, p11): `prior` itself, or (1 - 1.5 het, het, het / 2)."""
    p = (1.0 - 1.5 * float(het), float(het), float(het) / 2.0) if prior is None else tuple(float(v) for v in prior)
    if len(p) != 3 or not all(0.0 < v <= 1.0 for v in p):
        raise ValueError("genotypes: the prior %r is not three probabilities above 0" % (p,))
    return p


def call_genotypes(gl, n, het=1e-3, prior=None):
    """The host half of `genotypes` (design/genotypes.md 1.3), numpy float64: gl [V, 3] and n [V] -> (gt int [V], gq int [V], pl int
    [V, 3], qual float [V]).  The log-posteriors are gl + log prior, normalised by a max-shifted log-sum-exp; gt their arg-max (ties
    to the lower index), -1 where n == 0 or gl is NaN; gq = min(99, floor(10 / ln 10 x (best - second))); pl = round(-10 / ln 10 x
    (gl - max gl)) capped at 999, from the likelihoods; qual = min(999, -10 log10 P(0/0 | reads)) to one decimal.  An uncalled
    variant has zeros."""
    gl = np.asarray(gl, dtype=np.float64).reshape(-1, 3)
    n = np.asarray(n).reshape(-1)
    V = gl.shape[0]
    if n.shape[0] != V:
        raise ValueError("genotypes: %d rows of likelihoods for %d counts" % (V, n.shape[0]))
    called = (n > 0) & ~np.isnan(gl).any(axis=1)
    g = np.where(called[:, None], gl, 0.0)
    post = g + np.log(np.array(genotype_prior(het, prior), dtype=np.float64))[None, :]
    mx = post.max(axis=1, keepdims=True)
    post = post - (mx + np.log(np.exp(post - mx).sum(axis=1, keepdims=True)))
    gt = np.argmax(post, axis=1)                                     # (the first of equal values)
    ranked = np.sort(post, axis=1)
    k = 10.0 / np.log(10.0)
    gq = np.minimum(np.floor(k * (ranked[:, 2] - ranked[:, 1])), GQ_CAP).astype(np.int64)
    pl = np.minimum(np.rint(-k * (g - g.max(axis=1, keepdims=True))), PL_CAP).astype(np.int64)
    qual = np.round(np.minimum(-k * post[:, 0], QUAL_CAP), 1) + 0.0  # (+ 0.0: no negative zero)
    gt = np.where(called, gt, -1).astype(np.int64)
    gq[~called] = 0
    pl[~called] = 0
    qual[~called] = 0.0
    return gt, gq, pl, qual


class VariantCalls(object):
    """The genotypes of proposed variants (genotypes; design/genotypes.md).  Every array is in the caller's order of the variants.

    gl float64 [V, 3], n int32 [V]: device tensors (genotype_likelihoods); gt, gq, pl, qual: host arrays (call_genotypes); support, pro,
    support_strand, pro_strand: host copies of the rescoring's tables; rescored: the GenomeVariantsRescored behind them; variants:
    its VariantSet.  Each variant is judged against the reference alone (biallelic): overlapping alleles are separate records.
    The likelihood ratios are the network's own and are not calibrated (design/genotypes.md 1.3): `scale` is the knob."""

    def __init__(self, rescored, gl, n, gt, gq, pl, qual, prior, scale):
        self.rescored, self.variants, self.index = rescored, rescored.variants, rescored.variants.index
        self.gl, self.n, self.gt, self.gq, self.pl, self.qual, self.prior, self.scale = gl, n, gt, gq, pl, qual, prior, scale
        self.support, self.pro = rescored.support.cpu().numpy(), rescored.pro.cpu().numpy()
        self.support_strand, self.pro_strand = rescored.support_strand.cpu().numpy(), rescored.pro_strand.cpu().numpy()
        self._n = n.cpu().numpy()

    def __len__(self):
        return len(self.variants)

    def rows(self, min_gq=0, nonref=True):
        """[VariantCall] of the variants with gq >= min_gq, in the caller's order; nonref: only those called 0/1 or 1/1."""
        rows = self.variants.rows()
        return [VariantCall(*rows[v], gt=int(self.gt[v]), gq=int(self.gq[v]), dp=int(self._n[v]),
                            ad=(int(self._n[v]) - int(self.pro[v]), int(self.pro[v])), pl=tuple(int(x) for x in self.pl[v]),
                            qual=float(self.qual[v]))
                for v in range(len(rows)) if self.gq[v] >= min_gq and (self.gt[v] > 0 or not nonref)]

    def vcf(self, sample='sample', min_gq=20, all_records=False):
        """VCFv4.2 text (genome.vcf_text): the non-reference calls, LowGQ below min_gq; all_records: 0/0 and ./. as well."""
        from . import genome as G
        return G.vcf_text(self.index, self.rows(0, nonref=not all_records), sample, min_gq=min_gq)


def genotypes(rescored, het=1e-3, prior=None, scale=1.0):
    """Genotype every variant of a GenomeVariantsRescored: genotype_likelihoods on the device, call_genotypes on the host.
    -> VariantCalls."""
    p = genotype_prior(het, prior)
    gl, n = genotype_likelihoods(rescored, scale)
    gt, gq, pl, qual = call_genotypes(gl.cpu().numpy(), n.cpu().numpy(), prior=p)
    return VariantCalls(rescored, gl, n, gt, gq, pl, qual, p, float(scale))


def merged_variants(index, first, more, kmer_len):
    """The rows of the VariantSet `first` followed by those of `more` (a list of (contig, pos, ndel, alt), a VariantSet or 'repeats')
    that are not among them already, by content (contig name, pos, ndel, alt).  -> `first` itself when nothing is added, else a new
    VariantSet (upload_variants)."""
    if more is None:
        return first
    added = _as_variant_set(index, more, kmer_len)
    if len(first) == 0 and len(set(added.rows())) == len(added):
        return added
    extra = added.rows()
    rows = first.rows()
    seen = set(rows)
    for row in extra:
        if row not in seen:
            seen.add(row)
            rows.append(row)
    return first if len(rows) == len(first) else upload_variants(index, rows, kmer_len)


def call_variants(post, steps, paths, lens, move_row, index, res, strand, info, ops, kmer_len, min_count=2, min_fraction=0.2, min_depth=3,
                  max_del=8, max_ins=4, het=1e-3, prior=None, scale=1.0, variants=None, region=None, width=512, margin=None, keep=None,
                  blank=0, min_prob=None, workspace_limit=None):
    """Call the variants of a sample against the genome its reads were mapped to (design/genotypes.md): a genome.Pileup of the kept
    reads over `region`, its alleles (Pileup.alleles; min_count, min_fraction, min_depth, max_del), with `variants` (a list, a
    VariantSet or 'repeats') added where they are not among them, put to the reads' signal on the SAME mapping (rescore_variants) and
    genotyped (genotypes).  Everything else as rescore_variants takes it.  -> VariantCalls."""
    from . import genome as G
    pile = G.Pileup(index, region=region, max_ins=max_ins)
    pile.add(res, strand, info, ops, keep=keep)
    alleles = pile.alleles(kmer_len, min_count=min_count, min_fraction=min_fraction, min_depth=min_depth, max_del=max_del)
    asked = merged_variants(index, alleles, variants, kmer_len)
    got = rescore_variants(post, steps, paths, lens, move_row, index, res, strand, info, ops, kmer_len, asked, width=width, margin=margin,
                           keep=keep, blank=blank, min_prob=min_prob, workspace_limit=workspace_limit)
    calls = genotypes(got, het=het, prior=prior, scale=scale)
    calls.pileup, calls.skipped = pile, alleles.skipped
    return calls
