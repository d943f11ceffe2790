"""Signal-level polishing: turn the forward likelihood back on the sequence (design/rescore_edits.md).

Given draft base strings and the posteriors of the reads that cover them, score every single-letter edit of every draft under every
read (decode.rescore_edits_batch: one lattice per read, T x (m + 1) cells per candidate) and apply the edits the signal prefers.

    rescore_drafts(post, drafts, kmer_len, group=None, ...)   -> per group the edit table, the gains and the summed score
    polish(post, drafts, kmer_len, group=None, ...)           -> per group the polished string, the applied edits, rounds and score

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
