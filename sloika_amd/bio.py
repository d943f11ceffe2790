"""States -> k-mers -> bases (the step after the decoded path; reference: sloika/bio.py:12-36, 145-237).

A k-mer over an alphabet of `nbase` letters is handled as the base-`nbase` NUMBER of its letters, first letter most
significant -- the index `all_kmers` gives it (bio.py:12-24).  The reference's string tests then become integer ones:

    k1[i:] == k2[:-i]      <=>      s1 mod nbase^(k-i) == s2 div nbase^i

`paths_to_bases` runs whole batches of decoded paths on the device (csrc/bases.hip, C ABI slk_paths_to_bases);
`paths_to_bases_qual` does the same with a Phred value beside every letter (slk_paths_to_bases_qual, design/lattice_marginals.md)
and `fastq_text` prints them;
`kmers_to_sequence` & co. keep the reference's string-level signatures for single calls and evaluate the same integer
rule with numpy (they are host-side string utilities in the reference too).
"""
from itertools import product

import numpy as np


def all_kmers(length, alphabet='ACGT'):
    """Every k-mer of `length` letters in alphabet order (bio.py:12-24); bytes in, bytes out."""
    as_bytes = isinstance(alphabet, bytes)
    letters = alphabet.decode('utf-8') if as_bytes else alphabet
    words = (''.join(w) for w in product(letters, repeat=length))
    return [w.encode('utf-8') for w in words] if as_bytes else list(words)


def kmer_mapping(length, alphabet='ACGT'):
    """k-mer -> its index in all_kmers (bio.py:27-36)."""
    return dict((kmer, idx) for idx, kmer in enumerate(all_kmers(length, alphabet)))


def seq_to_kmers(seq, length):
    """The overlapping k-mers of a string, in order (bio.py:145-157)."""
    return [seq[start:start + length] for start in range(len(seq) - length + 1)]


def _alphabet_of(kmers):
    letters = sorted(set(ch for k in kmers for ch in (k.decode('utf-8') if isinstance(k, bytes) else k)))
    return ''.join(letters)


def _states(kmers, alphabet):
    """k-mer strings -> (state numbers int64, k, nbase) under `alphabet` (letter rank = digit)."""
    k = len(kmers[0])
    rank = np.full(256, -1, dtype=np.int64)
    rank[np.frombuffer(alphabet.encode('utf-8'), dtype=np.uint8)] = np.arange(len(alphabet))
    text = b''.join(x if isinstance(x, bytes) else x.encode('utf-8') for x in kmers)
    digits = rank[np.frombuffer(text, dtype=np.uint8)].reshape(len(kmers), k)
    if (digits < 0).any():
        raise ValueError("k-mer letter outside the alphabet %r" % alphabet)
    weights = len(alphabet) ** np.arange(k - 1, -1, -1, dtype=np.int64)
    return digits @ weights, k, len(alphabet)


def moves_of_states(states, k, nbase, allow_identical=True):
    """Moves between consecutive states: 0 for a repeat (when allowed), else the smallest shift i in 1..k-1 whose
    suffix/prefix digits agree, else k (bio.py:160-179)."""
    states = np.asarray(states, dtype=np.int64)
    s1, s2 = states[:-1], states[1:]
    move = np.full(len(s1), k, dtype=np.int64)
    for shift in range(k - 1, 0, -1):                       # later assignments are smaller shifts: the smallest wins
        agree = (s1 % nbase ** (k - shift)) == (s2 // nbase ** shift)
        move[agree] = shift
    if allow_identical:
        move[s1 == s2] = 0
    return move


def sequence_of_states(states, k, nbase, moves, alphabet):
    """First state in full, then the last min(move, k) letters of every following state (bio.py:206-225)."""
    states = np.asarray(states, dtype=np.int64)
    moves = np.minimum(np.asarray(moves, dtype=np.int64), k)
    take = np.concatenate(([k], moves))                      # letters contributed by each state
    total = int(take.sum())
    owner = np.repeat(np.arange(len(states)), take)          # which state each output letter comes from
    start = np.cumsum(take) - take
    within = np.arange(total) - start[owner]                 # 0 .. take-1 inside the contribution
    place = take[owner] - 1 - within                         # digit position counted from the least significant
    digits = (states[owner] // nbase ** place) % nbase
    return np.frombuffer(alphabet.encode('utf-8'), dtype=np.uint8)[digits].tobytes().decode('utf-8')


def max_overlap(kmers, allow_identical=True):
    """List of moves between consecutive k-mer strings (bio.py:160-179)."""
    kmers = list(kmers)
    if len(kmers) < 2:
        return []
    alphabet = _alphabet_of(kmers)
    states, k, nbase = _states(kmers, alphabet)
    return [int(m) for m in moves_of_states(states, k, max(nbase, 2), allow_identical)]


def moves_compatible(kmers, moves):
    """Per transition: does the claimed move agree with the two k-mers (bio.py:182-203)?  A move of k or more always
    does (nothing left to compare), a move of 0 needs identical k-mers."""
    kmers = list(kmers)
    if len(kmers) < 2:
        return []
    alphabet = _alphabet_of(kmers)
    states, k, nbase = _states(kmers, alphabet)
    nbase = max(nbase, 2)
    out = []
    for s1, s2, m in zip(states[:-1], states[1:], moves):
        if m == 0:
            out.append(bool(s1 == s2))
        elif m >= k:
            out.append(True)
        else:
            out.append(bool(s1 % nbase ** (k - m) == s2 // nbase ** m))
    return out


def reduce_kmers(kmers, moves):
    """k-mer strings + moves -> sequence (bio.py:206-225)."""
    kmers = list(kmers)
    assert all(moves_compatible(kmers, moves)), 'Moves not consistent with kmers'
    alphabet = _alphabet_of(kmers)
    states, k, nbase = _states(kmers, alphabet)
    seq = sequence_of_states(states, k, max(nbase, 2), list(moves)[:len(kmers) - 1], alphabet)
    return seq.encode('utf-8') if isinstance(kmers[0], bytes) else seq


def kmers_to_sequence(kmers, always_move=False):
    """Sequence of a list of k-mer strings by maximum overlap (bio.py:228-237)."""
    kmers = list(kmers)
    return reduce_kmers(kmers, max_overlap(kmers, not always_move))


def states_to_sequence(states, klen, alphabet='ACGT', always_move=False):
    """The same for a path of STATE NUMBERS (what decode.viterbi returns): no strings are built on the way."""
    if isinstance(alphabet, bytes):
        alphabet = alphabet.decode('utf-8')
    states = np.asarray(states, dtype=np.int64)
    if states.size == 0:
        return ''
    moves = moves_of_states(states, klen, len(alphabet), not always_move)
    return sequence_of_states(states, klen, len(alphabet), moves, alphabet)


def paths_to_bases(paths, lens, klen, alphabet='ACGT', always_move=True):
    """Batch of decoded paths on the device -> list of base strings.  paths:[B, T] int32 device tensor (rows valid for
    lens[b] entries, as pipeline.Basecaller.call_chunks returns them), lens:[B] int32 device tensor."""
    import torch
    from . import _lib, device as D
    _lib.require_gpu()
    if isinstance(alphabet, str):
        alphabet = alphabet.encode('utf-8')
    B, Tmax = paths.shape
    cap = max(klen * max(Tmax, 1), klen)
    out = torch.empty((B, cap), dtype=torch.uint8, device=paths.device)
    nb = torch.empty((B,), dtype=torch.int32, device=paths.device)
    packed = int.from_bytes(alphabet.ljust(8, b'\0'), 'little')
    _lib.check(_lib.lib().slk_paths_to_bases(paths.data_ptr(), paths.stride(0), lens.data_ptr(), B, klen, len(alphabet),
                                             int(bool(always_move)), packed, out.data_ptr(), cap, nb.data_ptr(),
                                             D.stream_ptr()), "paths_to_bases")
    counts = nb.cpu().numpy()
    host = out[:, :int(counts.max()) if B else 0].cpu().numpy()
    return [host[b, :counts[b]].tobytes().decode('utf-8') for b in range(B)]


#: the largest Phred value a FASTQ line can print (Phred + 33 <= 126, '~')
PHRED_MAX = 93


def phred_thresholds(qmax=60):
    """float64 [qmax]: entry k - 1 is 10^(-k/10), the largest error probability that still earns Phred k.  The Phred value of an error
    probability is the number of entries it does not exceed -- on the device (slk_paths_to_bases_qual) and, for the same table,
    `qmax - np.searchsorted(table[::-1], err, side='left')`."""
    qmax = int(qmax)
    if not 1 <= qmax <= PHRED_MAX:
        raise ValueError("qmax must lie in 1 .. %d" % PHRED_MAX)
    return np.array([10.0 ** (-k / 10.0) for k in range(1, qmax + 1)], dtype=np.float64)


def phred_of_error(err, qmax=60):
    """Host restatement of the device's rule: int64 Phred values of error probabilities (NaN -> 0)."""
    table = phred_thresholds(qmax)
    err = np.asarray(err, dtype=np.float64)
    q = qmax - np.searchsorted(table[::-1], err, side='left')
    return np.where(np.isnan(err), 0, q).astype(np.int64)


def paths_to_bases_qual(paths, lens, conf, klen, alphabet='ACGT', qmax=60):
    """paths_to_bases(always_move=True) with a quality per letter: conf [B, T] float64 device tensor, one confidence per path position
    (decode.viterbi_marginals_batch); a letter gets the Phred value of 1 - conf of the position that emitted it, capped at qmax.
    -> list of B (base string, uint8 array of Phred values)."""
    import torch
    from . import _lib, device as D
    _lib.require_gpu()
    if isinstance(alphabet, str):
        alphabet = alphabet.encode('utf-8')
    B, Tmax = paths.shape
    if conf.dtype != torch.float64 or conf.shape[0] != B or conf.shape[1] < Tmax or conf.stride(1) != 1:
        raise ValueError("conf must be a float64 device tensor with one row per path and one entry per position")
    table = torch.from_numpy(phred_thresholds(qmax)).to(paths.device)
    cap = max(klen * max(Tmax, 1), klen)
    out = torch.empty((B, cap), dtype=torch.uint8, device=paths.device)
    qual = torch.empty((B, cap), dtype=torch.uint8, device=paths.device)
    nb = torch.empty((B,), dtype=torch.int32, device=paths.device)
    packed = int.from_bytes(alphabet.ljust(8, b'\0'), 'little')
    _lib.check(_lib.lib().slk_paths_to_bases_qual(paths.data_ptr(), paths.stride(0), lens.data_ptr(), conf.data_ptr(), conf.stride(0),
                                                  table.data_ptr(), int(qmax), B, klen, len(alphabet), 1, packed, out.data_ptr(),
                                                  qual.data_ptr(), cap, nb.data_ptr(), D.stream_ptr()), "paths_to_bases_qual")
    counts = nb.cpu().numpy()
    width = int(counts.max()) if B else 0
    host, hq = out[:, :width].cpu().numpy(), qual[:, :width].cpu().numpy()
    return [(host[b, :counts[b]].tobytes().decode('utf-8'), hq[b, :counts[b]].copy()) for b in range(B)]


def fastq_text(names, bases, quals):
    """FASTQ text of calls: four lines per read, qualities as Phred + 33 (Sanger).  quals[b]: one integer in 0 .. 93 per letter."""
    if not len(names) == len(bases) == len(quals):
        raise ValueError("fastq_text needs one name, one sequence and one quality array per read")
    out = []
    for name, seq, q in zip(names, bases, quals):
        q = np.asarray(q)
        if isinstance(seq, bytes):
            seq = seq.decode('ascii')
        if q.shape != (len(seq),):
            raise ValueError("read %s: %d qualities for %d letters" % (name, q.size, len(seq)))
        if q.size and (q.min() < 0 or q.max() > PHRED_MAX):
            raise ValueError("read %s: qualities must lie in 0 .. %d" % (name, PHRED_MAX))
        out.append("@%s\n%s\n+\n%s\n" % (name, seq, (q.astype(np.uint8) + 33).tobytes().decode('ascii')))
    return "".join(out)


def fastq_records(text):
    """The inverse of fastq_text: FASTQ text of four lines per record -> [(name, bases str, uint8 array of Phred values)].  A record
    that is not '@name', letters, '+' (a repeated name is allowed), as many quality characters in '!' .. '~' raises a ValueError
    that gives the record's number (from 1)."""
    if isinstance(text, bytes):
        text = text.decode('ascii')
    lines = text.split("\n")
    if lines and lines[-1] == "":
        lines.pop()
    if len(lines) % 4:
        raise ValueError("fastq_records: record %d is cut short: %d lines are no whole number of records" % (len(lines) // 4 + 1, len(lines)))
    out = []
    for k in range(len(lines) // 4):
        head, seq, plus, qual = lines[4 * k:4 * k + 4]
        if not head.startswith("@"):
            raise ValueError("fastq_records: record %d does not begin with '@'" % (k + 1))
        if not plus.startswith("+") or (len(plus) > 1 and plus[1:] != head[1:]):
            raise ValueError("fastq_records: record %d has no '+' line" % (k + 1))
        if len(qual) != len(seq):
            raise ValueError("fastq_records: record %d has %d qualities for %d letters" % (k + 1, len(qual), len(seq)))
        try:
            q = np.frombuffer(qual.encode('ascii'), dtype=np.uint8).astype(np.int16) - 33
        except UnicodeEncodeError:
            q = np.array([-1], dtype=np.int16)
        if q.size and (q.min() < 0 or q.max() > PHRED_MAX):
            raise ValueError("fastq_records: record %d has a quality character outside '!' .. '~'" % (k + 1))
        out.append((head[1:], seq, q.astype(np.uint8)))
    return out


#: the kinds of single_letter_edits, in the order in which a position lists them
EDIT_KINDS = ('sub', 'del', 'ins')


def single_letter_edits(seq, kinds=EDIT_KINDS, alphabet='ACGT'):
    """Every single-letter edit of a base string: rows (kind, letter_pos, letter, edited_string), ordered by letter_pos, then kind
    ('sub', 'del', 'ins'), then letter in alphabet order.  'sub' puts another letter at letter_pos, 'del' removes the letter there
    (letter ''), 'ins' puts a letter in front of letter_pos (letter_pos = len(seq): behind the end): about 8 len(seq) rows."""
    unknown = [k for k in kinds if k not in EDIT_KINDS]
    if unknown:
        raise ValueError("unknown kind of edit %r (known: %s)" % (unknown[0], ', '.join(EDIT_KINDS)))
    rows = []
    for pos in range(len(seq) + 1):
        for kind in EDIT_KINDS:
            if kind not in kinds:
                continue
            if kind == 'sub' and pos < len(seq):
                rows.extend((kind, pos, c, seq[:pos] + c + seq[pos + 1:]) for c in alphabet if c != seq[pos])
            elif kind == 'del' and pos < len(seq):
                rows.append((kind, pos, '', seq[:pos] + seq[pos + 1:]))
            elif kind == 'ins':
                rows.extend((kind, pos, c, seq[:pos] + c + seq[pos:]) for c in alphabet)
    return rows


def apply_letter_edits(seq, edits):
    """`seq` after the (kind, letter_pos, letter) edits of single_letter_edits, all of them positions of `seq` itself (applied from
    the back, so that no edit moves another; at most one edit per position)."""
    out = seq
    for kind, pos, letter in sorted(edits, key=lambda e: -e[1]):
        if kind == 'sub':
            out = out[:pos] + letter + out[pos + 1:]
        elif kind == 'del':
            out = out[:pos] + out[pos + 1:]
        elif kind == 'ins':
            out = out[:pos] + letter + out[pos:]
        else:
            raise ValueError("unknown kind of edit %r" % (kind,))
    return out


def seq_to_states(seq, length, alphabet='ACGT'):
    """The k-mer states of a base string (seq_to_kmers numbered by kmer_mapping) as int64, without building the k-mers."""
    text = seq.encode('utf-8') if isinstance(seq, str) else bytes(seq)
    rank = np.full(256, -1, dtype=np.int64)
    rank[np.frombuffer(alphabet.encode('utf-8'), dtype=np.uint8)] = np.arange(len(alphabet))
    digits = rank[np.frombuffer(text, dtype=np.uint8)]
    if (digits < 0).any():
        raise ValueError("letter outside the alphabet %r" % alphabet)
    n = len(digits) - length + 1
    if n <= 0:
        return np.zeros(0, dtype=np.int64)
    states = np.zeros(n, dtype=np.int64)
    for j in range(length):
        states = states * len(alphabet) + digits[j:j + n]
    return states


def edit_states(old_states, new_states):
    """The edit that turns one state sequence into another: (start, ndel, new) with
    new_states == old_states[:start] + new + old_states[start + ndel:], by stripping the common prefix, then the common suffix of
    what is left.  A single-letter edit of a base string changes at most kmer_len consecutive k-mers and adds or removes one, so `new`
    has at most kmer_len + 1 entries."""
    old = np.asarray(old_states, dtype=np.int64).reshape(-1)
    new = np.asarray(new_states, dtype=np.int64).reshape(-1)
    n = min(len(old), len(new))
    diff = np.nonzero(old[:n] != new[:n])[0]
    pre = int(diff[0]) if diff.size else n
    rest = n - pre
    diff = np.nonzero(old[len(old) - rest:][::-1] != new[len(new) - rest:][::-1])[0] if rest else diff[:0]
    suf = int(diff[0]) if diff.size else rest
    return pre, len(old) - pre - suf, new[pre:len(new) - suf].copy()
