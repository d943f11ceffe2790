"""The two helpers of sloika/util.py that sit on the path (behaviour of util.py:12-26 and :94-99, restated)."""
import numpy as np


def geometric_prior(n, m, rev=False):
    """log P(start at step k), k = 0 .. n-1, for a geometric start time with mean `m` steps: log p + k log(1 - p), p = 1 / (1 + m);
    `rev` gives the same numbers back to front (the prior on the END of the sequence, transducer.py:39-41, 63-64)."""
    p = 1.0 / (1.0 + m)
    steps = np.arange(n, dtype=np.float64)
    steps = steps[::-1] if rev else steps
    out = np.full(n, np.log(p))
    out[steps > 0] += steps[steps > 0] * np.log1p(-p)         # (step 0 keeps log p itself: m = 0 gives p = 1, and 0 * log 0 is not 0)
    return out


def trim_array(x, from_start, from_end):
    """`x` without its first `from_start` and last `from_end` entries (a view; empty when they overlap, as the reference's
    `x[from_start:-from_end]`); negative counts are refused."""
    if from_start < 0 or from_end < 0:
        raise AssertionError("trim counts must not be negative")
    return x[from_start:max(from_start, len(x) - from_end)]


def fasta_records(fasta_file_name):
    """The records of a FASTA file in file order -> list of (id, sequence str).  The id is the header up to its first white space;
    the lines of a record are joined as they stand (no change of case); blank lines and text in front of the first header are
    ignored."""
    records, name, parts = [], None, []
    with open(fasta_file_name, 'r') as fh:
        for line in fh:
            line = line.strip()
            if line.startswith('>'):
                if name is not None:
                    records.append((name, ''.join(parts)))
                words = line[1:].split()
                name, parts = (words[0] if words else ''), []
            elif line and name is not None:
                parts.append(line)
    if name is not None:
        records.append((name, ''.join(parts)))
    return records


def fasta_file_to_dict(fasta_file_name):
    """The records of a FASTA file as a dict id -> sequence bytes (util.py:102-111, restated without Biopython): records that are
    empty or hold an 'N' are left out, as the reference leaves them out; a later record replaces an earlier one of the same id."""
    return {name: seq.encode('utf-8') for name, seq in fasta_records(fasta_file_name) if len(seq) > 0 and 'N' not in seq}
