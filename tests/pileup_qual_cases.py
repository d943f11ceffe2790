"""Inputs shared by tests/test_pileup_qual_host.py and tests/test_gpu_pileup_qual.py: the genome and the sample of
tests/pileup_cases.py (its five planted edits), and reads of the sample from both strands that carry no random error but, at a
handful of sample positions away from the repeats, a LOW-QUALITY error in about 65 % of the reads that cover the position:

    a substitution at Phred 3, a spurious inserted letter at Phred 2, or a dropped letter with the letter in front of it at Phred 2.

Every other letter has a quality of 25..40.  A majority vote follows the 65 %; a vote weighted by quality does not.  The case is a
condition on the INPUTS that only the plain-loop model of tests/pileup_qual_ref.py checks (tests/test_pileup_qual_host.py): the
majority consensus is not the sample, the weighted consensus is.  Nothing here looks at the code under test."""
import functools

import numpy as np

from tests import align_ops_ref, pileup_cases, pileup_ref

CONTIG = pileup_cases.CONTIG
SEED, NREADS, SHARE = 5, 70, 0.65
LEN_LO, LEN_HI = pileup_cases.LEN_LO, pileup_cases.LEN_HI
#: positions of the SAMPLE
SUBS, INSS, DELS = (20, 150, 330), (40, 250), (30, 350)
Q_SUB, Q_INS, Q_DEL = 3, 2, 2
MARGIN = 12                                                      # an error this close to a read's end is not planted


def _other(c, k=1):
    return "ACGT"[("ACGT".index(c) + k) % 4]


@functools.lru_cache(maxsize=None)
def designed():
    """-> dict: genome, sample (str), reads [str] as sequenced, quals [uint8 array] as sequenced (a '-' read's qualities are
    reversed with it), strands [str]."""
    base = pileup_cases.planted()
    genome, sample = base['genome'], base['sample']
    for p in DELS:                                               # the dropped letter's gap has nowhere to go, nor has the inserted one
        assert sample[p] != sample[p - 1]
    rs = np.random.RandomState(SEED)
    reads, quals, strands = [], [], []
    for k in range(NREADS):
        n = int(rs.randint(LEN_LO, LEN_HI + 1))
        s = int(rs.randint(0, len(sample) - n + 1))
        if k < 4:
            s = 0 if k < 2 else len(sample) - n
        letters, qs = [], []
        for g in range(s, s + n):
            c, v = sample[g], int(rs.randint(25, 41))
            inner = s + MARGIN <= g < s + n - MARGIN
            hit = inner and rs.random_sample() < SHARE if g in SUBS + INSS + DELS else False
            if hit and g in SUBS:
                letters.append(_other(c))
                qs.append(Q_SUB)
            elif hit and g in INSS:                              # a letter that is neither neighbour's, behind the position's own
                nxt = sample[g + 1]
                letters += [c, [x for x in "ACGT" if x != c and x != nxt][0]]
                qs += [v, Q_INS]
            elif hit and g in DELS:                              # the letter is dropped; the one in front of it is the doubtful one
                qs[-1] = Q_DEL
            else:
                letters.append(c)
                qs.append(v)
        read, q = ''.join(letters), np.array(qs, dtype=np.uint8)
        minus = k % 2 == 1
        reads.append(pileup_ref.revcomp(read).decode('ascii') if minus else read)
        quals.append(q[::-1].copy() if minus else q)
        strands.append('-' if minus else '+')
    return {'genome': genome, 'sample': sample, 'reads': reads, 'quals': quals, 'strands': strands}


@functools.lru_cache(maxsize=None)
def host_pairs():
    """The designed reads aligned by tests/align_ops_ref.ops, each against the whole contig as its window, as
    pileup_cases.host_pairs does -> [(q, window letters, row, codes, minus, t0, qual)]."""
    case = designed()
    g = case['genome']
    rc = pileup_ref.revcomp(g).decode('ascii')
    pairs = []
    for read, qual, strand in zip(case['reads'], case['quals'], case['strands']):
        minus = strand == '-'
        w = rc if minus else g
        row, codes = align_ops_ref.ops(read, w)
        t0 = len(g) - row[4] if minus else row[3]
        pairs.append((read, w, row, codes, minus, t0, qual))
    return pairs
