"""Inputs shared by tests/test_pileup_host.py and tests/test_gpu_pileup.py: a small genome with homopolymers and a dinucleotide
repeat, a sample that differs from it in five planted places, and reads of the sample from both strands.

The case is a condition on the INPUTS (design/pileup.md, "what the rules cannot do"): seed, depth and error rate are chosen so that
the plain-loop model of tests/pileup_ref.py, fed with the reference aligner's columns, reproduces the sample with gap normalisation
and does not without it.  Nothing here looks at the code under test."""
import functools

import numpy as np

from tests import align_ops_ref, pileup_ref

CONTIG = "chr"
SEED, NREADS, ERROR = 5, 70, 0.03
LEN_LO, LEN_HI = 150, 260


def _genome(rs):
    """About 470 letters: random stretches around a run of 7 A, a run of 6 T and (CA) x 5, each with flanks that differ from it."""
    def rnd(n):
        return ''.join("ACGT"[k] for k in rs.randint(0, 4, size=n))
    parts = [rnd(60), "G", rnd(39), "C", "AAAAAAA", "G", rnd(90), "G", "TTTTTT", "C", rnd(90), "G", "CACACACACA", "T", rnd(90), "ACA",
             rnd(70)]
    return parts


@functools.lru_cache(maxsize=None)
def planted():
    """-> dict: genome, sample (str), variants [(contig, pos, kind, ref, alt)] in position order as left-normalised calls report
    them, reads [str] as sequenced (a '-' read is the reverse complement of its stretch of the sample), strands [str]."""
    rs = np.random.RandomState(SEED)
    parts = _genome(rs)
    genome = ''.join(parts)
    off = np.concatenate(([0], np.cumsum([len(p) for p in parts])))
    sub_pos = int(off[1])                                        # the lone 'G' after the first stretch
    a_run, t_run, ca_run, aca = int(off[4]), int(off[8]), int(off[12]), int(off[15])
    assert genome[a_run:a_run + 7] == "AAAAAAA" and genome[t_run:t_run + 6] == "TTTTTT" and genome[ca_run:ca_run + 10] == "CA" * 5
    sample = list(genome)
    edits = [(sub_pos, 1, "T"),                                  # (position, letters replaced, by)
             (a_run + 3, 1, ""),                                 # one A out of the run
             (t_run + 2, 0, "T"),                                # one T into the run
             (ca_run + 4, 2, ""),                                # one CA out of the repeat
             (aca + 2, 0, "GT")]                                 # GT behind the C of ACA
    for pos, n, by in sorted(edits, reverse=True):
        sample[pos:pos + n] = list(by)
    sample = ''.join(sample)
    variants = [(CONTIG, sub_pos, 'sub', 'G', 'T'), (CONTIG, a_run, 'del', 'A', ''), (CONTIG, t_run - 1, 'ins', '', 'T'),
                (CONTIG, ca_run, 'del', 'C', ''), (CONTIG, ca_run + 1, 'del', 'A', ''), (CONTIG, aca + 1, 'ins', '', 'GT')]
    reads, strands = [], []
    for k in range(NREADS):
        n = int(rs.randint(LEN_LO, LEN_HI + 1))
        s = int(rs.randint(0, len(sample) - n + 1))
        if k < 4:                                                # both ends of the genome are reached on both strands
            s = 0 if k < 2 else len(sample) - n
        out = []
        for c in sample[s:s + n]:
            u = rs.random_sample()
            if u < ERROR / 3:
                out.append("ACGT"[("ACGT".index(c) + int(rs.randint(1, 4))) % 4])
            elif u < 2 * ERROR / 3:
                out.append(c + "ACGT"[int(rs.randint(0, 4))])
            elif u >= ERROR:
                out.append(c)
        read = ''.join(out)
        minus = k % 2 == 1
        reads.append(pileup_ref.revcomp(read).decode('ascii') if minus else read)
        strands.append('-' if minus else '+')
    return {'genome': genome, 'sample': sample, 'variants': variants, 'reads': reads, 'strands': strands}


@functools.lru_cache(maxsize=None)
def host_pairs():
    """The planted reads aligned by tests/align_ops_ref.ops, each against the whole contig as its window ('-' reads against its
    reverse complement, as genome.Index.map cuts it) -> [(q, window letters, row, codes, minus, t0)]."""
    case = planted()
    g = case['genome']
    rc = pileup_ref.revcomp(g).decode('ascii')
    pairs = []
    for read, strand in zip(case['reads'], case['strands']):
        minus = strand == '-'
        w = rc if minus else g
        row, codes = align_ops_ref.ops(read, w)
        t0 = len(g) - row[4] if minus else row[3]                # window = [0, G): window_end - r_end / window_start + r_start
        pairs.append((read, w, row, codes, minus, t0))
    return pairs
