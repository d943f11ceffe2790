"""The ragged batch of tests/test_gpu_align.py, built from the kernel's pass width P so that its edges move with the kernel:
reference lengths around a lane (63, 64, 65), around one pass (P - 1, P, P + 1) and over two (2 P + 3); query lengths around the
pipeline's fill (0, 1, 2, 63, 64, 65, ~200); seeded 12 % errors, homopolymers, dinucleotide repeats, embedded queries, and gaps
that open on either side of the column between two passes."""
import numpy as np

QUERY_LENGTHS = (0, 1, 2, 63, 64, 65, 203)


def random_seq(rs, n):
    return ''.join('ACGT'[k] for k in rs.randint(0, 4, size=n))


def mutate(rs, seq, rate=0.12):
    """Substitutions, insertions and deletions in equal parts, `rate` of the letters in all."""
    out = []
    for ch in seq:
        u = rs.uniform()
        if u < rate / 3:
            out.append('ACGT'[('ACGT'.index(ch) + rs.randint(1, 4)) % 4])
        elif u < 2 * rate / 3:
            out.append(ch)
            out.append('ACGT'[rs.randint(0, 4)])
        elif u < rate:
            pass
        else:
            out.append(ch)
    return ''.join(out)


def revcomp(s):
    return s[::-1].translate(str.maketrans('ACGT', 'TGCA'))


def query_of(rs, ref, n):
    """A query of exactly n letters: a 12 % error copy of a stretch of ref (placed at a seeded offset), cut or padded to n."""
    if n == 0:
        return ''
    if len(ref) > n:
        at = rs.randint(0, len(ref) - n + 1)
        core = ref[at:at + n]
    else:
        core = ref
    q = mutate(rs, core)
    return (q + random_seq(rs, n))[:n]


def batch(P, seed=20):
    """-> list of (name, query, reference)."""
    rs = np.random.RandomState(seed)
    cases = []
    for m in (1, 63, 64, 65, P - 1, P, P + 1, 2 * P + 3):
        ref = random_seq(rs, m)
        for n in (QUERY_LENGTHS if m <= 65 else (1, 64, 65, 203)):
            cases.append(("err12_n%d_m%d" % (n, m), query_of(rs, ref, n), ref))
    # a whole-read-like pair: the query is an error copy of ALL of the reference, so the alignment runs through both passes
    ref = random_seq(rs, P + 1)
    cases.append(("whole_m%d" % (P + 1), mutate(rs, ref), ref))
    ref = random_seq(rs, P + 40)
    cases.append(("across_pass", mutate(rs, ref[P - 100:P + 40]), ref))
    # homopolymers and dinucleotide repeats: every tie rule decides something here
    cases.append(("homo_equal", 'A' * 65, 'A' * 65))
    cases.append(("homo_short_q", 'A' * 63, 'A' * (P + 1)))
    cases.append(("homo_long_q", 'A' * 203, 'A' * 64))
    cases.append(("homo_broken", 'A' * 64, 'A' * 30 + 'C' + 'A' * 40))
    cases.append(("homo_broken_q", 'A' * 30 + 'CC' + 'A' * 40, 'A' * (P - 1)))
    cases.append(("dinuc_equal", 'AC' * 32, 'AC' * 32))
    cases.append(("dinuc_shift", 'CA' * 32, 'AC' * (P // 2 + 2)))
    cases.append(("dinuc_del", 'AC' * 40 + 'AC' * 40, 'AC' * 40 + 'A' + 'AC' * 40))
    cases.append(("dinuc_ins", 'AC' * 50 + 'C' + 'AC' * 50, 'AC' * (P // 2 + 1)))
    cases.append(("dinuc_vs_homo", 'AC' * 32, 'A' * 65))
    cases.append(("no_common_letter", 'A' * 20, 'C' * 70))
    # a query embedded in 50 letters of random flank on each side, and the other way round
    core = random_seq(rs, 120)
    cases.append(("embedded_in_ref", mutate(rs, core), random_seq(rs, 50) + core + random_seq(rs, 50)))
    cases.append(("embedded_in_query", random_seq(rs, 50) + mutate(rs, core) + random_seq(rs, 50), core))
    core = random_seq(rs, 200)
    cases.append(("embedded_at_pass_edge", core, random_seq(rs, P - 100) + core + random_seq(rs, 50)))
    # gaps at the column between two passes (1-based columns P and P + 1): a deletion that opens in column P, one that opens in
    # column P + 1, a one-column deletion of each, and an insertion between the two columns
    ref = random_seq(rs, P + 100)
    cases.append(("del_opens_at_P", ref[P - 80:P - 1] + ref[P + 2:P + 80], ref))
    cases.append(("del_opens_at_P_plus_1", ref[P - 80:P] + ref[P + 3:P + 80], ref))
    cases.append(("del_only_P", ref[P - 80:P - 1] + ref[P:P + 80], ref))
    cases.append(("del_only_P_plus_1", ref[P - 80:P] + ref[P + 1:P + 80], ref))
    cases.append(("ins_between_passes", ref[P - 80:P] + 'GTG' + ref[P:P + 80], ref))
    cases.append(("ends_at_P", ref[P - 64:P], ref))
    cases.append(("starts_at_P", ref[P:P + 64], ref))
    return cases


def strand_batch(P, seed=21):
    """Planted reverse-complement pairs among forward ones -> list of (query, reference, planted strand)."""
    rs = np.random.RandomState(seed)
    out = []
    for k, m in enumerate((40, 65, 130, P + 7, 64, 200, 90)):
        ref = random_seq(rs, m)
        q = mutate(rs, ref[m // 8: m - m // 8])
        minus = k % 2 == 1
        out.append((revcomp(q) if minus else q, ref, '-' if minus else '+'))
    out.append(('ACGT' * 10, 'ACGT' * 10, '+'))            # its own reverse complement: a tie, which goes to '+'
    return out
