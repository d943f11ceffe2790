"""CPU model of csrc/genotype.hip and of the host half of the variant caller, plain loops written from design/genotypes.md section 1: the
alleles a pileup proposes, the genotype sums in extended precision (np.longdouble), the call, the VCF text, a helper that applies VCF
records to a reference, and a planted diploid sample.  Pure Python and numpy; it shares no arithmetic with the kernels or with
sloika_amd.polish.  tests/test_genotype_ref.py pins it with no GPU, tests/test_gpu_genotype.py compares the device with it."""
import numpy as np

from tests.polish_genome_ref import SAMPLE_RUN, SAMPLE_WINDOWS, revcomp

MAX_NEW = 8
SKIP_INS, SKIP_DEL = 1, 2
LD = np.longdouble


def max_alt(klen):
    return MAX_NEW - klen + 1


# ---- 1. alleles ----------------------------------------------------------------------------------------------------------------------

def passes(n, d, min_count, permille, min_depth):
    return int(n) >= min_count and 1000 * int(n) >= permille * int(d) and int(d) >= min_depth


def alleles(counts, ins, genome, contig_off, lo, klen, min_depth=3, min_count=2, permille=200, max_del=8):
    """counts [P][8], ins [P][S][5] over the packed positions lo .. lo + P - 1 of the genome string; contig_off: the contigs' starts
    and G.  -> (variants [(contig offset, pos, ndel, alt)] in order, nprop [P], nalt [P], skipped [P])."""
    counts, ins = np.asarray(counts).reshape(-1, 8), np.asarray(ins)
    P = counts.shape[0]
    S = ins.shape[1] if P else 0
    ok = lambda n, d: passes(n, d, min_count, permille, min_depth)           # noqa: E731
    depth = [int(counts[t, :6].sum()) for t in range(P)]
    deleted = [ok(counts[t, 5], depth[t]) for t in range(P)]
    out, nprop, nalt, skipped = [], [0] * P, [0] * P, [0] * P
    for t in range(P):
        g = lo + t
        ci = max(i for i in range(len(contig_off) - 1) if contig_off[i] <= g)
        c0, c1 = contig_off[ci], contig_off[ci + 1]
        if genome[g] not in 'ACGT':
            continue
        q, mine = g - c0, []
        before = t >= 1 and g - 1 >= c0                                        # the table holds the letter in front, in this contig
        if before:
            alt = ''
            for k in range(S):
                row = [int(v) for v in ins[t - 1, k]]
                best = max(row[:4])
                if not ok(sum(row), counts[t - 1, 7]) or best <= 0:
                    break
                alt += 'ACGT'[row[:4].index(best)]
            if len(alt) > max_alt(klen):
                skipped[t] |= SKIP_INS
            elif alt:
                mine.append((c0, q, 0, alt))
        for c in range(4):
            if 'ACGT'[c] != genome[g] and ok(counts[t, c], depth[t]):
                mine.append((c0, q, 1, 'ACGT'[c]))
        if deleted[t] and not (before and deleted[t - 1]):
            L = 1
            while t + L < P and g + L < c1 and deleted[t + L]:
                L += 1
            if L > max_del:
                skipped[t] |= SKIP_DEL
            elif all(ch in 'ACGT' for ch in genome[g:g + L]):
                mine.append((c0, q, L, ''))
        out += mine
        nprop[t], nalt[t] = len(mine), sum(len(v[3]) for v in mine)
    return out, nprop, nalt, skipped


# ---- 2. genotype sums, extended precision --------------------------------------------------------------------------------------------

def genotype_sums(score, ll_edit, cand_read, cand_var, V, scale=1.0):
    """-> (gl [V][3] longdouble, n [V] int, size [V] longdouble: the sum of max(1, |d|) over the reads counted).  The candidates of a
    variant in read order (ties as they come); both values finite: d = scale (ll_edit - score), gl1 += log(1/2 + 1/2 e^d), gl2 += d; a
    NaN of either value makes the three NaN; an infinity is not counted."""
    gl = np.zeros((V, 3), dtype=LD)
    n, size, bad = np.zeros(V, dtype=np.int64), np.zeros(V, dtype=LD), np.zeros(V, dtype=bool)
    for i in sorted(range(len(cand_var)), key=lambda i: (int(cand_var[i]), int(cand_read[i]))):
        v, r = int(cand_var[i]), int(cand_read[i])
        if v < 0 or v >= V:
            continue
        l, s = float(ll_edit[i]), float(score[r]) if 0 <= r < len(score) else float('nan')
        if l != l or s != s:
            bad[v] = True
        elif np.isfinite(l) and np.isfinite(s):
            d = LD(scale) * (LD(l) - LD(s))
            gl[v, 1] += max(d, LD(0)) + np.log1p(np.exp(-abs(d))) - np.log(LD(2))
            gl[v, 2] += d
            n[v] += 1
            size[v] += max(LD(1), abs(d))
    gl[bad] = np.nan
    return gl, n, size


def e_gt(n, size):
    """E_gt = 2^-53 (n + 4) x the sum of max(1, |d_r|): the sequential float64 sum of n terms (n - 1 roundings, each at most 2^-53 of
    a partial sum that the sum of |term| bounds, |term| <= max(1, |d|) since 0 <= log(1/2 + 1/2 e^d) + ln 2 - max(d, 0) <= ln 2) plus
    the roundings of one term: the difference l - s, the product with scale, exp, log1p and the two additions, a few units in the last
    place of a value of at most max(1, |d|) each."""
    return np.asarray(size, dtype=np.float64) * (np.asarray(n, dtype=np.float64) + 4.0) * 2.0 ** -53


# ---- 3. the call ---------------------------------------------------------------------------------------------------------------------

def prior_of(het=1e-3):
    return (1.0 - 1.5 * het, het, het / 2.0)


def posteriors(gl, prior):
    """Normalised log-posteriors of one variant in extended precision."""
    p = np.array([LD(g) + np.log(LD(q)) for g, q in zip(gl, prior)], dtype=LD)
    mx = p.max()
    return p - (mx + np.log(np.exp(p - mx).sum()))


def call(gl, n, prior):
    """One variant: -> (gt, gq, pl, qual, lead: best - second log-posterior)."""
    if n == 0 or any(g != g for g in gl):
        return -1, 0, (0, 0, 0), 0.0, None
    post = posteriors(gl, prior)
    gt = max(range(3), key=lambda g: (post[g], -g))
    ranked = sorted(post)
    k = LD(10) / np.log(LD(10))
    lead = ranked[2] - ranked[1]
    gq = int(min(99, np.floor(k * lead)))
    top = max(LD(g) for g in gl)
    pl = tuple(int(min(999, np.rint(-k * (LD(g) - top)))) for g in gl)
    qual = float(round(float(min(LD(999), -k * post[0])), 1)) + 0.0
    return gt, gq, pl, qual, float(lead)


# ---- 4. VCF --------------------------------------------------------------------------------------------------------------------------

def vcf_record(c, pos, ndel, alt):
    if ndel == 1 and len(alt) == 1:
        return pos + 1, c[pos], alt
    if ndel and alt:
        return pos + 1, c[pos:pos + ndel], alt
    if pos > 0:
        return pos, c[pos - 1:pos + ndel], c[pos - 1] + alt
    return 1, c[0:ndel + 1], alt + c[ndel]


def apply_vcf(reference, text, want=lambda fields, gt: fields[6] == 'PASS' and gt in ('0/1', '1/1')):
    """Apply the records of a VCF text that `want(fields, GT)` accepts to reference: {contig: string} -> {contig: string}.  REF must
    stand where the record says; records are applied from the back of each contig, and two that overlap raise."""
    recs = {}
    for line in text.splitlines():
        if line.startswith('#'):
            continue
        f = line.split('\t')
        gt = f[9].split(':')[f[8].split(':').index('GT')]
        if want(f, gt):
            recs.setdefault(f[0], []).append((int(f[1]) - 1, f[3], f[4]))
    out = dict(reference)
    for name, mine in recs.items():
        s, limit = out[name], None
        for start, ref, alt in sorted(mine, reverse=True):
            assert s[start:start + len(ref)] == ref, (name, start, ref)
            if limit is not None and start + len(ref) > limit:
                raise ValueError("the records at %s:%d and behind it overlap" % (name, start + 1))
            s, limit = s[:start] + alt + s[start + len(ref):], start
        out[name] = s
    return out


# ---- a planted diploid sample ----------------------------------------------------------------------------------------------------------

#: reference coordinates: (AC)x6, and where the haplotypes differ from the reference
DIPLOID_AC, DIPLOID_SUB_A, DIPLOID_SUB_B, DIPLOID_INS = (150, 162), 80, 220, 450


def planted_diploid(seed=7, k=3, nletters=600):
    """polish_genome_ref.planted_genome's recipe for a diploid sample: a reference of `nletters` random letters with (AC)x6 at DIPLOID_AC
    and a homopolymer of five A at SAMPLE_RUN.  Haplotype A is the reference with a substitution at DIPLOID_SUB_A and one letter of
    the run dropped; haplotype B is A with a second substitution at DIPLOID_SUB_B, one AC unit deleted and 'GT' put in front of
    DIPLOID_INS, away from any tract.  SAMPLE_WINDOWS is spelled once from each haplotype (A: the odd reads as the reverse complement,
    B: the even ones), 24 float32 posteriors over twice as many rows as the window has k-mers, and read 24 spells an unrelated
    string.  -> dict(reference, hap_a, hap_b, post, steps, texts, k, planted: the five variants (pos, ndel, alt) on the reference, as a
    left-normalised pileup reports them, genotypes: theirs)"""
    rng = np.random.default_rng(seed)
    letters = [('ACGT')[i] for i in rng.integers(0, 4, size=nletters)]
    a, b = DIPLOID_AC
    letters[a - 1], letters[b] = 'G', 'T'
    letters[a:b] = 'AC' * ((b - a) // 2)
    a, b = SAMPLE_RUN
    letters[a - 1], letters[b] = 'C', 'G'
    letters[a:b] = 'A' * (b - a)
    x = DIPLOID_INS
    letters[x - 4:x + 6] = 'GATCACTGCA'                           # ... G A T C [G T] A C T G C A ...: the insertion lengthens no tract
    for p in (DIPLOID_SUB_A, DIPLOID_SUB_B):                       # a substituted letter stands in no run and makes none
        letters[p - 2:p + 3] = 'GATCG'
    ref = ''.join(letters)
    sub_a = next(c for c in 'ACGT' if c not in (ref[DIPLOID_SUB_A - 1], ref[DIPLOID_SUB_A], ref[DIPLOID_SUB_A + 1]))
    sub_b = next(c for c in 'TGCA' if c not in (ref[DIPLOID_SUB_B - 1], ref[DIPLOID_SUB_B], ref[DIPLOID_SUB_B + 1]))
    planted = [(DIPLOID_SUB_A, 1, sub_a), (DIPLOID_AC[0], 2, ''), (DIPLOID_SUB_B, 1, sub_b), (SAMPLE_RUN[0], 1, ''), (x, 0, 'GT')]
    genotypes = [2, 1, 1, 2, 1]

    def spell(which):
        s = ref
        for pos, ndel, alt in sorted(which, reverse=True):
            s = s[:pos] + alt + s[pos + ndel:]
        return s
    hap_a = spell([planted[0], planted[3]])
    hap_b = spell(planted)
    texts = [hap_a[s:e] if i % 2 == 0 else revcomp(hap_a[s:e]) for i, (s, e) in enumerate(SAMPLE_WINDOWS)]
    texts += [hap_b[s:e] if i % 2 == 1 else revcomp(hap_b[s:e]) for i, (s, e) in enumerate(SAMPLE_WINDOWS)]
    texts.append(''.join('ACGT'[i] for i in rng.integers(0, 4, size=260)))
    S = 4 ** k + 1
    steps = np.array([2 * (len(t) - k + 1) for t in texts], dtype=np.int32)
    post = rng.uniform(size=(int(steps.max()), len(texts), S)).astype(np.float32) * np.float32(0.2)
    post[:, :, 0] += 1.0
    for r, t in enumerate(texts):
        st = np.array([sum('ACGT'.index(c) * 4 ** (k - 1 - i) for i, c in enumerate(t[p:p + k])) for p in range(len(t) - k + 1)])
        rows = np.sort(rng.choice(int(steps[r]), size=len(st), replace=False))
        post[rows, r, 0] -= 1.0
        post[rows, r, st + 1] += 1.0
    post /= post.sum(axis=2, keepdims=True)
    return dict(reference=ref, hap_a=hap_a, hap_b=hap_b, post=post, steps=steps, texts=texts, k=k, planted=planted, genotypes=genotypes)
