"""The variant caller on the device (csrc/genotype.hip through genome.Pileup.alleles, polish.genotype_likelihoods / genotypes /
call_variants, genome.vcf_text, pipeline.Basecaller.call_variants; design/genotypes.md).

The alleles are compared integer for integer with the plain loops of tests/genotype_ref.py on tables written by hand into a Pileup.
The genotype sums: n exactly, gl[:, 2] bit for bit with polish.sum_variant_gains at scale 1, gl[:, 1] within 4 E_gt of the
np.longdouble model, E_gt = 2^-53 (n + 4) x the sum of max(1, |d_r|) (tests/genotype_ref.e_gt; design/genotypes.md 4).  The planted
diploid sample runs through the real decoder and mapper."""

import numpy as np
import pytest

from tests.gpu_util import need_gpu, dev
from tests import genotype_ref as gr
from tests import polish_genome_ref as pg
from tests import polish_variants_ref as pv

pytestmark = pytest.mark.gpu

MIN_PROB = 1e-5


def random_letters(seed, n, letters='ACGT'):
    rng = np.random.RandomState(seed)
    return ''.join(letters[v] for v in rng.randint(0, len(letters), n))


def bits(a):
    return np.asarray(a, dtype=np.float64).view(np.uint64)


# ---- 1: alleles ----------------------------------------------------------------------------------------------------------------------

def check_alleles(contigs, region, S, klen, counts, ins, min_count=2, min_fraction=0.2, min_depth=3, max_del=8):
    """Tables written by hand into a Pileup of `region` of an index of `contigs`: every array of the set, both offset tables and the
    skipped bits equal the model, and polish.variant_edits accepts the set with every status OK.  -> (rows of the model, skipped)"""
    import torch
    from sloika_amd import genome, polish
    idx = genome.Index(contigs, k=8)
    text, off = ''.join(s for _, s in contigs), [int(v) for v in idx.offsets]
    pile = genome.Pileup(idx, region=region, max_ins=S)
    P = pile.P
    counts, ins = np.asarray(counts, dtype=np.int32).reshape(P, 8), np.asarray(ins, dtype=np.int32).reshape(P, S, 5)
    pile.counts_dev[:P].copy_(dev(counts))
    pile.ins_dev[:P].copy_(dev(ins))
    vs = pile.alleles(klen, min_count=min_count, min_fraction=min_fraction, min_depth=min_depth, max_del=max_del)
    torch.cuda.synchronize()
    want, nprop, nalt, skipped = gr.alleles(counts, ins, text, off, pile.lo, klen, min_depth, min_count, int(round(1000 * min_fraction)),
                                            max_del)
    fetch = lambda t: t.cpu().numpy()                                                           # noqa: E731
    assert np.array_equal(fetch(vs.prop_off), np.concatenate([[0], np.cumsum(nprop)])), "prop_off"
    assert np.array_equal(fetch(vs.alt_off), np.concatenate([[0], np.cumsum(nalt)])), "alt_off"
    assert np.array_equal(fetch(vs.skipped_dev), np.array(skipped, dtype=np.int32)), "skipped"
    assert len(vs) == len(want) and vs.A == sum(len(v[3]) for v in want)
    assert np.array_equal(fetch(vs.var_off), np.array([v[0] for v in want], dtype=np.int64)), "var_off"
    assert np.array_equal(fetch(vs.var_pos), np.array([v[1] for v in want], dtype=np.int64)), "var_pos"
    assert np.array_equal(fetch(vs.var_ndel), np.array([v[2] for v in want], dtype=np.int32)), "var_ndel"
    assert np.array_equal(fetch(vs.var_alt_off), np.concatenate([[0], np.cumsum([len(v[3]) for v in want])])), "var_alt_off"
    assert fetch(vs.var_alt).tobytes().decode('ascii') == ''.join(v[3] for v in want), "var_alt"
    assert vs.skipped == {'insertion': sum(1 for s in skipped if s & 1), 'deletion': sum(1 for s in skipped if s & 2)}
    assert sorted((v[0], v[1]) for v in want) == [(v[0], v[1]) for v in want]                   # sorted as it comes
    # one window per contig, both strands: the set goes into the candidate kernels as it is
    w = np.array([(off[c], 0, off[c + 1] - off[c], m) for c in range(len(contigs)) for m in (0, 1)], dtype=np.int64)
    c = polish.variant_edits(idx.genome, vs.contig_off, dev(w[:, 0].copy()), dev(w[:, 1].copy()), dev(w[:, 2].copy()),
                             dev(w[:, 3].astype(np.int32)), vs, klen, 0, 0)
    assert not fetch(c.var_status).any()
    fits = sum(2 for o, p, nd, alt in want if off[off.index(o) + 1] - o - nd + len(alt) >= klen and off[off.index(o) + 1] - o >= klen)
    assert c.ncand == fits
    return want, skipped


def random_tables(seed, text, S):
    """Small random counts: with min_count 2, 200 per mille and min_depth 3 every threshold is met and missed somewhere."""
    rng = np.random.RandomState(seed)
    P = len(text)
    counts = rng.randint(0, 4, size=(P, 8)).astype(np.int32)
    for t, ch in enumerate(text):
        if ch in 'ACGT':
            counts[t, 'ACGT'.index(ch)] += rng.randint(0, 9)
    counts[:, 5] = np.where(rng.rand(P) < 0.5, counts[:, 5], 0)
    counts[:, 7] = rng.randint(0, 14, size=P)
    ins = rng.randint(0, 4, size=(P, S, 5)).astype(np.int32)
    ins[rng.rand(P) < 0.5] = 0
    for _ in range(P // 10 + 1):                                       # deletion runs of 1 .. 4 letters
        t = rng.randint(0, P)
        counts[t:t + rng.randint(1, 5), 5] += 8
    thin = rng.rand(P) < 0.1
    counts[thin, :6] = counts[thin, :6] // 4                           # depths round min_depth
    return counts, ins


#: P -> (contigs, region): one position of a contig, two short contigs whole, two contigs whole, a slice behind a first contig
SHAPES = {1: ([("a", random_letters(1, 30))], ("a", 7, 8)),
          9: ([("a", random_letters(2, 4)), ("b", random_letters(3, 5))], None),
          70: ([("a", random_letters(4, 30, 'ACGTN')), ("b", random_letters(5, 40))], None),
          300: ([("a", random_letters(6, 20)), ("b", random_letters(7, 330, 'AACCGGTTN'))], ("b", 10, 310))}


@pytest.mark.parametrize("klen", [3, 5])
@pytest.mark.parametrize("S", [1, 4])
@pytest.mark.parametrize("P", [1, 9, 70, 300])
def test_alleles_equal_the_model(P, S, klen):
    need_gpu()
    contigs, region = SHAPES[P]
    text = ''.join(s for _, s in contigs)
    lo = 0 if region is None else (20 if P == 300 else 0) + region[1]
    counts, ins = random_tables(11 * P + S + klen, text[lo:lo + P], S)
    proposed = 0
    for kw in (dict(), dict(max_del=2, min_fraction=0.25), dict(min_count=1, min_depth=1, min_fraction=0.001, max_del=1)):
        want, skipped = check_alleles(contigs, region, S, klen, counts, ins, **kw)
        proposed += len(want)
        if P >= 70 and kw.get('max_del') == 2:
            assert any(s & 2 for s in skipped) and {0, 1, 2} <= set(v[2] for v in want)
    assert proposed > 0 or P == 1
    want, _ = check_alleles(contigs, region, S, klen, np.zeros_like(counts), np.zeros_like(ins))   # all-zero tables
    assert want == []


def edge_tables(genome, S):
    """Reference counts of 10 at every position and span 10: nothing proposes until a test spoils a row."""
    P = len(genome)
    counts, ins = np.zeros((P, 8), dtype=np.int32), np.zeros((P, S, 5), dtype=np.int32)
    for t, ch in enumerate(genome):
        counts[t, 'ACGT'.find(ch) if ch in 'ACGT' else 4] = 10
    counts[:, 7] = 10
    return counts, ins


def test_alleles_on_every_threshold():
    """A count exactly on each of the three thresholds and one below it, for a substitution, a deletion and an insertion."""
    need_gpu()
    genome = "GATC" * 10
    contigs = [("a", genome)]
    counts, ins = edge_tables(genome, 2)
    kw = dict(min_count=3, min_fraction=0.25, min_depth=12)
    sub = lambda t, n, ref: counts.__setitem__((t, slice(0, 4)), [n if x == 'C' else ref if x == genome[t] else 0 for x in 'ACGT'])   # noqa: E731
    sub(1, 3, 9)                 # A: 3 of 12 C: on min_count, on 250 per mille, on min_depth
    sub(5, 2, 10)                # 2 of 12: below min_count
    sub(9, 3, 10)                # 3 of 13: below 250 per mille
    sub(13, 3, 8)                # 3 of 11: below min_depth
    for t, (n, ref) in ((17, (3, 9)), (21, (3, 10)), (25, (3, 8)), (29, (2, 10))):
        counts[t, 'ACGT'.index(genome[t])], counts[t, 5] = ref, n
    for t, (n, span) in ((32, (3, 12)), (34, (3, 13)), (36, (3, 11)), (38, (2, 12))):
        ins[t, 0, 3], counts[t, 7] = n, span
    want, skipped = check_alleles(contigs, None, 2, 3, counts, ins, **kw)
    assert want == [(0, 1, 1, 'C'), (0, 17, 1, ''), (0, 33, 0, 'T')] and not any(skipped)


@pytest.mark.parametrize("klen", [3, 5])
def test_allele_runs_insertions_and_ends(klen):
    """Two contigs with a deletion run that would continue across their boundary; a run ending at the span's end; a region whose lo
    cuts a run; runs of max_del and max_del + 1; insertions of max_alt and max_alt + 1 letters, one whose second letter fails the
    threshold, one with a tie between letters, one behind a contig's last letter; a reference N alone and inside a run; every
    position proposing."""
    need_gpu()
    a, b = "GATC" * 8 + "GANC" + "GATC" * 3, "TCAG" * 12
    contigs = [("a", a), ("b", b)]
    S, cap = 8, gr.max_alt(klen)
    counts, ins = edge_tables(a + b, S)
    na = len(a)

    def delete(first, last):
        for t in range(first, last):
            counts[t, :6] = 0
            counts[t, 4 if (a + b)[t] == 'N' else 'ACGT'.index((a + b)[t])], counts[t, 5] = 5, 5

    delete(na - 2, na + 3)                                            # across the boundary: (a, na - 2, 2) and (b, 0, 3)
    delete(4, 7)                                                      # max_del = 3 letters
    delete(12, 16)                                                    # max_del + 1: skipped
    delete(33, 36)                                                    # round the N at 34: nothing
    counts[38, 0] = 6                                                 # beside it a plain substitution
    delete(na + len(b) - 2, na + len(b))                              # ends with the span
    ins[20, :cap, 1] = 4                                              # max_alt letters of C
    ins[24, :cap + 1, 2] = 4                                          # max_alt + 1: skipped
    ins[28, 0, 0], ins[28, 1, 0] = 4, 1                               # the second letter fails
    ins[30, 0, 1], ins[30, 0, 3] = 3, 3                               # a tie: the lower class
    ins[na - 1, 0, 2] = 9                                             # behind a's last letter: position 0 of b does not propose it
    ins[33, 0, 2] = 9                                                 # in front of the N: nothing either
    kw = dict(max_del=3)
    want, skipped = check_alleles(contigs, None, S, klen, counts, ins, **kw)
    assert (0, na - 2, 2, '') in want and (na, 0, 3, '') in want and (0, 4, 3, '') in want and (na, len(b) - 2, 2, '') in want
    assert skipped[12] == gr.SKIP_DEL and not [v for v in want if 12 <= v[1] < 16 and v[0] == 0]
    assert not [v for v in want if v[0] == 0 and 33 <= v[1] <= 36] and (0, 38, 1, 'A') in want
    assert (0, 21, 0, 'C' * cap) in want and skipped[25] == gr.SKIP_INS and (0, 29, 0, 'A') in want and (0, 31, 0, 'C') in want
    assert not [v for v in want if v[2] == 0 and v[1] in (25, 34)] and not [v for v in want if v[0] == na and v[2] == 0]
    assert sum(1 for s in skipped if s) == 2
    # a region whose lo cuts the run 4 .. 6, and whose end cuts the one at 12 .. 15 down to max_del
    lo, hi = 5, 15
    part, skipped = check_alleles(contigs, ("a", lo, hi), S, klen, counts[lo:hi], ins[lo:hi], **kw)
    assert part == [(0, 5, 2, ''), (0, 12, 3, '')] and not any(skipped)
    # every position proposing
    full, _ = edge_tables(a + b, S)
    for t, ch in enumerate(a + b):
        full[t, ('ACGT'.find(ch) + 1) % 4] += 5
    everything, _ = check_alleles(contigs, None, S, klen, full, np.zeros_like(ins))
    assert len(everything) == len(a + b) - 1 and len(set(v[:2] for v in everything)) == len(everything)


def test_alleles_of_mapped_reads_hold_the_consensus_proposals():
    """tests/pileup_cases.planted() mapped by the real mapper: the alleles at min_fraction 0.5 contain every variant of
    Consensus.proposals() that has no more than max_alt letters, and the tables are as they were."""
    need_gpu()
    from sloika_amd import genome, polish
    from tests import pileup_cases
    case = pileup_cases.planted()
    idx = genome.Index([(pileup_cases.CONTIG, case['genome'])], k=8, bin_width=512)
    res, strand, info, ops = idx.map(case['reads'], ops=True)
    pile, cons = genome.pileup(idx, res, strand, info, ops)
    before = (pile.counts().copy(), pile.insertions().copy(), cons.proposals())
    for klen in (3, 5):
        props = cons.proposals(polish.max_alt(klen))
        got = pile.alleles(klen, min_fraction=0.5).rows()
        assert len(props) >= 1 and set(props) <= set(got), sorted(set(props) - set(got))
        want = gr.alleles(before[0], before[1], case['genome'], [0, len(case['genome'])], 0, klen, 3, 2, 500, 8)[0]
        assert got == [(pileup_cases.CONTIG,) + v[1:] for v in want]
        assert len(pile.alleles(klen, min_fraction=0.2)) >= len(got)
    assert np.array_equal(pile.counts(), before[0]) and np.array_equal(pile.insertions(), before[1])
    assert pile.consensus().proposals() == before[2]
    with pytest.raises(ValueError):
        pile.alleles(3, min_fraction=0.0)
    with pytest.raises(ValueError):
        pile.alleles(3, max_del=0)


# ---- 2: likelihoods ------------------------------------------------------------------------------------------------------------------

def likelihood_case():
    """Hand-made candidates of 9 variants over 210 reads: variant 0 has none, 1 one, 2 two, 3 two hundred; 4 the differences 0,
    +-1e-300, +-40 and +-800 (the small ones against scores of 0); 5 a -inf among finite values; 6 a NaN in ll_edit; 7 a NaN in its
    read's score; 8 every read preferring it by about 3."""
    rng = np.random.default_rng(19)
    nread = 210
    score = -rng.uniform(200.0, 300.0, size=nread)
    score[:3] = 0.0
    score[209] = np.nan
    read, var, ll = [], [], []

    def add(v, r, d):
        read.append(r)
        var.append(v)
        ll.append(score[r] + d if np.isfinite(score[r]) else -250.0)

    add(1, 5, -2.25)
    add(2, 4, 1.5)
    add(2, 9, -0.75)
    for r in range(5, 205):
        add(3, r, float(rng.normal(0.0, 6.0)))
    for r, d in enumerate((0.0, 1e-300, -1e-300)):
        add(4, r, d)
    for r, d in zip(range(10, 14), (40.0, -40.0, 800.0, -800.0)):
        add(4, r, d)
    for r in range(20, 26):
        add(5, r, -np.inf if r == 22 else float(rng.normal(1.0, 2.0)))
    for r in range(30, 34):
        add(6, r, np.nan if r == 31 else 2.0)
    for r in (40, 209, 41):
        add(7, r, 1.0)
    for r in range(50, 80):
        add(8, r, float(rng.normal(3.0, 0.5)))
    return score, np.array(ll), np.array(read, dtype=np.int32), np.array(var, dtype=np.int32), 9


@pytest.mark.parametrize("scale", [1.0, 0.37])
def test_likelihoods_equal_the_model(scale):
    from sloika_amd import polish
    need_gpu()
    score, ll, read, var, V = likelihood_case()
    want, n_want, size = gr.genotype_sums(score, ll, read, var, V, scale)
    assert n_want.tolist() == [0, 1, 2, 200, 7, 5, 3, 2, 30]                         # (6 and 7: the finite pairs beside the NaN)
    run = lambda sel: polish.variant_genotype_likelihoods(dev(score), dev(ll[sel]), dev(read[sel]), dev(var[sel]), V, scale)    # noqa: E731
    everything = np.arange(len(ll))
    gl_d, n_d = run(everything)
    gl, n = gl_d.cpu().numpy(), n_d.cpu().numpy()
    assert gl.shape == (V, 3) and n.dtype == np.int32 and np.array_equal(n, n_want)
    nan = np.isnan(np.asarray(want, dtype=np.float64)).any(axis=1)
    assert nan.tolist() == [False] * 6 + [True, True, False]
    assert np.array_equal(np.isnan(gl), np.repeat(nan[:, None], 3, axis=1))            # NaN exactly where the model has it
    assert (gl[~nan, 0] == 0.0).all() and not np.signbit(gl[~nan, 0]).any()
    assert n[0] == 0 and not gl[0].any()                                                # no read scored it: zeros
    assert n[5] == 5                                                                    # the -inf is not counted
    eg = gr.e_gt(n_want, size)[~nan]
    bound = 4.0 * gr.e_gt(n_want, size)
    err = np.abs((gl[~nan, 1].astype(gr.LD) - want[~nan, 1]).astype(np.float64))
    ratio = float((err[eg > 0] / eg[eg > 0]).max())
    print("genotype likelihoods at scale %g: gl1 %s, largest |device - model| / E_gt = %.4f" % (scale, np.round(gl[~nan, 1], 4).tolist(), ratio))
    assert (err <= bound[~nan]).all()
    err2 = np.abs((gl[~nan, 2].astype(gr.LD) - want[~nan, 2]).astype(np.float64))
    assert (err2 <= bound[~nan]).all()
    assert gl[4, 1] > 700 * scale and gl[8, 1] > 0 and gl[8, 2] > gl[8, 1] and gl[1, 1] < 0
    if scale == 1.0:
        minus = dev(np.zeros(len(score), dtype=np.int32))
        tables = polish.sum_variant_gains(dev(score), dev(ll), dev(read), dev(var), minus, V)
        assert np.array_equal(bits(np.nan_to_num(tables[0].cpu().numpy(), nan=-1.0)), bits(np.nan_to_num(gl[:, 2], nan=-1.0)))
        assert np.array_equal(np.isnan(tables[0].cpu().numpy()), nan) and np.array_equal(tables[1].cpu().numpy(), n)
    # the bits do not depend on the candidates' order in memory: reversed read-block order, and a shuffle
    rev = np.concatenate([np.flatnonzero(read == r) for r in range(len(score) - 1, -1, -1)])
    for sel in (rev, np.random.RandomState(3).permutation(len(ll))):
        g2, n2 = run(sel)
        assert np.array_equal(bits(np.nan_to_num(g2.cpu().numpy(), nan=-1.0)), bits(np.nan_to_num(gl, nan=-1.0)))
        assert np.array_equal(n2.cpu().numpy(), n)
    with pytest.raises(ValueError):
        polish.variant_genotype_likelihoods(dev(score), dev(ll), dev(read), dev(var), V, 0.0)
    with pytest.raises(ValueError):
        polish.variant_genotype_likelihoods(dev(score), dev(ll), dev(read), dev(var), V, float('nan'))


# ---- 3: a planted diploid sample -----------------------------------------------------------------------------------------------------

def called(sample):
    from sloika_amd import decode
    post, steps = dev(sample["post"]), dev(sample["steps"])
    _, paths, lens, move_row, _, _ = decode.viterbi_marginals_batch(post, sample["k"], min_prob=MIN_PROB, lengths=steps)
    return post, steps, paths, lens, move_row


@pytest.fixture(scope="module")
def diploid():
    need_gpu()
    from sloika_amd import genome, polish
    s = gr.planted_diploid()
    call = called(s)
    idx = genome.Index([("ref", s["reference"])], k=14)
    res, strand, info, _, ops = idx.map_paths(call[2], call[3], s["k"], ops=True)
    post, steps, paths, lens, move_row = call
    calls = polish.call_variants(post, steps, paths, lens, move_row, idx, res, strand, info, ops, s["k"], min_fraction=0.2, width=256)
    return dict(sample=s, call=call, idx=idx, mapping=(res, strand, info, ops), calls=calls)


def model_candidates(text, k, call, host_post, mapping, variants, width=256):
    """The CPU model on the device's mapping of the calls (tests/test_gpu_polish_variants.model_variants' construction): windows and
    centre lines of tests/polish_genome_ref.py, candidates of tests/polish_variants_ref.py, float64 scores of
    tests/rescore_band_ref.evaluate.  -> (score per read, ll, read and variant per candidate, in the caller's numbering)"""
    from tests import rescore_band_ref as rb
    res, strand, info, ops = mapping
    paths, lens, move_row, steps = (v.cpu().numpy() for v in call)
    qlen = ops.query_lengths()
    rows_sorted, order = pv.sort_variants(variants)
    score = np.full(len(steps), np.nan)
    reads, var, lls = [], [], []
    for r in range(len(steps)):
        if info['contig'][r] < 0:
            continue
        rlen = int(info['window_end'][r] - info['window_start'][r])
        codes = ops.codes(r)
        st, span, win, cen = pg.read_window(paths[r, :lens[r]].tolist(), move_row[r], int(steps[r]), int(qlen[r]), ops.ldq, ops.rows[r], codes,
                                            len(codes), strand[r] == '-', int(info['window_start'][r]), 0, rlen, len(text), k,
                                            int(steps[r]) + 1)
        if st != pg.DONE:
            continue
        c = pv.variant_edits(text, [0, len(text)], [(0, win[0], win[1], strand[r] == '-')], rows_sorted, k, 0, 2 * k)
        off = c["cand_new_off"]
        trip = [(int(a), int(d), c["cand_new"][off[i]:off[i + 1]]) for i, (a, d) in enumerate(zip(c["cand_start"], c["cand_ndel"]))]
        sc, ll = rb.evaluate(host_post[span[0]:span[1], r, :], c["seq"], trip, rb.band_lo(cen, len(c["seq"]), width), width, 0, np.float64)
        score[r] = float(sc)
        reads += [r] * len(trip)
        var += [order[v] for v in c["cand_var"]]
        lls += [float(v) for v in ll]
    return score, np.array(lls), np.array(reads, dtype=np.int32), np.array(var, dtype=np.int32)


def test_planted_diploid(diploid):
    """Two haplotypes under 24 planted reads on both strands, decoded and mapped by the real decoder and mapper.  The alleles at
    min_fraction 0.2 contain the five planted variants; the two both haplotypes carry are 1/1 and the three of haplotype B alone 0/1,
    each with GQ >= 20; gt equals the CPU model's for every variant whose top two model posteriors differ by more than 8 E_gt (no
    planted variant and at most 1 in 100 of all may fall under that); the 1/1 records applied to the reference give haplotype A and
    every PASS non-reference record haplotype B."""
    from sloika_amd import genome, polish
    s, calls, idx = diploid["sample"], diploid["calls"], diploid["idx"]
    ref, k = s["reference"], s["k"]
    rows = calls.variants.rows()
    assert calls.rescored.status.tolist() == [polish.READ_DONE] * 24 + [polish.READ_UNMAPPED]
    planted = [("ref",) + v for v in s["planted"]]
    assert set(planted) <= set(rows), sorted(set(planted) - set(rows))
    where = [rows.index(v) for v in planted]
    gl, n = calls.gl.cpu().numpy(), calls.n.cpu().numpy()
    print("planted diploid: %d proposed; planted %s -> gt %s gq %s n %s pro %s gl %s" % (
        len(rows), planted, calls.gt[where].tolist(), calls.gq[where].tolist(), n[where].tolist(), calls.pro[where].tolist(),
        np.round(gl[where], 2).tolist()))
    for v in range(len(rows)):
        if v not in where and calls.gt[v] > 0:
            print("  a call beside the planted ones: %r gt %d gq %d gl %s, read gains %s" % (
                rows[v], calls.gt[v], calls.gq[v], np.round(gl[v], 2).tolist(), np.round(calls.rescored.read_gains(v)[1], 2).tolist()))
    assert calls.gt[where].tolist() == s["genotypes"] and (calls.gq[where] >= 20).all()
    assert np.array_equal(n, calls.support) and np.array_equal(bits(gl[:, 2]), bits(calls.rescored.gain.cpu().numpy()))
    # the CPU model on the same mapping
    score, lls, reads, var = model_candidates(ref, k, diploid["call"][2:] + (diploid["call"][1],), s["post"], diploid["mapping"],
                                              [(0,) + v[1:] for v in rows])
    m_gl, m_n, size = gr.genotype_sums(score, lls, reads, var, len(rows))
    assert np.array_equal(m_n, n)
    prior = gr.prior_of()
    eg = gr.e_gt(m_n, size)
    model = [gr.call([float(x) for x in m_gl[v]], int(m_n[v]), prior) for v in range(len(rows))]
    clear = [v for v in range(len(rows)) if model[v][4] is None or model[v][4] > 8.0 * eg[v]]
    assert set(where) <= set(clear) and 100 * (len(rows) - len(clear)) <= len(rows)
    assert [model[v][0] for v in where] == s["genotypes"] and all(model[v][1] >= 20 for v in where)    # the model alone satisfies both
    assert [int(calls.gt[v]) for v in clear] == [model[v][0] for v in clear]
    # the records
    text = calls.vcf('diploid')
    assert text == genome.vcf_text(idx, calls.rows(), 'diploid', min_gq=20)
    assert gr.apply_vcf({"ref": ref}, text, lambda f, gt: gt == '1/1') == {"ref": s["hap_a"]}
    assert gr.apply_vcf({"ref": ref}, text) == {"ref": s["hap_b"]}
    assert [r[:4] for r in calls.rows(min_gq=20)] == [v for v in rows if v in planted]


def nine(g):
    return [t.cpu().numpy() for t in (g.gain, g.support, g.pro, g.gain_strand, g.support_strand, g.pro_strand)]


def test_unchanged_paths(diploid):
    """rescore_variants beside call_variants(variants=<the same list>): the nine sum tables of the list's variants are bit for bit the
    same, and a variant the pileup proposes as well is there once.  Consensus.proposals() and polish_genome() return the same values
    before and after the caller has run on their pileup and reads."""
    from sloika_amd import genome, polish
    s, idx = diploid["sample"], diploid["idx"]
    post, steps, paths, lens, move_row = diploid["call"]
    res, strand, info, ops = diploid["mapping"]
    k = s["k"]
    mine = [("ref", 100, 0, 'ACG'), ("ref",) + s["planted"][1], ("ref", 400, 3, 'T'), ("ref", 305, 1, '')]
    pile, cons = genome.pileup(idx, res, strand, info, ops)
    before = cons.proposals()
    polished = polish.polish_genome(post, steps, paths, lens, move_row, idx, k, width=256, max_rounds=1)
    want = polish.rescore_variants(post, steps, paths, lens, move_row, idx, res, strand, info, ops, k, mine, width=256)
    calls = polish.call_variants(post, steps, paths, lens, move_row, idx, res, strand, info, ops, k, width=256, variants=mine)
    rows = calls.variants.rows()
    assert len(rows) == len(set(rows)) == len(diploid["calls"].variants.rows()) + 3
    at = [rows.index(v) for v in mine]
    for a, b in zip(nine(calls.rescored), nine(want)):
        assert a[at].tobytes() == b.tobytes()
    assert genome.pileup(idx, res, strand, info, ops)[1].proposals() == before == cons.proposals()
    again = polish.polish_genome(post, steps, paths, lens, move_row, idx, k, width=256, max_rounds=1)
    assert [tuple(p) for p in again[0]] == [tuple(p) for p in polished[0]]
    assert again[1].gain.cpu().numpy().tobytes() == polished[1].gain.cpu().numpy().tobytes()
    # 'repeats' beside the alleles: the repeat family's own deletion of one AC unit is the planted one, and is there once
    more = polish.call_variants(post, steps, paths, lens, move_row, idx, res, strand, info, ops, k, width=256, variants='repeats')
    rows = more.variants.rows()
    assert len(rows) == len(set(rows)) > len(diploid["calls"].variants.rows())
    assert more.gt[rows.index(("ref",) + s["planted"][1])] == 1


def test_basecaller_call_variants():
    """Two synthetic reads through a small built model, the genome a stretch of each read's own call with a letter changed:
    Basecaller.call_variants is polish.call_variants on the posterior, the calls and the mapping of the same reads, bit for bit, and
    its vcf() is genome.vcf_text of its rows."""
    need_gpu()
    from sloika_amd import bio, genome, models, pipeline, polish
    net = models.randomise_zero_layers(models.build_model("raw_0.98_rgrgr", klen=5, sd=0.5, seed=7))
    bc = pipeline.Basecaller(net, kmer_len=5, skip=0.0)
    base = pipeline.synthetic_chunks(2, chunk_len=3000, seed=21)
    reads = [base[0], base[1][:2200], base[0], base[0]]
    _, paths, lens, move_row, _, _, _ = bc.call_reads_qual(reads)
    calls = bio.paths_to_bases(paths, lens, 5)
    a = calls[0][20:144]
    a = a[:60] + 'ACGT'[('ACGT'.index(a[60]) + 1) % 4] + a[61:]
    idx = genome.Index([("a", a), ("b", calls[1][10:94])], k=14)
    variants = [("a", 40, 2, ''), ("b", 30, 0, 'ACGT'), ("a", 70, 3, 'T')]
    kw = dict(min_depth=2, min_fraction=0.3, het=0.01, scale=0.5, variants=variants, width=256)
    got = bc.call_variants(reads, idx, **kw)
    padded, ns = bc._padded_reads(reads, (0, 0), 0.0, None, "test")
    post, steps = bc._read_posteriors(padded, ns)
    res, strand, info, _, ops = idx.map_paths(paths, lens, 5, ops=True)
    want = polish.call_variants(post, steps, paths, lens, move_row, idx, res, strand, info, ops, 5, blank=0, min_prob=bc.min_prob, **kw)
    rows = got.variants.rows()
    assert rows == want.variants.rows() and set(variants) <= set(rows) and ("a", 60, 1, calls[0][80]) in rows
    raw = lambda t: t.cpu().numpy().tobytes()                        # noqa: E731
    assert raw(got.gl) == raw(want.gl) and raw(got.n) == raw(want.n)
    for name in ("gt", "gq", "pl", "qual", "support", "pro", "support_strand", "pro_strand"):
        assert getattr(got, name).tobytes() == getattr(want, name).tobytes(), name
    for name in polish.VARIANT_TABLES + ("score", "ll_edit", "cand_var", "cand_read"):
        assert raw(getattr(got.rescored, name)) == raw(getattr(want.rescored, name)), name
    assert got.scale == 0.5 and got.prior == polish.genotype_prior(0.01)
    assert got.vcf() == genome.vcf_text(idx, got.rows(), 'sample', min_gq=20) and got.vcf().startswith("##fileformat=VCFv4.2\n")
    assert got.vcf(all_records=True).count("\n") == 11 + len(rows)
