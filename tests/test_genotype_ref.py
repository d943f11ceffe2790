"""The variant caller without a GPU: the plain-loop model of tests/genotype_ref.py on hand-checked tables, the host half of
sloika_amd.polish.genotypes against the extended-precision posterior, and the VCF text of hand-written cases as exact strings
(design/genotypes.md section 1)."""
import types

import numpy as np
import pytest

from tests import genotype_ref as gr


# ---- the model on hand-checked tables --------------------------------------------------------------------------------------------------

def hand_tables():
    genome = "ACGTACGTAC"
    counts = np.zeros((10, 8), dtype=np.int32)
    ins = np.zeros((10, 2, 5), dtype=np.int32)
    for t, ch in enumerate(genome):
        counts[t, 'ACGT'.index(ch)] = 10
        counts[t, 7] = 10
    counts[2, 2], counts[2, 0], counts[2, 1] = 7, 2, 1                # G: 2 of 10 A (exactly 200 per mille), 1 C (below min_count)
    for t in (4, 5, 7, 8, 9):
        counts[t, 'ACGT'.index(genome[t])], counts[t, 5] = 5, 5       # two deletion runs: 4-5 and 7-9
    ins[0, 0] = [0, 0, 3, 0, 0]                                       # behind letter 0: G three times, then a letter seen once
    ins[0, 1] = [1, 0, 0, 0, 0]
    return genome, counts, ins


def test_model_on_hand_checked_tables():
    genome, counts, ins = hand_tables()
    got, nprop, nalt, skipped = gr.alleles(counts, ins, genome, [0, 10], 0, 3, min_depth=3, min_count=2, permille=200, max_del=2)
    assert got == [(0, 1, 0, 'G'), (0, 2, 1, 'A'), (0, 4, 2, '')]
    assert nprop == [0, 1, 1, 0, 1, 0, 0, 0, 0, 0] and nalt == [0, 1, 1, 0, 0, 0, 0, 0, 0, 0]
    assert skipped == [0, 0, 0, 0, 0, 0, 0, gr.SKIP_DEL, 0, 0]
    # a longer run is proposed once max_del allows it; 2 of 11 is below 200 per mille; a depth below min_depth proposes nothing
    assert gr.alleles(counts, ins, genome, [0, 10], 0, 3, max_del=3)[0][-1] == (0, 7, 3, '')
    counts[2, 2] = 8
    assert (0, 2, 1, 'A') not in gr.alleles(counts, ins, genome, [0, 10], 0, 3)[0]
    assert gr.alleles(counts, ins, genome, [0, 10], 0, 3, min_depth=11)[0] == [] and counts[0, 7] == 10
    assert (0, 1, 0, 'G') not in gr.alleles(counts, ins, genome, [0, 10], 0, 3, min_count=4)[0]
    # two contigs: the run 4-5 is cut at the boundary, and the insertion behind letter 0 stays; behind a contig's last letter none
    ins[4, 0] = [0, 0, 0, 6, 0]
    two = gr.alleles(counts, ins, genome, [0, 5, 10], 0, 3, max_del=3)[0]
    assert (0, 4, 1, '') in two and (5, 0, 1, '') in two and (5, 2, 3, '') in two and not [v for v in two if v[2] == 0 and v[0] == 5]
    assert (0, 5, 0, 'T') in gr.alleles(counts, ins, genome, [0, 10], 0, 3, max_del=3)[0]
    # a region whose lo cuts the run 7-9: position 8 starts what is left of it
    part = gr.alleles(counts[8:], ins[8:], genome, [0, 10], 8, 3)[0]
    assert part == [(0, 8, 2, '')]
    # a reference N proposes nothing and voids the run it stands in
    other = genome[:5] + 'N' + genome[6:]
    assert not [v for v in gr.alleles(counts, ins, other, [0, 10], 0, 3, max_del=3)[0] if v[1] in (4, 5)]
    # an insertion longer than max_alt(5) = 4 letters is skipped
    long_ins = np.zeros((10, 5, 5), dtype=np.int32)
    long_ins[0, :, 1] = 4
    out, _, _, skip = gr.alleles(counts, long_ins, genome, [0, 10], 0, 5)
    assert skip[1] == gr.SKIP_INS and not [v for v in out if v[2] == 0]
    assert (0, 1, 0, 'CCCCC') in gr.alleles(counts, long_ins, genome, [0, 10], 0, 3)[0]


def test_planted_diploid_is_what_it_says():
    s = gr.planted_diploid()
    ref, a, b = s["reference"], s["hap_a"], s["hap_b"]
    assert len(ref) == 600 and ref[150:162] == 'AC' * 6 and len(a) == 599 and len(b) == 599
    pos = sorted(p for p, _, _ in s["planted"])
    assert min(np.diff(pos)) >= 20 and len(s["texts"]) == 25 and s["post"].shape[1] == 25
    assert [g for g in s["genotypes"]] == [2, 1, 1, 2, 1]

    def spell(which):
        t = ref
        for p, nd, alt in sorted(which, reverse=True):
            t = t[:p] + alt + t[p + nd:]
        return t
    assert a == spell([v for v, g in zip(s["planted"], s["genotypes"]) if g == 2]) and b == spell(s["planted"]) and a != b != ref
    assert s["texts"][0] == a[0:300] and s["texts"][12] == gr.revcomp(b[0:300]) and s["texts"][13] == b[40:360]


# ---- the host half of polish.genotypes ---------------------------------------------------------------------------------------------------

GL_CASES = [(0.0, 0.0, 0.0), (0.0, -3.0, -9.0), (0.0, 12.5, 3.0), (0.0, 40.0, 95.0), (0.0, -745.0, -1490.0), (0.0, 745.0, 1490.0),
            (0.0, -800.0, -1600.0), (0.0, 800.0, 790.0), (0.0, 5000.0, 12000.0), (0.0, 1e-300, -1e-300), (0.0, 6.5, 6.5),
            (0.0, 0.7, -2.0), (0.0, 25.0, 26.0), (np.nan, np.nan, np.nan), (0.0, 3.0, 1.0)]
N_CASES = [4, 7, 9, 30, 12, 12, 20, 20, 64, 1, 3, 2, 8, 5, 0]


@pytest.mark.parametrize("het,prior", [(1e-3, None), (0.01, None), (1e-3, (1.0 / 3, 1.0 / 3, 1.0 / 3)), (1e-3, (0.25, 0.5, 0.25))])
def test_call_equals_the_extended_precision_posterior(het, prior):
    """n = 0, NaN, exact ties (equal likelihoods under a flat prior), differences of 745 and beyond: gt, GQ, PL and QUAL are the model's."""
    from sloika_amd import polish
    p = polish.genotype_prior(het, prior)
    assert p == (gr.prior_of(het) if prior is None else prior)
    gt, gq, pl, qual = polish.call_genotypes(np.array(GL_CASES), np.array(N_CASES), het=het, prior=prior)
    for v, (gl, n) in enumerate(zip(GL_CASES, N_CASES)):
        want = gr.call(gl, n, p)
        assert (int(gt[v]), int(gq[v]), tuple(int(x) for x in pl[v]), float(qual[v])) == want[:4], (v, gl, want)
    assert gt[13] == -1 and gt[14] == -1 and qual[14] == 0.0 and gq[13] == 0
    if prior is not None and prior[0] == prior[1] == prior[2]:
        assert gt[0] == 0 and gq[0] == 0 and gt[10] == 1 and gq[10] == 0           # ties go to the lower index
    if prior is None:
        assert gt[5] == 2 and gq[5] == 99 and qual[5] == 999.0 and pl[5].tolist() == [999, 999, 0]
        assert gt[4] == 0 and gq[4] == 99 and qual[4] == 0.0 and pl[4].tolist() == [0, 999, 999]
    assert np.isfinite(qual).all() and not np.signbit(qual).any()


# ---- VCF text ----------------------------------------------------------------------------------------------------------------------------

def fake_index():
    import torch
    contigs = [("c1", "ACGTACGT"), ("c2", "GGCATT")]
    text = ''.join(s for _, s in contigs)
    return types.SimpleNamespace(names=[n for n, _ in contigs], offsets=np.array([0, 8, 14], dtype=np.int64), G=14,
                                 lengths=np.array([8, 6]), genome=torch.from_numpy(np.frombuffer(text.encode(), dtype=np.uint8).copy()))


HEADER = ('##fileformat=VCFv4.2\n##source=sloika_amd\n##contig=<ID=c1,length=8>\n##contig=<ID=c2,length=6>\n'
          '##FILTER=<ID=LowGQ,Description="Genotype quality below 20">\n'
          '##FORMAT=<ID=GT,Number=1,Type=String,Description="Genotype">\n'
          '##FORMAT=<ID=GQ,Number=1,Type=Integer,Description="Genotype quality">\n'
          '##FORMAT=<ID=DP,Number=1,Type=Integer,Description="Reads whose signal scored the variant">\n'
          '##FORMAT=<ID=AD,Number=R,Type=Integer,Description="Reads whose signal prefers the reference, the variant">\n'
          '##FORMAT=<ID=PL,Number=G,Type=Integer,Description="Phred-scaled genotype likelihoods, not calibrated">\n'
          '#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tNA1\n')


def test_vcf_text_of_hand_written_cases():
    from sloika_amd import genome, polish
    C = polish.VariantCall
    rows = [C("c2", 3, 2, "G", 1, 40, 10, (5, 5), (60, 0, 90), 58.2),          # a replacement
            C("c2", 0, 2, "", 2, 99, 9, (0, 9), (400, 30, 0), 999.0),          # a deletion at pos 0: the base behind
            C("c1", 8, 0, "C", 1, 25, 8, (4, 4), (33, 0, 47), 30.0),           # an insertion at the contig's end
            C("c1", 2, 1, "T", 2, 5, 3, (1, 2), (20, 2, 0), 7.25),             # a SNV, LowGQ
            C("c1", 0, 0, "TT", 1, 20, 6, (3, 3), (25, 0, 31), 21.04),         # an insertion at pos 0, GQ exactly min_gq
            C("c1", 2, 1, "A", 0, 60, 6, (6, 0), (0, 18, 200), 0.0),           # 0/0 at the SNV's POS: stays behind it
            C("c1", 5, 1, "", -1, 0, 0, (0, 0), (0, 0, 0), 0.0)]               # ./.: a deletion with the base in front
    want = HEADER + ("c1\t1\t.\tA\tTTA\t21.0\tPASS\t.\tGT:GQ:DP:AD:PL\t0/1:20:6:3,3:25,0,31\n"
                     "c1\t3\t.\tG\tT\t7.2\tLowGQ\t.\tGT:GQ:DP:AD:PL\t1/1:5:3:1,2:20,2,0\n"
                     "c1\t3\t.\tG\tA\t0.0\tPASS\t.\tGT:GQ:DP:AD:PL\t0/0:60:6:6,0:0,18,200\n"
                     "c1\t5\t.\tAC\tA\t0.0\tLowGQ\t.\tGT:GQ:DP:AD:PL\t./.:0:0:0,0:0,0,0\n"
                     "c1\t8\t.\tT\tTC\t30.0\tPASS\t.\tGT:GQ:DP:AD:PL\t0/1:25:8:4,4:33,0,47\n"
                     "c2\t1\t.\tGGC\tC\t999.0\tPASS\t.\tGT:GQ:DP:AD:PL\t1/1:99:9:0,9:400,30,0\n"
                     "c2\t4\t.\tAT\tG\t58.2\tPASS\t.\tGT:GQ:DP:AD:PL\t0/1:40:10:5,5:60,0,90\n")
    ix = fake_index()
    assert genome.vcf_text(ix, rows, 'NA1', min_gq=20) == want
    assert genome.vcf_text(ix, [], 'NA1') == HEADER
    for row in rows:
        text = "ACGTACGT" if row.contig == "c1" else "GGCATT"
        assert genome.vcf_record(text, row.pos, row.ndel, row.alt) == gr.vcf_record(text, row.pos, row.ndel, row.alt)
    with pytest.raises(ValueError):
        genome.vcf_text(ix, [C("c3", 0, 1, "A", 1, 30, 3, (1, 2), (9, 0, 9), 9.0)], 'NA1')
    with pytest.raises(ValueError):
        genome.vcf_record("ACG", 0, 3, "")
    # the helper applies what the text says
    ref = {"c1": "ACGTACGT", "c2": "GGCATT"}
    assert gr.apply_vcf(ref, want) == {"c1": "TTACGTACGTC", "c2": "CGT"}
    assert gr.apply_vcf(ref, want, lambda f, gt: gt == '1/1') == {"c1": "ACTTACGT", "c2": "CATT"}


def test_variant_calls_rows_and_all_records():
    """VariantCalls over a hand-made rescoring: rows() filters by GQ and reference calls, vcf() is vcf_text of its rows, and 0/0 and
    ./. records are written with all_records alone."""
    import torch
    from sloika_amd import genome, polish
    ix = fake_index()
    rows = [("c2", 3, 2, "G"), ("c1", 2, 1, "T"), ("c1", 5, 1, ""), ("c1", 0, 0, "TT")]
    vs = types.SimpleNamespace(index=ix, rows=lambda: list(rows))
    t = lambda a, dt: torch.from_numpy(np.array(a, dtype=dt))                                  # noqa: E731
    res = types.SimpleNamespace(variants=vs, support=t([10, 6, 0, 2], np.int32), pro=t([5, 0, 0, 2], np.int32),
                                support_strand=t([[5, 5], [3, 3], [0, 0], [1, 1]], np.int32),
                                pro_strand=t([[2, 3], [0, 0], [0, 0], [1, 1]], np.int32))
    gl = np.array([[0.0, 30.0, 10.0], [0.0, -12.0, -40.0], [0.0, 0.0, 0.0], [0.0, 9.0, 7.0]])
    n = np.array([10, 6, 0, 2], dtype=np.int32)
    prior = polish.genotype_prior()
    gt, gq, pl, qual = polish.call_genotypes(gl, n, prior=prior)
    assert gt.tolist() == [1, 0, -1, 1] and gq[3] < 20 <= gq[0]
    calls = polish.VariantCalls(res, t(gl, np.float64), t(n, np.int32), gt, gq, pl, qual, prior, 1.0)
    assert [r[:4] for r in calls.rows()] == [rows[0], rows[3]] and [r[:4] for r in calls.rows(min_gq=20)] == [rows[0]]
    assert [r[:4] for r in calls.rows(nonref=False)] == rows and calls.rows()[0].ad == (5, 5) and calls.rows()[0].dp == 10
    text = calls.vcf('NA1')
    assert text == genome.vcf_text(ix, calls.rows(), 'NA1', min_gq=20)
    body = [ln.split('\t') for ln in text.splitlines() if not ln.startswith('#')]
    assert [(f[0], f[1], f[6], f[9][:3]) for f in body] == [("c1", "1", "LowGQ", "0/1"), ("c2", "4", "PASS", "0/1")]
    every = [ln.split('\t') for ln in calls.vcf('NA1', all_records=True).splitlines() if not ln.startswith('#')]
    assert [(f[0], f[1], f[9][:3]) for f in every] == [("c1", "1", "0/1"), ("c1", "3", "0/0"), ("c1", "5", "./."), ("c2", "4", "0/1")]
