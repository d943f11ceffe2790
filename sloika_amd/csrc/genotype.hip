// genotype.hip -- a variant caller on the chain call -> map -> pileup -> rescore_variants (design/genotypes.md; the quantities are
// defined in its section 1 and restated as plain loops in tests/genotype_ref.py).  Two things: the alleles a pileup's own disagreeing
// reads propose, as a sorted variant list in polish_variants.hip's layout, and the genotype log-likelihoods of proposed variants from the
// candidates the scoring entry returned.  The contig search, the base digit and the pieces of the sorted candidate list are
// genome_edits.h's, shared with polish_genome.hip and polish_variants.hip.
//
// Integer kernels but the last; no LDS, no MFMA, no floating-point atomics.  Every input is device data and is NOT trusted: no loop
// bound and no address depends on a value that has not been checked in the same kernel.
//   pileup_alleles_count_kernel  one thread per packed position: the number of variants it proposes and of their alt letters, and why
//                                it proposed nothing where it would have (skipped).
//   pileup_alleles_emit_kernel   one thread per packed position, the same walk again: writes its variants behind the prefix sums when
//                                they are its own counts.
//   variant_genotypes_kernel     one thread per candidate of the sorted list; the head of a segment of equal variants walks it in read
//                                order and writes the three log-likelihoods and the number of reads of the variant.
#include "genome_edits.h"

#define GT_MAX_INS 16              // genome.MAX_INS: the S of a pileup
#define GT_MAX_DEL (1 << 20)

// ---- 1. alleles of a pileup ----------------------------------------------------------------------------------------------------------

struct gt_rule {
    int S, max_alt, min_depth, min_count, permille, max_del;
    __device__ __forceinline__ bool pass(long long n, long long d) const
    {
        return n >= min_count && 1000ll * n >= (long long)permille * d && d >= min_depth;
    }
};

// the depth of a row of counts: entries 0 .. 5 (int32 each: the sum stays far inside int64)
__device__ __forceinline__ long long gt_depth(const int32_t *__restrict__ row)
{
    long long d = 0;
    for (int x = 0; x < 6; x++) d += row[x];
    return d;
}

// does the deletion count of table row t pass?
__device__ __forceinline__ bool gt_deleted(const gt_rule &R, const int32_t *__restrict__ counts, long long t)
{
    return R.pass(counts[8 * t + 5], gt_depth(counts + 8 * t));
}

// What table row t (packed position lo + t) proposes.  EMIT false: -> (proposals, alt letters, skipped bits).  EMIT true: writes them from
// variant `vi` and alt letter `ai` on, in the order insertion, substitutions by ascending class, deletion.
template <bool EMIT>
__device__ __forceinline__ void gt_propose(const gt_rule &R, const int32_t *__restrict__ counts, const int32_t *__restrict__ ins,
                                           const uint8_t *__restrict__ genome, long long G, const int64_t *__restrict__ contig_off,
                                           int ncontig, long long lo, long long P, long long t, long long *nprop, long long *nalt,
                                           int *skipped, long long vi, long long ai, int64_t *var_off, int64_t *var_pos,
                                           int32_t *var_ndel, int64_t *var_alt_off, uint8_t *var_alt)
{
    *nprop = 0;
    *nalt = 0;
    *skipped = 0;
    const long long g = lo + t;
    const int ci = ge_find(contig_off, ncontig, g);
    const long long c0 = contig_off[ci], c1 = contig_off[ci + 1];
    if (c0 < 0 || c0 > g || c1 <= g || c1 > G) return;            // (the table is device data: g lies in no contig it names)
    const int r = ge_digit(genome[g]);
    if (r < 0) return;
    const long long q = g - c0;
    const int32_t *row = counts + 8 * t;
    const long long depth = gt_depth(row);
    long long np = 0, na = 0;
    int skip = 0;
    // the insertion in front: the letters behind the row before, when that row is the letter before in this contig
    if (t >= 1 && g - 1 >= c0) {
        const int32_t *slot = ins + (t - 1) * R.S * 5;
        const long long span = counts[8 * (t - 1) + 7];
        int m = 0;
        unsigned letters = 0;                                     // two bits per letter: S <= 16
        for (int k = 0; k < R.S; k++) {
            long long n = 0, best = 0;
            int arg = 0;
            for (int x = 0; x < 5; x++) n += slot[5 * k + x];
            for (int x = 0; x < 4; x++)
                if (slot[5 * k + x] > best) {
                    best = slot[5 * k + x];
                    arg = x;
                }
            if (!R.pass(n, span) || best <= 0) break;
            letters |= (unsigned)arg << (2 * k);
            m++;
        }
        if (m > R.max_alt) skip |= SLK_ALLELES_SKIPPED_INS;
        else if (m >= 1) {
            if (EMIT) {
                var_off[vi] = c0;
                var_pos[vi] = q;
                var_ndel[vi] = 0;
                for (int k = 0; k < m; k++) var_alt[ai + k] = (uint8_t)"ACGT"[(letters >> (2 * k)) & 3];
                var_alt_off[vi + 1] = ai + m;
            }
            np = 1;
            na = m;
        }
    }
    for (int c = 0; c < 4; c++) {
        if (c == r || !R.pass(row[c], depth)) continue;
        if (EMIT) {
            var_off[vi + np] = c0;
            var_pos[vi + np] = q;
            var_ndel[vi + np] = 1;
            var_alt[ai + na] = (uint8_t)"ACGT"[c];
            var_alt_off[vi + np + 1] = ai + na + 1;
        }
        np++;
        na++;
    }
    // the deletion run that starts here: the row before is outside the table or the contig, or does not pass
    if (R.pass(row[5], depth) && !(t >= 1 && g - 1 >= c0 && gt_deleted(R, counts, t - 1))) {
        int L = 1;
        bool acgt = true;
        while (L <= R.max_del && t + L < P && g + L < c1 && gt_deleted(R, counts, t + L)) {
            acgt &= ge_digit(genome[g + L]) >= 0;
            L++;
        }
        if (L > R.max_del) skip |= SLK_ALLELES_SKIPPED_DEL;
        else if (acgt) {
            if (EMIT) {
                var_off[vi + np] = c0;
                var_pos[vi + np] = q;
                var_ndel[vi + np] = L;
                var_alt_off[vi + np + 1] = ai + na;
            }
            np++;
        }
    }
    *nprop = np;
    *nalt = na;
    *skipped = skip;
}

__global__ void __launch_bounds__(GE_THREADS) pileup_alleles_count_kernel(
    gt_rule R, const int32_t *__restrict__ counts, const int32_t *__restrict__ ins, const uint8_t *__restrict__ genome, long long G,
    const int64_t *__restrict__ contig_off, int ncontig, long long lo, long long P, int64_t *__restrict__ nprop,
    int64_t *__restrict__ nalt, int32_t *__restrict__ skipped)
{
    const long long t = (long long)blockIdx.x * GE_THREADS + threadIdx.x;
    if (t == 0) {
        nprop[0] = 0;
        nalt[0] = 0;
    }
    if (t >= P) return;
    long long np, na;
    int skip;
    gt_propose<false>(R, counts, ins, genome, G, contig_off, ncontig, lo, P, t, &np, &na, &skip, 0, 0, nullptr, nullptr, nullptr, nullptr,
                      nullptr);
    nprop[t + 1] = np;
    nalt[t + 1] = na;
    skipped[t] = skip;
}

__global__ void __launch_bounds__(GE_THREADS) pileup_alleles_emit_kernel(
    gt_rule R, const int32_t *__restrict__ counts, const int32_t *__restrict__ ins, const uint8_t *__restrict__ genome, long long G,
    const int64_t *__restrict__ contig_off, int ncontig, long long lo, long long P, const int64_t *__restrict__ prop_off,
    const int64_t *__restrict__ alt_off, long long V, long long A, int64_t *__restrict__ var_off, int64_t *__restrict__ var_pos,
    int32_t *__restrict__ var_ndel, int64_t *__restrict__ var_alt_off, uint8_t *__restrict__ var_alt)
{
    const long long t = (long long)blockIdx.x * GE_THREADS + threadIdx.x;
    if (t == 0) var_alt_off[0] = 0;
    if (t >= P) return;
    const long long vi = prop_off[t], ai = alt_off[t], nv = prop_off[t + 1] - vi, nl = alt_off[t + 1] - ai;
    if (vi < 0 || nv <= 0 || nv > V - vi || ai < 0 || nl < 0 || nl > A - ai) return;
    long long np, na;
    int skip;
    gt_propose<false>(R, counts, ins, genome, G, contig_off, ncontig, lo, P, t, &np, &na, &skip, 0, 0, nullptr, nullptr, nullptr, nullptr,
                      nullptr);
    if (np != nv || na != nl) return;                            // (offsets that are not this position's own counts are not followed)
    gt_propose<true>(R, counts, ins, genome, G, contig_off, ncontig, lo, P, t, &np, &na, &skip, vi, ai, var_off, var_pos, var_ndel,
                     var_alt_off, var_alt);
}

// ---- 2. genotype log-likelihoods -----------------------------------------------------------------------------------------------------

// order: the candidates sorted by (variant, read), the host's sort for variant_sum_gains_kernel.  The thread of a segment's first entry
// walks the segment: both sums are taken in read order whatever the launch's shape.  A read is a draw from one of the two haplotypes,
// so under 0/1 its likelihood ratio against 0/0 is 1/2 + 1/2 e^d; its log is taken as max(d, 0) + log1p(e^-|d|) - ln 2.
__global__ void __launch_bounds__(GE_THREADS) variant_genotypes_kernel(
    const double *__restrict__ score, int nread, const double *__restrict__ ll_edit, const int32_t *__restrict__ cand_read,
    const int32_t *__restrict__ cand_var, const int64_t *__restrict__ order, long long ncand, long long V, double scale,
    double *__restrict__ gl, int32_t *__restrict__ nscored)
{
    const long long i = (long long)blockIdx.x * GE_THREADS + threadIdx.x;
    if (i >= ncand) return;
    const long long ci = order[i];
    if (!ge_listed(ci, ncand)) return;
    const long long v = cand_var[ci];
    if (!ge_segment_head(order, ncand, i, cand_var, (int32_t)v)) return;
    if (v < 0 || v >= V) return;
    const double ln2 = 0.6931471805599453;
    double g1 = 0.0, g2 = 0.0;
    int cnt = 0;
    bool bad = false;
    for (long long x = i; x < ncand; x++) {
        const long long c = order[x];
        if (!ge_listed(c, ncand) || cand_var[c] != v) break;
        const int r = cand_read[c];
        const double l = ll_edit[c], s = r >= 0 && r < nread ? score[r] : __builtin_nan("");
        const int what = ge_classify(l, s);
        if (what == GE_PAIR_NAN) bad = true;
        else if (what == GE_PAIR_FINITE) {
            const double d = scale * (l - s);
            g1 += (fmax(d, 0.0) + log1p(exp(-fabs(d)))) - ln2;
            g2 += d;
            cnt++;
        }
    }
    gl[3 * v] = bad ? __builtin_nan("") : 0.0;
    gl[3 * v + 1] = bad ? __builtin_nan("") : g1;
    gl[3 * v + 2] = bad ? __builtin_nan("") : g2;
    nscored[v] = cnt;
}

// ---- entries -------------------------------------------------------------------------------------------------------------------------

static inline bool gt_make_rule(long G, int ncontig, int64_t lo, int64_t P, int max_ins, int klen, int min_depth, int min_count,
                                int permille, int max_del, gt_rule *R)
{
    if (G < 0 || ncontig < 1 || lo < 0 || P < 0 || lo > G || P > G - lo || !ge_klen(klen)) return false;
    if (max_ins < 1 || max_ins > GT_MAX_INS || min_depth < 1 || min_count < 1 || permille < 1 || permille > 1000 || max_del < 1 ||
        max_del > GT_MAX_DEL)
        return false;
    R->S = max_ins;
    R->max_alt = SLK_RESCORE_MAX_NEW - klen + 1;
    R->min_depth = min_depth;
    R->min_count = min_count;
    R->permille = permille;
    R->max_del = max_del;
    return true;
}

extern "C" int slk_pileup_alleles_count(const int32_t *counts, const int32_t *ins, const uint8_t *genome, long G,
                                        const int64_t *contig_off, int ncontig, int64_t lo, int64_t P, int max_ins, int kmer_len,
                                        int min_depth, int min_count, int permille, int max_del, int64_t *nprop, int64_t *nalt,
                                        int32_t *skipped, slk_stream_t stream)
{
    gt_rule R;
    if (!gt_make_rule(G, ncontig, lo, P, max_ins, kmer_len, min_depth, min_count, permille, max_del, &R) || !contig_off || !nprop || !nalt)
        return SLK_ERR_INVALID_ARG;
    if (P > 0 && (!counts || !ins || !genome || !skipped)) return SLK_ERR_INVALID_ARG;
    hipLaunchKernelGGL(pileup_alleles_count_kernel, dim3(ge_blocks(P > 0 ? P : 1)), dim3(GE_THREADS), 0, slk_stream(stream), R, counts, ins,
                       genome, (long long)G, contig_off, ncontig, (long long)lo, (long long)P, nprop, nalt, skipped);
    return slk_launch_status();
}

extern "C" int slk_pileup_alleles_emit(const int32_t *counts, const int32_t *ins, const uint8_t *genome, long G,
                                       const int64_t *contig_off, int ncontig, int64_t lo, int64_t P, int max_ins, int kmer_len,
                                       int min_depth, int min_count, int permille, int max_del, const int64_t *prop_off,
                                       const int64_t *alt_off, int64_t V, int64_t A, int64_t *var_off, int64_t *var_pos,
                                       int32_t *var_ndel, int64_t *var_alt_off, uint8_t *var_alt, slk_stream_t stream)
{
    gt_rule R;
    if (!gt_make_rule(G, ncontig, lo, P, max_ins, kmer_len, min_depth, min_count, permille, max_del, &R) || V < 0 || A < 0 ||
        !contig_off || !var_alt_off)
        return SLK_ERR_INVALID_ARG;
    if (V > 0 && (!counts || !ins || !genome || !prop_off || !alt_off || !var_off || !var_pos || !var_ndel)) return SLK_ERR_INVALID_ARG;
    if (A > 0 && !var_alt) return SLK_ERR_INVALID_ARG;
    hipLaunchKernelGGL(pileup_alleles_emit_kernel, dim3(ge_blocks(V > 0 && P > 0 ? P : 1)), dim3(GE_THREADS), 0, slk_stream(stream), R,
                       counts, ins, genome, (long long)G, contig_off, ncontig, (long long)lo, V > 0 ? (long long)P : 0ll, prop_off, alt_off,
                       (long long)V, (long long)A, var_off, var_pos, var_ndel, var_alt_off, var_alt);
    return slk_launch_status();
}

extern "C" int slk_variant_genotypes_f64(const double *score, int nread, const double *ll_edit, const int32_t *cand_read,
                                         const int32_t *cand_var, const int64_t *order, int64_t ncand, int64_t V, double scale, double *gl,
                                         int32_t *n, slk_stream_t stream)
{
    if (nread < 0 || ncand < 0 || V < 0 || !(scale > 0.0) || scale - scale != 0.0) return SLK_ERR_INVALID_ARG;
    if (ncand == 0 || V == 0) return SLK_OK;
    if (!score || !ll_edit || !cand_read || !cand_var || !order || !gl || !n) return SLK_ERR_INVALID_ARG;
    hipLaunchKernelGGL(variant_genotypes_kernel, dim3(ge_blocks(ncand)), dim3(GE_THREADS), 0, slk_stream(stream), score, nread, ll_edit,
                       cand_read, cand_var, order, (long long)ncand, (long long)V, scale, gl, n);
    return slk_launch_status();
}
