// polish_variants.hip -- proposed variants of any length put to the reads' signal (design/polish_variants.md; the quantities are defined
// in its section 1 and restated as plain loops in tests/polish_variants_ref.py).  The scoring kernels are f10b's, unchanged; this file
// makes their candidates from a sorted variant list, sums their answers per variant and strand, and proposes the repeat-unit family.
// The window, the edit as a replacement, its (start, ndel, new symbols) and the pieces of the sum kernel's walk are genome_edits.h's,
// shared with polish_genome.hip; this file keeps the variant list and its status, which variants a window has and where they sit in
// it, the nine sums of a variant and the repeat-unit family.
//
// Integer kernels but the sum; no LDS, no MFMA.  Every input is device data and is NOT trusted: no loop bound and no address depends
// on a value that has not been checked in the same kernel.
//   variant_status_kernel        one thread per variant: 0 or why it is refused.
//   variant_edits_count_kernel   one wave per window: the range of variants that start inside it by binary search in the sorted list,
//                                those that also fit at their far end counted 64 at a time with ballots.
//   variant_edits_emit_kernel    one wave per window, the same walk: a fitting variant's rank is a population count below its lane
//                                plus a running base; its lane writes the candidate (pair, start, ndel, variant, number of new symbols).
//   variant_edits_new_kernel     one thread per candidate: its new symbols, behind the prefix sum of their numbers.
//   variant_sum_gains_kernel     one thread per candidate of the sorted list; the head of a segment of equal variants walks it in read
//                                order and writes the nine values of the variant.  No floating-point atomics.
//   repeat_variants_*_kernel     one thread per packed position: the tracts that start there and what they propose.
#include "genome_edits.h"

#define PV_MAX_UNIT 4
#define PV_MAX_CHANGE 8

// the variant list as the entries take it
struct pv_list {
    const int64_t *off;        // [V] the packed position of the variant's contig
    const int64_t *pos;        // [V] within the contig
    const int32_t *ndel;       // [V]
    const int64_t *alt_off;    // [V + 1] into alt
    const uint8_t *alt;
    long long V, A;            // variants, letters of alt
    int max_alt;               // SLK_RESCORE_MAX_NEW - kmer_len + 1
};

// ---- 1. the variants themselves ------------------------------------------------------------------------------------------------------

__global__ void __launch_bounds__(GE_THREADS) variant_status_kernel(
    pv_list L, const uint8_t *__restrict__ genome, long long G, const int64_t *__restrict__ contig_off, int ncontig,
    int32_t *__restrict__ var_status)
{
    const long long v = (long long)blockIdx.x * GE_THREADS + threadIdx.x;
    if (v >= L.V) return;
    const long long off = L.off[v], pos = L.pos[v], a0 = L.alt_off[v], a1 = L.alt_off[v + 1];
    const int nd = L.ndel[v];
    // the contig: the last c with contig_off[c] <= off; the table is device data too (its entries are clamped, not followed)
    const int lo = ge_find(contig_off, ncontig, off);
    const long long c0 = contig_off[lo], c1 = contig_off[lo + 1];
    int st = SLK_VARIANT_OK;
    if (c0 != off || c0 < 0 || c1 < c0 || c1 > G) st = SLK_VARIANT_CONTIG;
    else if (nd < 0) st = SLK_VARIANT_NDEL;
    else if (pos < 0 || pos > c1 - c0 || nd > c1 - c0 - pos) st = SLK_VARIANT_SPAN;
    else if (a0 < 0 || a1 < a0 || a1 > L.A || a1 - a0 > L.max_alt) st = SLK_VARIANT_ALT;
    else if (nd + (a1 - a0) < 1) st = SLK_VARIANT_EMPTY;
    else if (nd == a1 - a0) {                                     // (at most max_alt letters)
        bool same = true;
        for (int x = 0; x < nd; x++) same &= genome[off + pos + x] == L.alt[a0 + x];
        if (same) st = SLK_VARIANT_SAME;
    }
    var_status[v] = st;
}

// ---- 2. candidates from variants -----------------------------------------------------------------------------------------------------

// the first v of the sorted list with (off[v], pos[v]) >= (o, p)
__device__ __forceinline__ long long pv_lower(const pv_list &L, long long o, long long p)
{
    long long lo = 0, hi = L.V;
    while (lo < hi) {
        const long long mid = lo + (hi - lo) / 2;
        const long long mo = L.off[mid];
        if (mo < o || (mo == o && L.pos[mid] < p)) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// Is variant v a candidate of window w?  Everything the emit and new kernels go on to use is checked here, whatever var_status says:
// the variant's span inside the window's margins (so inside the genome), its alt slice inside alt and short enough, and a k-mer left.
__device__ __forceinline__ bool pv_fits(const pv_list &L, const int32_t *__restrict__ var_status, long long v, const ge_win &w, int klen,
                                        int margin)
{
    if (v < 0 || v >= L.V || var_status[v] != SLK_VARIANT_OK || L.off[v] != w.off || w.n < klen) return false;
    const long long pos = L.pos[v], a0 = L.alt_off[v], a1 = L.alt_off[v + 1];
    const int nd = L.ndel[v];
    if (nd < 0 || pos < w.w0 + margin || pos > w.w1 - margin || nd > w.w1 - margin - pos) return false;
    if (a0 < 0 || a1 < a0 || a1 > L.A || a1 - a0 > L.max_alt || nd + (a1 - a0) < 1) return false;
    return (long long)w.n - nd + (a1 - a0) >= klen;
}

// a candidate: the variant in window coordinates
struct pv_edit {
    int u, nd, m;              // s' = s[:u] + alt + s[u + nd:]
    const uint8_t *alt;        // forward letters
    bool rev;
    __device__ __forceinline__ int letter(int x) const { return rev ? ge_comp(alt[m - 1 - x]) : (int)alt[x]; }
};

__device__ __forceinline__ pv_edit pv_place(const pv_list &L, long long v, const ge_win &w)
{
    pv_edit e;
    e.nd = L.ndel[v];
    e.m = (int)(L.alt_off[v + 1] - L.alt_off[v]);
    e.alt = L.alt + L.alt_off[v];
    e.rev = w.rev;
    e.u = w.rev ? (int)(w.w1 - L.pos[v] - e.nd) : (int)(L.pos[v] - w.w0);
    return e;
}

// One wave walks the variants that start inside window b's margins, 64 at a time.  EMIT false: counts those that fit.  EMIT true:
// writes them as candidates cand_off[b] .. in ascending variant order for a '+' window and descending for a '-' one.
template <bool EMIT>
__device__ __forceinline__ long long pv_walk(const pv_list &L, const int32_t *__restrict__ var_status, const ge_win &w, int b, int klen,
                                             int margin, long long base, long long total, int32_t *__restrict__ cand_pair,
                                             int32_t *__restrict__ cand_start, int32_t *__restrict__ cand_ndel,
                                             int32_t *__restrict__ cand_var, int64_t *__restrict__ cand_new_off)
{
    const int lane = threadIdx.x & 63;
    if (w.n < klen || w.n < 2 * (long long)margin) return 0;
    const long long first = pv_lower(L, w.off, w.w0 + margin), last = pv_lower(L, w.off, w.w1 - margin + 1);
    long long run = 0;
    for (long long v0 = first; v0 < last; v0 += 64) {
        const long long v = v0 + lane;
        const bool ok = v < last && pv_fits(L, var_status, v, w, klen, margin);
        const u64 mask = __ballot(ok);
        if (EMIT && ok) {
            const long long rank = run + __popcll(mask & ((1ull << lane) - 1));
            if (rank < total) {                                   // (a list that changed since the count pass writes no further)
                const long long i = base + (w.rev ? total - 1 - rank : rank);
                const pv_edit e = pv_place(L, v, w);
                int start, ndel, nnew;
                ge_triple(w, e, klen, &start, &ndel, &nnew);
                cand_pair[i] = b;
                cand_start[i] = start;
                cand_ndel[i] = ndel;
                cand_var[i] = (int)v;
                cand_new_off[i + 1] = nnew;
            }
        }
        run += __popcll(mask);
    }
    return run;
}

__global__ void __launch_bounds__(64 * GE_WAVES) variant_edits_count_kernel(
    pv_list L, const int32_t *__restrict__ var_status, const uint8_t *__restrict__ genome, long long G,
    const int64_t *__restrict__ win_off, const int64_t *__restrict__ w0, const int64_t *__restrict__ w1, int nwin, int klen, int margin,
    int64_t *__restrict__ ncand, int64_t *__restrict__ nkmer)
{
    const int b = blockIdx.x * GE_WAVES + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (b == 0 && lane == 0) {
        ncand[0] = 0;
        nkmer[0] = 0;
    }
    if (b >= nwin) return;                                       // (whole waves)
    ge_win w;
    long long cnt = 0, km = 0;
    if (ge_open(genome, win_off, w0, w1, nullptr, b, G, &w)) {
        km = w.n < klen ? 0 : w.n - klen + 1;
        cnt = pv_walk<false>(L, var_status, w, b, klen, margin, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr);
    }
    if (lane == 0) {
        ncand[b + 1] = cnt;
        nkmer[b + 1] = km;
    }
}

__global__ void __launch_bounds__(64 * GE_WAVES) variant_edits_emit_kernel(
    pv_list L, const int32_t *__restrict__ var_status, const uint8_t *__restrict__ genome, long long G,
    const int64_t *__restrict__ win_off, const int64_t *__restrict__ w0, const int64_t *__restrict__ w1,
    const int32_t *__restrict__ minus, int nwin, int klen, int margin, const int64_t *__restrict__ cand_off, long long ncand,
    int32_t *__restrict__ cand_pair, int32_t *__restrict__ cand_start, int32_t *__restrict__ cand_ndel, int32_t *__restrict__ cand_var,
    int64_t *__restrict__ cand_new_off)
{
    const int b = blockIdx.x * GE_WAVES + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (b == 0 && lane == 0) cand_new_off[0] = 0;
    if (b >= nwin) return;
    const long long base = cand_off[b], total = cand_off[b + 1] - base;
    if (base < 0 || total <= 0 || total > ncand - base) return;   // (its share of the list lies inside the list)
    ge_win w;
    long long got = 0;
    bool rev = false;
    if (ge_open(genome, win_off, w0, w1, minus, b, G, &w)) {
        rev = w.rev;
        got = pv_walk<true>(L, var_status, w, b, klen, margin, base, total, cand_pair, cand_start, cand_ndel, cand_var, cand_new_off);
    }
    // a share that is not this window's own count: what was not written stays a refused candidate (start -1)
    for (long long r = (got < total ? got : total) + lane; r < total; r += 64) {
        const long long i = base + (rev ? total - 1 - r : r);
        cand_pair[i] = b;
        cand_start[i] = -1;
        cand_ndel[i] = 0;
        cand_var[i] = -1;
        cand_new_off[i + 1] = 0;
    }
}

__global__ void __launch_bounds__(GE_THREADS) variant_edits_new_kernel(
    pv_list L, const int32_t *__restrict__ var_status, const uint8_t *__restrict__ genome, long long G,
    const int64_t *__restrict__ win_off, const int64_t *__restrict__ w0, const int64_t *__restrict__ w1,
    const int32_t *__restrict__ minus, int nwin, int klen, int blank, int margin, long long ncand,
    const int32_t *__restrict__ cand_pair, const int32_t *__restrict__ cand_start, const int32_t *__restrict__ cand_var,
    const int64_t *__restrict__ cand_new_off, long long new_cap, int32_t *__restrict__ cand_new)
{
    const long long i = (long long)blockIdx.x * GE_THREADS + threadIdx.x;
    if (i >= ncand) return;
    const int b = cand_pair[i];
    const long long v = cand_var[i];
    ge_win w;
    if (b < 0 || b >= nwin || !ge_open(genome, win_off, w0, w1, minus, b, G, &w) || !pv_fits(L, var_status, v, w, klen, margin)) return;
    ge_write_new(w, pv_place(L, v, w), klen, blank, cand_start[i], cand_new_off + i, new_cap, SLK_RESCORE_MAX_NEW, cand_new);
}

// ---- 3. the reads' gains per variant and strand --------------------------------------------------------------------------------------

// order: the candidates sorted by (variant, read), the host's sort.  The thread of a segment's first entry walks the segment: every sum
// is taken in read order whatever the launch's shape, and continues from what the cell holds.
__global__ void __launch_bounds__(GE_THREADS) variant_sum_gains_kernel(
    const double *__restrict__ score, const int32_t *__restrict__ read_minus, int nread, const double *__restrict__ ll_edit,
    const int32_t *__restrict__ cand_read, const int32_t *__restrict__ cand_var, const int64_t *__restrict__ order, long long ncand,
    long long V, double *__restrict__ gain, int32_t *__restrict__ support, int32_t *__restrict__ pro, double *__restrict__ gain_strand,
    int32_t *__restrict__ support_strand, int32_t *__restrict__ pro_strand)
{
    const long long i = (long long)blockIdx.x * GE_THREADS + threadIdx.x;
    if (i >= ncand) return;
    const long long ci = order[i];
    if (!ge_listed(ci, ncand)) return;
    const long long v = cand_var[ci];
    if (!ge_segment_head(order, ncand, i, cand_var, (int32_t)v)) return;
    if (v < 0 || v >= V) return;
    double sum = gain[v], ss0 = gain_strand[2 * v], ss1 = gain_strand[2 * v + 1];
    int cnt = support[v], np = pro[v], sc0 = support_strand[2 * v], sc1 = support_strand[2 * v + 1], sp0 = pro_strand[2 * v],
        sp1 = pro_strand[2 * v + 1];
    for (long long x = i; x < ncand; x++) {
        const long long c = order[x];
        if (!ge_listed(c, ncand) || cand_var[c] != v) break;
        const int r = cand_read[c];
        const bool known = r >= 0 && r < nread;
        const double l = ll_edit[c], s = known ? score[r] : __builtin_nan("");
        const bool rev = known && read_minus[r] != 0;
        const int what = ge_classify(l, s);
        if (what == GE_PAIR_NAN) {                               // the cells say so
            sum = __builtin_nan("");
            if (known && rev) ss1 = __builtin_nan("");
            else if (known) ss0 = __builtin_nan("");
        } else if (what == GE_PAIR_FINITE) {
            const double d = l - s;
            const int up = d > 0.0 ? 1 : 0;
            sum += d;
            cnt++;
            np += up;
            if (rev) { ss1 += d; sc1++; sp1 += up; } else { ss0 += d; sc0++; sp0 += up; }
        }
    }
    gain[v] = sum;
    support[v] = cnt;
    pro[v] = np;
    gain_strand[2 * v] = ss0;
    gain_strand[2 * v + 1] = ss1;
    support_strand[2 * v] = sc0;
    support_strand[2 * v + 1] = sc1;
    pro_strand[2 * v] = sp0;
    pro_strand[2 * v + 1] = sp1;
}

// ---- 4. the repeat-unit family -------------------------------------------------------------------------------------------------------

// The tract of period u that starts at letter p of the contig c[0 .. n): its copies, or 0 when p starts none (design 1.5, (i)-(iv)).
__device__ __forceinline__ long long pv_tract(const uint8_t *__restrict__ c, long long n, long long p, int u)
{
    if (p + 2 * u > n) return 0;                                 // (i) needs two copies inside the contig
    for (int i = 0; i < u; i++)
        if (ge_digit(c[p + i]) < 0 || c[p + i] != c[p + i + u]) return 0;
    if (p > 0 && c[p - 1] == c[p - 1 + u]) return 0;             // (ii) leftmost
    if (u == 2 && c[p] == c[p + 1]) return 0;                    // (iii) primitive
    if (u == 3 && c[p] == c[p + 1] && c[p + 1] == c[p + 2]) return 0;
    if (u == 4 && c[p] == c[p + 2] && c[p + 1] == c[p + 3]) return 0;
    long long l = 2 * u;
    while (p + l < n && c[p + l] == c[p + l - u]) l++;           // (ends at the contig's end at the latest)
    return l / u;
}

// What position g of the packed genome proposes.  EMIT false: -> (proposals, alt letters).  EMIT true: writes them from variant `vi`
// and alt letter `ai` on, in the order u, deletions before insertions, cnt ascending.
template <bool EMIT>
__device__ __forceinline__ void pv_propose(const uint8_t *__restrict__ genome, long long G, const int64_t *__restrict__ contig_off,
                                           int ncontig, long long g, int max_alt, int max_unit, int max_change, int min_copies,
                                           long long *nprop, long long *nalt, long long vi, long long ai, int64_t *var_off,
                                           int64_t *var_pos, int32_t *var_ndel, int64_t *var_alt_off, uint8_t *var_alt)
{
    *nprop = 0;
    *nalt = 0;
    const int lo = ge_find(contig_off, ncontig, g);
    const long long c0 = contig_off[lo], c1 = contig_off[lo + 1];
    if (c0 < 0 || c0 > g || c1 <= g || c1 > G) return;            // (the table is device data: g lies in no contig it names)
    const uint8_t *c = genome + c0;
    const long long n = c1 - c0, p = g - c0;
    long long np = 0, na = 0;
    for (int u = 1; u <= max_unit; u++) {
        const long long copies = pv_tract(c, n, p, u);
        if (copies < 2 || copies < min_copies) continue;
        for (int cnt = 1; cnt <= max_change; cnt++) {
            if (u * cnt == 1 || cnt > copies - 1) continue;
            if (EMIT) {
                var_off[vi + np] = c0;
                var_pos[vi + np] = p;
                var_ndel[vi + np] = u * cnt;
                var_alt_off[vi + np + 1] = ai + na;
            }
            np++;
        }
        for (int cnt = 1; cnt <= max_change; cnt++) {
            if (u * cnt == 1 || u * cnt > max_alt) continue;
            if (EMIT) {
                var_off[vi + np] = c0;
                var_pos[vi + np] = p;
                var_ndel[vi + np] = 0;
                for (int x = 0; x < u * cnt; x++) var_alt[ai + na + x] = c[p + x % u];
                var_alt_off[vi + np + 1] = ai + na + u * cnt;
            }
            np++;
            na += u * cnt;
        }
    }
    *nprop = np;
    *nalt = na;
}

__global__ void __launch_bounds__(GE_THREADS) repeat_variants_count_kernel(
    const uint8_t *__restrict__ genome, long long G, const int64_t *__restrict__ contig_off, int ncontig, long long lo, long long P,
    int max_alt, int max_unit, int max_change, int min_copies, int64_t *__restrict__ nprop, int64_t *__restrict__ nalt)
{
    const long long t = (long long)blockIdx.x * GE_THREADS + threadIdx.x;
    if (t == 0) {
        nprop[0] = 0;
        nalt[0] = 0;
    }
    if (t >= P) return;
    long long np, na;
    pv_propose<false>(genome, G, contig_off, ncontig, lo + t, max_alt, max_unit, max_change, min_copies, &np, &na, 0, 0, nullptr, nullptr,
                      nullptr, nullptr, nullptr);
    nprop[t + 1] = np;
    nalt[t + 1] = na;
}

__global__ void __launch_bounds__(GE_THREADS) repeat_variants_emit_kernel(
    const uint8_t *__restrict__ genome, long long G, const int64_t *__restrict__ contig_off, int ncontig, long long lo, long long P,
    int max_alt, int max_unit, int max_change, int min_copies, const int64_t *__restrict__ prop_off, const int64_t *__restrict__ alt_off,
    long long V, long long A, int64_t *__restrict__ var_off, int64_t *__restrict__ var_pos, int32_t *__restrict__ var_ndel,
    int64_t *__restrict__ var_alt_off, uint8_t *__restrict__ var_alt)
{
    const long long t = (long long)blockIdx.x * GE_THREADS + threadIdx.x;
    if (t == 0) var_alt_off[0] = 0;
    if (t >= P) return;
    const long long vi = prop_off[t], ai = alt_off[t], nv = prop_off[t + 1] - vi, nl = alt_off[t + 1] - ai;
    if (vi < 0 || nv <= 0 || nv > V - vi || ai < 0 || nl < 0 || nl > A - ai) return;
    long long np, na;
    pv_propose<false>(genome, G, contig_off, ncontig, lo + t, max_alt, max_unit, max_change, min_copies, &np, &na, 0, 0, nullptr, nullptr,
                      nullptr, nullptr, nullptr);
    if (np != nv || na != nl) return;                            // (offsets that are not this position's own counts are not followed)
    pv_propose<true>(genome, G, contig_off, ncontig, lo + t, max_alt, max_unit, max_change, min_copies, &np, &na, vi, ai, var_off, var_pos,
                     var_ndel, var_alt_off, var_alt);
}

// ---- entries -------------------------------------------------------------------------------------------------------------------------

static inline bool pv_make_list(const int64_t *var_off, const int64_t *var_pos, const int32_t *var_ndel, const int64_t *var_alt_off,
                                const uint8_t *var_alt, int64_t V, int64_t A, int klen, pv_list *L)
{
    if (V < 0 || A < 0 || V > 0x7ffffff0ll || !ge_klen(klen) || !var_alt_off) return false;
    if (V > 0 && (!var_off || !var_pos || !var_ndel)) return false;
    if (A > 0 && !var_alt) return false;
    L->off = var_off;
    L->pos = var_pos;
    L->ndel = var_ndel;
    L->alt_off = var_alt_off;
    L->alt = var_alt;
    L->V = V;
    L->A = A;
    L->max_alt = SLK_RESCORE_MAX_NEW - klen + 1;
    return true;
}

extern "C" int slk_variant_edits_count(const uint8_t *genome, long G, const int64_t *contig_off, int ncontig, const int64_t *var_off,
                                       const int64_t *var_pos, const int32_t *var_ndel, const int64_t *var_alt_off,
                                       const uint8_t *var_alt, int64_t V, int64_t A, const int64_t *win_off, const int64_t *w0,
                                       const int64_t *w1, int nwin, int kmer_len, int margin, int32_t *var_status, int64_t *ncand,
                                       int64_t *nkmer, slk_stream_t stream)
{
    pv_list L;
    if (!pv_make_list(var_off, var_pos, var_ndel, var_alt_off, var_alt, V, A, kmer_len, &L)) return SLK_ERR_INVALID_ARG;
    if (nwin < 0 || G < 0 || ncontig < 1 || margin < 0 || !contig_off || !ncand || !nkmer) return SLK_ERR_INVALID_ARG;
    if ((V > 0 && (!var_status || !genome)) || (nwin > 0 && (!win_off || !w0 || !w1 || !genome))) return SLK_ERR_INVALID_ARG;
    if (V > 0) {
        hipLaunchKernelGGL(variant_status_kernel, dim3(ge_blocks(V)), dim3(GE_THREADS), 0, slk_stream(stream), L, genome, (long long)G,
                           contig_off, ncontig, var_status);
        if (slk_launch_status() != SLK_OK) return SLK_ERR_LAUNCH;
    }
    hipLaunchKernelGGL(variant_edits_count_kernel, dim3(nwin > 0 ? (nwin + GE_WAVES - 1) / GE_WAVES : 1), dim3(64 * GE_WAVES), 0,
                       slk_stream(stream), L, var_status, genome, (long long)G, win_off, w0, w1, nwin, kmer_len, margin, ncand, nkmer);
    return slk_launch_status();
}

extern "C" int slk_variant_edits_emit(const uint8_t *genome, long G, const int64_t *var_off, const int64_t *var_pos,
                                      const int32_t *var_ndel, const int64_t *var_alt_off, const uint8_t *var_alt, int64_t V, int64_t A,
                                      const int32_t *var_status, const int64_t *win_off, const int64_t *w0, const int64_t *w1,
                                      const int32_t *minus, int nwin, int kmer_len, int margin, const int64_t *cand_off, int64_t ncand,
                                      int32_t *cand_pair, int32_t *cand_start, int32_t *cand_ndel, int32_t *cand_var,
                                      int64_t *cand_new_off, slk_stream_t stream)
{
    pv_list L;
    if (!pv_make_list(var_off, var_pos, var_ndel, var_alt_off, var_alt, V, A, kmer_len, &L)) return SLK_ERR_INVALID_ARG;
    if (nwin < 0 || G < 0 || margin < 0 || ncand < 0 || !cand_new_off) return SLK_ERR_INVALID_ARG;
    if (ncand > 0 && (nwin < 1 || V < 1 || !genome || !var_status || !win_off || !w0 || !w1 || !minus || !cand_off || !cand_pair ||
                      !cand_start || !cand_ndel || !cand_var))
        return SLK_ERR_INVALID_ARG;
    hipLaunchKernelGGL(variant_edits_emit_kernel, dim3(ncand > 0 ? (nwin + GE_WAVES - 1) / GE_WAVES : 1), dim3(64 * GE_WAVES), 0,
                       slk_stream(stream), L, var_status, genome, (long long)G, win_off, w0, w1, minus, ncand > 0 ? nwin : 0, kmer_len,
                       margin, cand_off, (long long)ncand, cand_pair, cand_start, cand_ndel, cand_var, cand_new_off);
    return slk_launch_status();
}

extern "C" int slk_variant_edits_new(const uint8_t *genome, long G, const int64_t *var_off, const int64_t *var_pos,
                                     const int32_t *var_ndel, const int64_t *var_alt_off, const uint8_t *var_alt, int64_t V, int64_t A,
                                     const int32_t *var_status, const int64_t *win_off, const int64_t *w0, const int64_t *w1,
                                     const int32_t *minus, int nwin, int kmer_len, int blank, int margin, int64_t ncand,
                                     const int32_t *cand_pair, const int32_t *cand_start, const int32_t *cand_var,
                                     const int64_t *cand_new_off, int64_t new_cap, int32_t *cand_new, slk_stream_t stream)
{
    pv_list L;
    if (!pv_make_list(var_off, var_pos, var_ndel, var_alt_off, var_alt, V, A, kmer_len, &L)) return SLK_ERR_INVALID_ARG;
    if (nwin < 0 || G < 0 || margin < 0 || ncand < 0 || new_cap < 0 || blank < 0) return SLK_ERR_INVALID_ARG;
    if (ncand == 0) return SLK_OK;
    if (nwin < 1 || V < 1 || !genome || !var_status || !win_off || !w0 || !w1 || !minus || !cand_pair || !cand_start || !cand_var ||
        !cand_new_off || !cand_new)
        return SLK_ERR_INVALID_ARG;
    hipLaunchKernelGGL(variant_edits_new_kernel, dim3(ge_blocks(ncand)), dim3(GE_THREADS), 0, slk_stream(stream), L, var_status, genome,
                       (long long)G, win_off, w0, w1, minus, nwin, kmer_len, blank, margin, (long long)ncand, cand_pair, cand_start,
                       cand_var, cand_new_off, (long long)new_cap, cand_new);
    return slk_launch_status();
}

extern "C" int slk_polish_sum_variant_gains_f64(const double *score, const int32_t *read_minus, int nread, const double *ll_edit,
                                                const int32_t *cand_read, const int32_t *cand_var, const int64_t *order, int64_t ncand,
                                                int64_t V, double *gain, int32_t *support, int32_t *pro, double *gain_strand,
                                                int32_t *support_strand, int32_t *pro_strand, slk_stream_t stream)
{
    if (nread < 0 || ncand < 0 || V < 0) return SLK_ERR_INVALID_ARG;
    if (ncand == 0 || V == 0) return SLK_OK;
    if (!score || !read_minus || !ll_edit || !cand_read || !cand_var || !order || !gain || !support || !pro || !gain_strand ||
        !support_strand || !pro_strand)
        return SLK_ERR_INVALID_ARG;
    hipLaunchKernelGGL(variant_sum_gains_kernel, dim3(ge_blocks(ncand)), dim3(GE_THREADS), 0, slk_stream(stream), score, read_minus, nread,
                       ll_edit, cand_read, cand_var, order, (long long)ncand, (long long)V, gain, support, pro, gain_strand,
                       support_strand, pro_strand);
    return slk_launch_status();
}

static inline bool pv_repeat_args(long G, int ncontig, int64_t lo, int64_t P, int klen, int max_unit, int max_change, int min_copies)
{
    return G >= 0 && ncontig >= 1 && lo >= 0 && P >= 0 && lo <= G && P <= G - lo && ge_klen(klen) && max_unit >= 1 &&
           max_unit <= PV_MAX_UNIT && max_change >= 1 && max_change <= PV_MAX_CHANGE && min_copies >= 2;
}

extern "C" int slk_repeat_variants_count(const uint8_t *genome, long G, const int64_t *contig_off, int ncontig, int64_t lo, int64_t P,
                                         int kmer_len, int max_unit, int max_change, int min_copies, int64_t *nprop, int64_t *nalt,
                                         slk_stream_t stream)
{
    if (!pv_repeat_args(G, ncontig, lo, P, kmer_len, max_unit, max_change, min_copies) || !contig_off || !nprop || !nalt)
        return SLK_ERR_INVALID_ARG;
    if (P > 0 && !genome) return SLK_ERR_INVALID_ARG;
    hipLaunchKernelGGL(repeat_variants_count_kernel, dim3(ge_blocks(P > 0 ? P : 1)), dim3(GE_THREADS), 0, slk_stream(stream), genome,
                       (long long)G, contig_off, ncontig, (long long)lo, (long long)P, SLK_RESCORE_MAX_NEW - kmer_len + 1, max_unit,
                       max_change, min_copies, nprop, nalt);
    return slk_launch_status();
}

extern "C" int slk_repeat_variants_emit(const uint8_t *genome, long G, const int64_t *contig_off, int ncontig, int64_t lo, int64_t P,
                                        int kmer_len, int max_unit, int max_change, int min_copies, const int64_t *prop_off,
                                        const int64_t *alt_off, int64_t V, int64_t A, int64_t *var_off, int64_t *var_pos,
                                        int32_t *var_ndel, int64_t *var_alt_off, uint8_t *var_alt, slk_stream_t stream)
{
    if (!pv_repeat_args(G, ncontig, lo, P, kmer_len, max_unit, max_change, min_copies) || V < 0 || A < 0 || !contig_off || !var_alt_off)
        return SLK_ERR_INVALID_ARG;
    if (V > 0 && (!genome || !prop_off || !alt_off || !var_off || !var_pos || !var_ndel)) return SLK_ERR_INVALID_ARG;
    if (A > 0 && !var_alt) return SLK_ERR_INVALID_ARG;
    hipLaunchKernelGGL(repeat_variants_emit_kernel, dim3(ge_blocks(V > 0 && P > 0 ? P : 1)), dim3(GE_THREADS), 0, slk_stream(stream),
                       genome, (long long)G, contig_off, ncontig, (long long)lo, V > 0 ? (long long)P : 0ll, SLK_RESCORE_MAX_NEW - kmer_len + 1,
                       max_unit, max_change, min_copies, prop_off, alt_off, (long long)V, (long long)A, var_off, var_pos, var_ndel,
                       var_alt_off, var_alt);
    return slk_launch_status();
}
