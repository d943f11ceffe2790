// polish_genome.hip -- the join of the genome half and the signal half (design/polish_genome.md; the quantities are defined in its
// section 1 and restated as plain loops in tests/polish_genome_ref.py).
//
// Integer kernels but the last; no LDS, no MFMA.  Every input is device data and is NOT trusted: no loop bound and no address depends
// on a value that has not been checked in the same kernel.
//   polish_read_windows_kernel  one wave per read: checks the read's call and alignment (device data, NOT trusted), writes the row of
//                               every called letter into a work table, and takes the centre line of the aligned rows through the
//                               alignment's columns, 64 columns per step with ballots as csrc/pileup.hip walks them.
//   letter_edits_count_kernel   one thread per window: how many candidates and k-mers it has (closed forms).
//   letter_edits_emit_kernel    one thread per candidate: (pair, start, ndel, number of new symbols, edit).
//   letter_edits_new_kernel     one thread per candidate: its new symbols, behind the prefix sum of their numbers.
//   window_kmers_kernel         one thread per k-mer of a window: its posterior column.
//   polish_sum_gains_kernel     one thread per candidate of the sorted list; the head of a segment of equal edits walks it in read
//                               order, so a cell's bits depend on no launch shape.  No floating-point atomics.
// The window, the edit as a replacement, its (start, ndel, new symbols) and the pieces of the sum kernel's walk are genome_edits.h's,
// shared with polish_variants.hip; this file keeps the read's window and centre line, the closed-form counts, which edit candidate r
// of a window is, the edit's forward-strand cell and the cell's sum.
#include "genome_edits.h"

#define PG_MAX_LEN 65535                        // as the traceback: a pair has at most 2 * 65535 columns

// ---- 1. windows ------------------------------------------------------------------------------------------------------------------

__device__ __forceinline__ int pg_check_row(const int *row, long long nq, long ldq, long long nr, long long o0, long long o1,
                                            long long ops_bytes, long long ws, long long G)
{
    const int qs = row[1], qe = row[2], rs = row[3], re = row[4];
    if (nq < 0 || nq > PG_MAX_LEN || nq > ldq || nr < 0 || nr > PG_MAX_LEN || qs < 0 || qe < qs || qe > nq || rs < 0 || re < rs ||
        re > nr)
        return SLK_POLISH_BAD_SPAN;
    if (row[5] < 0 || row[6] < 0 || row[7] < 0 || row[8] < 0) return SLK_POLISH_BAD_COUNT;
    if ((long long)row[5] + row[6] + row[7] != qe - qs || (long long)row[5] + row[6] + row[8] != re - rs) return SLK_POLISH_BAD_SUM;
    const long long ncol = (long long)row[5] + row[6] + row[7] + row[8];
    if (o0 < 0 || o1 > ops_bytes || o1 - o0 != ncol) return SLK_POLISH_OPS;
    if (ws < 0 || ws + nr > G) return SLK_POLISH_POSITION;
    return SLK_POLISH_DONE;
}

__global__ void __launch_bounds__(64 * GE_WAVES) polish_read_windows_kernel(
    const int32_t *__restrict__ paths, long ldp, const int32_t *__restrict__ lens, const int32_t *__restrict__ move_row, long ldm,
    int T, const int32_t *__restrict__ nrow, const int32_t *__restrict__ qlen, long ldq, const int64_t *__restrict__ roff,
    const int32_t *__restrict__ rows, const uint8_t *__restrict__ ops, const int64_t *__restrict__ ops_off, long long ops_bytes,
    const int32_t *__restrict__ tb_status, const int32_t *__restrict__ minus, const uint8_t *__restrict__ keep,
    const int64_t *__restrict__ wstart, const int64_t *__restrict__ coff, long long G, int B, int klen,
    const int64_t *__restrict__ center_off, int32_t *letter_row, int32_t *__restrict__ status, int32_t *__restrict__ row_span,
    int64_t *__restrict__ window, int32_t *center)
{
    const int lane = threadIdx.x & 63;
    const int b = blockIdx.x * GE_WAVES + (threadIdx.x >> 6);
    if (b >= B) return;                                          // (whole waves: nothing below synchronises across waves)
    if (keep[b] == 0 || tb_status[b] != SLK_ALIGN_TB_DONE) {
        if (lane == 0) status[b] = SLK_POLISH_SKIPPED;
        return;
    }
    int row[9];
#pragma unroll
    for (int k = 0; k < 9; k++) row[k] = rows[(size_t)b * 9 + k];
    const long long o0 = ops_off[b], nq = qlen[b], nr = roff[b + 1] - roff[b], ws = wstart[b];
    int st = pg_check_row(row, nq, ldq, nr, o0, ops_off[b + 1], ops_bytes, ws, G);
    const long long c0 = coff[b];
    if (st == SLK_POLISH_DONE && (c0 < 0 || c0 > ws)) st = SLK_POLISH_POSITION;
    if (st != SLK_POLISH_DONE) {
        if (lane == 0) status[b] = st;
        return;
    }
    const int ncol = row[5] + row[6] + row[7] + row[8];
    const uint8_t *o = ops + o0;
    {   // the codes themselves: every byte a code, and as many of each kind as the row says
        int cnt0 = 0, cnt1 = 0, cnt2 = 0, cnt3 = 0;
        bool bad = false;
        for (int cb = 0; cb < ncol; cb += 64) {
            const int c = cb + lane < ncol ? (int)o[cb + lane] : -1;
            bad |= __ballot(c > SLK_ALIGN_OP_DELETION) != 0;
            cnt0 += __popcll(__ballot(c == 0));
            cnt1 += __popcll(__ballot(c == 1));
            cnt2 += __popcll(__ballot(c == 2));
            cnt3 += __popcll(__ballot(c == 3));
        }
        if (bad) st = SLK_POLISH_BAD_CODE;
        else if (cnt0 != row[5] || cnt1 != row[6] || cnt2 != row[7] || cnt3 != row[8]) st = SLK_POLISH_CODE_COUNT;
        if (st != SLK_POLISH_DONE) {
            if (lane == 0) status[b] = st;
            return;
        }
    }
    // the call: every state a k-mer, the rows in range and not decreasing, and as many letters as the aligner saw
    const int n = lens[b], R = nrow[b];
    if (n < 1 || n > T || R < 1) {
        if (lane == 0) status[b] = SLK_POLISH_PATH;
        return;
    }
    int nstate = 1;
    for (int i = 0; i < klen; i++) nstate *= 4;
    const int32_t *p = paths + (size_t)b * ldp, *mr = move_row + (size_t)b * ldm;
    int32_t *lr = letter_row + (size_t)b * ldq;
    long long carry = 0;
    bool badpath = false, badrow = false;
    for (int base = 0; base < n; base += 64) {
        const int i = base + lane;
        int mv = 0, r = 0;
        bool bp = false, br = false;
        if (i < n) {
            const int s2 = p[i];
            r = mr[i];
            bp = s2 < 0 || s2 >= nstate;
            br = r < 0 || r >= R;
            mv = klen;
            if (i > 0) {
                const int s1 = p[i - 1];
                bp |= s1 < 0 || s1 >= nstate;
                br |= mr[i - 1] > r;
                if (!bp) {
                    int hi = 4, lo = nstate / 4;                   // 4^sh, 4^(klen - sh): the overlap rule of csrc/bases.hip
                    for (int sh = 1; sh < klen; sh++) {
                        if (mv == klen && s1 % lo == s2 / hi) mv = sh;
                        hi *= 4;
                        lo /= 4;
                    }
                }
            }
        }
        badpath |= __ballot(bp) != 0;
        badrow |= __ballot(br) != 0;
        int incl = mv;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const int v = __shfl_up(incl, off);
            if (lane >= off) incl += v;
        }
        const long long pos = carry + incl - mv;
        if (!badpath && !badrow)
            for (int d = 0; d < mv; d++)
                if (pos + d < nq) lr[pos + d] = r;
        carry += __shfl(incl, 63);
    }
    if (badpath || carry != nq) st = SLK_POLISH_PATH;
    else if (badrow) st = SLK_POLISH_MOVE_ROW;
    const int qs = row[1], qe = row[2], rs = row[3], re = row[4];
    const int L = re - rs - klen + 1;
    if (st == SLK_POLISH_DONE && L < 1) st = SLK_POLISH_SHORT;
    if (st != SLK_POLISH_DONE) {
        if (lane == 0) status[b] = st;
        return;
    }
    __threadfence();                                             // every lane's letter rows, read by all below
    // a window letter's row is that of the query letter in its column, or of the next one for a deletion.  r0: the row of the
    // window's letter klen - 1 (its first k-mer is whole); r1: the first row behind the rows of the last aligned letter's k-mer
    int r0 = 0;
    {
        int jbase = 0, ibase = 0;
        for (int cb = 0; cb < ncol; cb += 64) {
            const int col = cb + lane;
            const int c = col < ncol ? (int)o[col] : 255;
            const u64 lt = (1ull << lane) - 1;
            const u64 mq = __ballot(c <= SLK_ALIGN_OP_INSERTION), mrf = __ballot(c <= SLK_ALIGN_OP_MISMATCH || c == SLK_ALIGN_OP_DELETION);
            const int ci = ibase + __popcll(mq & lt), cj = jbase + __popcll(mrf & lt);
            const bool rc = c <= SLK_ALIGN_OP_MISMATCH || c == SLK_ALIGN_OP_DELETION;
            const u64 hit = __ballot(rc && cj == klen - 1);
            if (hit) {
                const int src = __ffsll((long long)hit) - 1;
                const int qi = qs + ci < qe - 1 ? qs + ci : qe - 1;
                const int mine = qe > qs ? lr[qi] : 0;
                r0 = __shfl(mine, src);
                break;
            }
            ibase += __popcll(mq);
            jbase += __popcll(mrf);
        }
    }
    if (qe <= qs) {                                              // (no query letter: L >= 1 needs deletions only, nothing to score)
        if (lane == 0) status[b] = SLK_POLISH_FEW_ROWS;
        return;
    }
    const int rl = lr[qe - 1];
    int r1 = R;
    for (int x0 = qe; x0 < nq; x0 += 64) {
        const int x = x0 + lane;
        const u64 above = __ballot(x < nq && lr[x < nq ? x : qe - 1] > rl);
        if (above) {
            const int src = __ffsll((long long)above) - 1;
            r1 = __shfl(lr[x < nq ? x : qe - 1], src);
            break;
        }
    }
    const long long Tp = (long long)r1 - r0;
    if (Tp < L) st = SLK_POLISH_FEW_ROWS;
    else if (center_off[b] < 0 || center_off[b + 1] - center_off[b] < Tp + 1) st = SLK_POLISH_CENTER;
    if (st != SLK_POLISH_DONE) {
        if (lane == 0) status[b] = st;
        return;
    }
    int32_t *cen = center + center_off[b];
    for (int t = lane; t <= Tp; t += 64) cen[t] = 0;
    __threadfence();
    {
        int jbase = 0, ibase = 0;
        for (int cb = 0; cb < ncol; cb += 64) {
            const int col = cb + lane;
            const int c = col < ncol ? (int)o[col] : 255;
            const u64 lt = (1ull << lane) - 1;
            const u64 mq = __ballot(c <= SLK_ALIGN_OP_INSERTION), mrf = __ballot(c <= SLK_ALIGN_OP_MISMATCH || c == SLK_ALIGN_OP_DELETION);
            const int ci = ibase + __popcll(mq & lt), cj = jbase + __popcll(mrf & lt);
            const bool rc = c <= SLK_ALIGN_OP_MISMATCH || c == SLK_ALIGN_OP_DELETION;
            if (rc && cj >= klen - 1) {
                const int qi = qs + ci < qe - 1 ? qs + ci : qe - 1;
                const long long idx = (long long)lr[qi] - r0 + 1;
                if (idx >= 1 && idx <= Tp) atomicAdd(cen + idx, 1);   // (integer: the sums depend on no order)
            }
            ibase += __popcll(mq);
            jbase += __popcll(mrf);
        }
    }
    __threadfence();
    int run = 0;                                                 // the running sum: the k-mers passed before each row
    for (long long t0 = 0; t0 <= Tp; t0 += 64) {
        const long long t = t0 + lane;
        int incl = t <= Tp ? cen[t] : 0;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const int v = __shfl_up(incl, off);
            if (lane >= off) incl += v;
        }
        if (t <= Tp) cen[t] = run + incl;
        run += __shfl(incl, 63);
    }
    if (lane == 0) {
        const bool rev = minus[b] != 0;
        row_span[2 * b] = r0;
        row_span[2 * b + 1] = r1;
        window[2 * b] = (rev ? ws + (nr - re) : ws + rs) - c0;
        window[2 * b + 1] = (rev ? ws + (nr - rs) : ws + re) - c0;
        status[b] = SLK_POLISH_DONE;
    }
}

// ---- 2. candidates from letters ------------------------------------------------------------------------------------------------------

// per position: 3 substitutions, a deletion (when the shorter string still has a k-mer), 4 insertions, each when its kind is asked for
__device__ __forceinline__ int pg_per_position(int n, int klen, int kinds)
{
    return ((kinds & 1) ? 3 : 0) + (((kinds & 2) && n - 1 >= klen) ? 1 : 0) + ((kinds & 4) ? 4 : 0);
}

__device__ __forceinline__ long long pg_ncand(long long n, int klen, int kinds, int margin)
{
    const long long lo = margin, hi = n - margin;
    if (n < klen || hi < lo) return 0;
    return (hi - lo) * pg_per_position((int)n, klen, kinds) + ((kinds & 4) ? 4 : 0);
}

__global__ void __launch_bounds__(GE_THREADS) letter_edits_count_kernel(
    const int64_t *__restrict__ win_off, const int64_t *__restrict__ w0, const int64_t *__restrict__ w1, int nwin, long long G, int klen,
    int kinds, int margin, int64_t *__restrict__ ncand, int64_t *__restrict__ nkmer)
{
    const int b = blockIdx.x * GE_THREADS + threadIdx.x;
    if (b == 0) {
        ncand[0] = 0;
        nkmer[0] = 0;
    }
    if (b >= nwin) return;
    const long long n = ge_window_len(win_off[b], w0[b], w1[b], G);
    ncand[b + 1] = n < 0 ? 0 : pg_ncand(n, klen, kinds, margin);
    nkmer[b + 1] = n < klen ? 0 : n - klen + 1;
}

struct pg_edit {
    int kind;                  // 0 substitution, 1 deletion, 2 insertion
    int u, nd, m;              // window position; the letters it removes and puts there (genome_edits.h)
    int c;                     // the window's new letter (substitution, insertion)
    __device__ __forceinline__ int letter(int) const { return c; }
    __device__ __forceinline__ void set(int k, int l) { kind = k; c = l; nd = k == 2 ? 0 : 1; m = k == 1 ? 0 : 1; }
};

// candidate r of a window, in the order of bio.single_letter_edits on the window's own string
__device__ __forceinline__ pg_edit pg_decode(const ge_win &w, long long r, int klen, int kinds, int margin)
{
    const int per = pg_per_position(w.n, klen, kinds), lo = margin, hi = w.n - margin;
    pg_edit e;
    int q;
    if (per > 0 && r < (long long)(hi - lo) * per) {
        e.u = lo + (int)(r / per);
        q = (int)(r % per);
    } else {
        e.u = hi;
        q = (int)(r - (long long)(hi - lo) * per) + per - 4;     // (behind the last letter: insertions only)
    }
    if (kinds & 1) {
        if (q < 3) {
            const int d = ge_digit(w.at(e.u));
            e.set(0, "ACGT"[q + (d >= 0 && q >= d ? 1 : 0)]);
            return e;
        }
        q -= 3;
    }
    if ((kinds & 2) && w.n - 1 >= klen) {
        if (q == 0) {
            e.set(1, 0);
            return e;
        }
        q -= 1;
    }
    e.set(2, "ACGT"[q & 3]);
    return e;
}

// Candidate i of the list laid out by cand_off: its window and its edit.  A candidate list that is not the window's own count is not
// followed (false).
__device__ __forceinline__ bool pg_candidate(const uint8_t *__restrict__ genome, long long G, const int64_t *__restrict__ win_off,
                                             const int64_t *__restrict__ w0, const int64_t *__restrict__ w1,
                                             const int32_t *__restrict__ minus, int nwin, int klen, int kinds, int margin,
                                             const int64_t *__restrict__ cand_off, long long i, int *b, ge_win *w, pg_edit *e)
{
    *b = ge_find(cand_off, nwin, i);
    const long long first = cand_off[*b];
    if (!ge_open(genome, win_off, w0, w1, minus, *b, G, w) || cand_off[*b + 1] - first != pg_ncand(w->n, klen, kinds, margin)) return false;
    *e = pg_decode(*w, i - first, klen, kinds, margin);
    return true;
}

__global__ void __launch_bounds__(GE_THREADS) letter_edits_emit_kernel(
    const uint8_t *__restrict__ genome, long long G, const int64_t *__restrict__ win_off, const int64_t *__restrict__ w0,
    const int64_t *__restrict__ w1, const int32_t *__restrict__ minus, int nwin, int klen, int kinds, int margin,
    const int64_t *__restrict__ cand_off, long long ncand, int32_t *__restrict__ cand_pair, int32_t *__restrict__ cand_start,
    int32_t *__restrict__ cand_ndel, int64_t *__restrict__ cand_new_off, int64_t *__restrict__ cand_edit)
{
    const long long i = (long long)blockIdx.x * GE_THREADS + threadIdx.x;
    if (i == 0) cand_new_off[0] = 0;
    if (i >= ncand) return;
    ge_win w;
    pg_edit e;
    // a candidate that is not followed stays a refused one (start -1)
    int b, start = -1, ndel = 0, nnew = 0;
    long long edit = -1;
    if (pg_candidate(genome, G, win_off, w0, w1, minus, nwin, klen, kinds, margin, cand_off, i, &b, &w, &e)) {
        ge_triple(w, e, klen, &start, &ndel, &nnew);
        // the edit on the forward strand: position, and the slot 0-2 substitutions, 3 deletion, 4-7 insertions in front of it
        const int fu = !w.rev ? e.u : e.kind == 2 ? w.n - e.u : w.n - 1 - e.u;
        int slot = 3;
        if (e.kind != 1) {
            const int fl = ge_digit(w.rev ? ge_comp(e.c) : e.c);
            if (e.kind == 2) slot = 4 + fl;
            else {
                const int fd = ge_digit(w.g[fu]);
                slot = fl - (fd >= 0 && fl > fd ? 1 : 0);
                if (slot > 2) slot = 2;
            }
        }
        edit = 8 * (w.off + w.w0 + fu) + slot;
    }
    cand_pair[i] = b;
    cand_start[i] = start;
    cand_ndel[i] = ndel;
    cand_new_off[i + 1] = nnew;
    cand_edit[i] = edit;
}

__global__ void __launch_bounds__(GE_THREADS) letter_edits_new_kernel(
    const uint8_t *__restrict__ genome, long long G, const int64_t *__restrict__ win_off, const int64_t *__restrict__ w0,
    const int64_t *__restrict__ w1, const int32_t *__restrict__ minus, int nwin, int klen, int blank, int kinds, int margin,
    const int64_t *__restrict__ cand_off, long long ncand, const int32_t *__restrict__ cand_start,
    const int64_t *__restrict__ cand_new_off, long long new_cap, int32_t *__restrict__ cand_new)
{
    const long long i = (long long)blockIdx.x * GE_THREADS + threadIdx.x;
    if (i >= ncand) return;
    ge_win w;
    pg_edit e;
    int b;
    if (!pg_candidate(genome, G, win_off, w0, w1, minus, nwin, klen, kinds, margin, cand_off, i, &b, &w, &e)) return;
    ge_write_new(w, e, klen, blank, cand_start[i], cand_new_off + i, new_cap, klen + 1, cand_new);
}

__global__ void __launch_bounds__(GE_THREADS) window_kmers_kernel(
    const uint8_t *__restrict__ genome, long long G, const int64_t *__restrict__ win_off, const int64_t *__restrict__ w0,
    const int64_t *__restrict__ w1, const int32_t *__restrict__ minus, int nwin, int klen, int blank,
    const int64_t *__restrict__ pos_off, long long npos, int32_t *__restrict__ seq)
{
    const long long i = (long long)blockIdx.x * GE_THREADS + threadIdx.x;
    if (i >= npos) return;
    const int b = ge_find(pos_off, nwin, i);
    ge_win w;
    if (!ge_open(genome, win_off, w0, w1, minus, b, G, &w) || pos_off[b + 1] - pos_off[b] != (w.n < klen ? 0 : w.n - klen + 1)) {
        seq[i] = -1;
        return;
    }
    seq[i] = ge_column([&](int j) { return w.at(j); }, (int)(i - pos_off[b]), klen, blank);
}

// ---- 3. the reads' gains on genome coordinates ---------------------------------------------------------------------------------------

// order: the candidates sorted by (edit, read), the host's sort.  The thread of a segment's first entry walks the segment: the cell's
// sum is taken in read order whatever the launch's shape, and continues from what the cell holds (the caller zeroes once; launches
// that come in read order give the bits of one).
__global__ void __launch_bounds__(GE_THREADS) polish_sum_gains_kernel(
    const double *__restrict__ score, int nread, const double *__restrict__ ll_edit, const int32_t *__restrict__ cand_pair,
    const int64_t *__restrict__ cand_edit, const int64_t *__restrict__ order, long long ncand, long long region_start, long long P,
    double *__restrict__ gain, int32_t *__restrict__ support)
{
    const long long i = (long long)blockIdx.x * GE_THREADS + threadIdx.x;
    if (i >= ncand) return;
    const long long ci = order[i];
    if (!ge_listed(ci, ncand)) return;
    const long long edit = cand_edit[ci];
    if (!ge_segment_head(order, ncand, i, cand_edit, (int64_t)edit)) return;
    const long long cell = edit - 8 * region_start;
    if (edit < 0 || cell < 0 || cell >= 8 * P) return;
    double sum = gain[cell];
    int cnt = support[cell];
    for (long long x = i; x < ncand; x++) {
        const long long c = order[x];
        if (!ge_listed(c, ncand) || cand_edit[c] != edit) break;
        const int r = cand_pair[c];
        const double l = ll_edit[c], s = r >= 0 && r < nread ? score[r] : __builtin_nan("");
        const int what = ge_classify(l, s);
        if (what == GE_PAIR_NAN) sum = __builtin_nan("");        // the cell says so
        else if (what == GE_PAIR_FINITE) {
            sum += l - s;
            cnt++;
        }
    }
    gain[cell] = sum;
    support[cell] = cnt;
}

// ---- entries --------------------------------------------------------------------------------------------------------------------------

static inline bool pg_edit_args(int nwin, long G, int klen, int kinds, int margin)
{
    return nwin >= 0 && G >= 0 && ge_klen(klen) && kinds >= 0 && kinds <= 7 && margin >= 0;
}

extern "C" int slk_polish_read_windows(const int32_t *paths, long ldp, const int32_t *lens, const int32_t *move_row, long ldm, int T,
                                       const int32_t *nrow, const int32_t *qlen, long ldq, const int64_t *roff, const int32_t *rows,
                                       const uint8_t *ops, const int64_t *ops_off, size_t ops_bytes, const int32_t *tb_status,
                                       const int32_t *minus, const uint8_t *keep, const int64_t *wstart, const int64_t *coff, long G,
                                       int B, int kmer_len, const int64_t *center_off, int32_t *letter_row, int32_t *status,
                                       int32_t *row_span, int64_t *window, int32_t *center, slk_stream_t stream)
{
    if (B < 0 || G < 0 || T < 0 || !ge_klen(kmer_len)) return SLK_ERR_INVALID_ARG;
    if (B == 0) return SLK_OK;
    if (!paths || !lens || !move_row || !nrow || !qlen || !roff || !rows || !ops || !ops_off || !tb_status || !minus || !keep || !wstart ||
        !coff || !center_off || !letter_row || !status || !row_span || !window || !center || ldp < T || ldm < T || ldq < 0)
        return SLK_ERR_INVALID_ARG;
    hipLaunchKernelGGL(polish_read_windows_kernel, dim3((B + GE_WAVES - 1) / GE_WAVES), dim3(64 * GE_WAVES), 0, slk_stream(stream),
                       paths, ldp, lens, move_row, ldm, T, nrow, qlen, ldq, roff, rows, ops, ops_off, (long long)ops_bytes, tb_status,
                       minus, keep, wstart, coff, (long long)G, B, kmer_len, center_off, letter_row, status, row_span, window, center);
    return slk_launch_status();
}

extern "C" int slk_letter_edits_count(const int64_t *win_off, const int64_t *w0, const int64_t *w1, int nwin, long G, int kmer_len,
                                      int kinds, int margin, int64_t *ncand, int64_t *nkmer, slk_stream_t stream)
{
    if (!pg_edit_args(nwin, G, kmer_len, kinds, margin) || !ncand || !nkmer) return SLK_ERR_INVALID_ARG;
    if (nwin > 0 && (!win_off || !w0 || !w1)) return SLK_ERR_INVALID_ARG;
    hipLaunchKernelGGL(letter_edits_count_kernel, dim3(ge_blocks(nwin > 0 ? nwin : 1)), dim3(GE_THREADS), 0, slk_stream(stream), win_off,
                       w0, w1, nwin, (long long)G, kmer_len, kinds, margin, ncand, nkmer);
    return slk_launch_status();
}

extern "C" int slk_letter_edits_emit(const uint8_t *genome, long G, const int64_t *win_off, const int64_t *w0, const int64_t *w1,
                                     const int32_t *minus, int nwin, int kmer_len, int kinds, int margin, const int64_t *cand_off,
                                     int64_t ncand, int32_t *cand_pair, int32_t *cand_start, int32_t *cand_ndel,
                                     int64_t *cand_new_off, int64_t *cand_edit, slk_stream_t stream)
{
    if (!pg_edit_args(nwin, G, kmer_len, kinds, margin) || ncand < 0 || !cand_new_off) return SLK_ERR_INVALID_ARG;
    if (ncand > 0 && (nwin < 1 || !genome || !win_off || !w0 || !w1 || !minus || !cand_off || !cand_pair || !cand_start || !cand_ndel ||
                      !cand_edit))
        return SLK_ERR_INVALID_ARG;
    hipLaunchKernelGGL(letter_edits_emit_kernel, dim3(ge_blocks(ncand > 0 ? ncand : 1)), dim3(GE_THREADS), 0, slk_stream(stream), genome,
                       (long long)G, win_off, w0, w1, minus, nwin, kmer_len, kinds, margin, cand_off, (long long)ncand, cand_pair,
                       cand_start, cand_ndel, cand_new_off, cand_edit);
    return slk_launch_status();
}

extern "C" int slk_letter_edits_new(const uint8_t *genome, long G, const int64_t *win_off, const int64_t *w0, const int64_t *w1,
                                    const int32_t *minus, int nwin, int kmer_len, int blank, int kinds, int margin,
                                    const int64_t *cand_off, int64_t ncand, const int32_t *cand_start, const int64_t *cand_new_off,
                                    int64_t new_cap, int32_t *cand_new, slk_stream_t stream)
{
    if (!pg_edit_args(nwin, G, kmer_len, kinds, margin) || ncand < 0 || new_cap < 0 || blank < 0) return SLK_ERR_INVALID_ARG;
    if (ncand == 0) return SLK_OK;
    if (nwin < 1 || !genome || !win_off || !w0 || !w1 || !minus || !cand_off || !cand_start || !cand_new_off || !cand_new)
        return SLK_ERR_INVALID_ARG;
    hipLaunchKernelGGL(letter_edits_new_kernel, dim3(ge_blocks(ncand)), dim3(GE_THREADS), 0, slk_stream(stream), genome, (long long)G,
                       win_off, w0, w1, minus, nwin, kmer_len, blank, kinds, margin, cand_off, (long long)ncand, cand_start, cand_new_off,
                       (long long)new_cap, cand_new);
    return slk_launch_status();
}

extern "C" int slk_polish_window_kmers(const uint8_t *genome, long G, const int64_t *win_off, const int64_t *w0, const int64_t *w1,
                                       const int32_t *minus, int nwin, int kmer_len, int blank, const int64_t *pos_off, int64_t npos,
                                       int32_t *seq, slk_stream_t stream)
{
    if (nwin < 0 || G < 0 || !ge_klen(kmer_len) || blank < 0 || npos < 0) return SLK_ERR_INVALID_ARG;
    if (npos == 0) return SLK_OK;
    if (nwin < 1 || !genome || !win_off || !w0 || !w1 || !minus || !pos_off || !seq) return SLK_ERR_INVALID_ARG;
    hipLaunchKernelGGL(window_kmers_kernel, dim3(ge_blocks(npos)), dim3(GE_THREADS), 0, slk_stream(stream), genome, (long long)G, win_off,
                       w0, w1, minus, nwin, kmer_len, blank, pos_off, (long long)npos, seq);
    return slk_launch_status();
}

extern "C" int slk_polish_sum_gains_f64(const double *score, int nread, const double *ll_edit, const int32_t *cand_pair,
                                        const int64_t *cand_edit, const int64_t *order, int64_t ncand, int64_t region_start, int64_t P,
                                        double *gain, int32_t *support, slk_stream_t stream)
{
    if (nread < 0 || ncand < 0 || region_start < 0 || P < 0) return SLK_ERR_INVALID_ARG;
    if (ncand == 0 || P == 0) return SLK_OK;
    if (!score || !ll_edit || !cand_pair || !cand_edit || !order || !gain || !support) return SLK_ERR_INVALID_ARG;
    hipLaunchKernelGGL(polish_sum_gains_kernel, dim3(ge_blocks(ncand)), dim3(GE_THREADS), 0, slk_stream(stream), score, nread, ll_edit,
                       cand_pair, cand_edit, order, (long long)ncand, (long long)region_start, (long long)P, gain, support);
    return slk_launch_status();
}
