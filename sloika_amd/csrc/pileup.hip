// pileup.hip -- alignments on top of each other: per-position counts over the packed genome and the consensus they give, on the
// device (design/pileup.md; the quantities are defined in its section 1 and nowhere else).
//
// Five kernels, all integer.
//   pileup_columns_kernel  one wave per pair: checks the pair (its row and codes are device data and are NOT trusted), copies its
//                          columns into forward-strand order with all lanes and, when asked, moves every gap run as far to the
//                          front as its letters allow (left-normalisation).  Runs are found 64 columns at a time from ballots of
//                          the ORIGINAL codes -- the pass never changes a column at or behind the place it has reached, so the
//                          runs it meets are the runs of the input --; only the moving of one run is serial, in lane 0.
//   pileup_count_kernel    one wave per pair, 64 columns per step: a column's query / reference letter index is a ballot's
//                          population count below the lane plus a running base, an insertion's slot the distance to the last
//                          column that is none (clz on a ballot plus the run carried in).  Adds into the tables with integer
//                          atomics, which commute: the tables do not depend on the launch's shape or on any order.
//   pileup_call_kernel     one thread per position: winner, insertion letters, flags.
//   pileup_count_qual_kernel / pileup_call_qual_kernel: the same walk and the same call with a second pair of tables that hold sums
//                          of per-letter weights (a table of 256 bytes indexed by the letter's quality byte) instead of heads, and a
//                          quality per emitted letter (design/pileup.md section 9).
#include "common.h"

#define PILEUP_WAVES 4
#define PILEUP_MAX_LEN 65535                    // as the traceback: a pair has at most 2 * 65535 columns
#define PILEUP_CALL_THREADS 256

typedef unsigned long long u64;

__device__ __forceinline__ int pileup_letter_class(int c) { return c == 'A' ? 0 : c == 'C' ? 1 : c == 'G' ? 2 : c == 'T' ? 3 : 4; }

// Everything a pair's row, lengths and offsets must satisfy before a letter or a code of it is read (no loop bound depends on
// anything that has not passed here).  -> SLK_PILEUP_DONE or the reason.
__device__ __forceinline__ int pileup_check_row(const int *row, long long nq, long ldq, long long nr, long long o0, long long o1,
                                                long long ops_bytes, long long t0, long long G)
{
    const int qs = row[1], qe = row[2], rs = row[3], re = row[4];
    if (nq < 0 || nq > PILEUP_MAX_LEN || nq > ldq || nr < 0 || nr > PILEUP_MAX_LEN || qs < 0 || qe < qs || qe > nq || rs < 0 ||
        re < rs || re > nr)
        return SLK_PILEUP_BAD_SPAN;
    if (row[5] < 0 || row[6] < 0 || row[7] < 0 || row[8] < 0) return SLK_PILEUP_BAD_COUNT;
    if ((long long)row[5] + row[6] + row[7] != qe - qs || (long long)row[5] + row[6] + row[8] != re - rs) return SLK_PILEUP_BAD_SUM;
    const long long ncol = (long long)row[5] + row[6] + row[7] + row[8];       // (every count is at most 65535 from here on)
    if (o0 < 0 || o1 > ops_bytes || o1 - o0 != ncol) return SLK_PILEUP_OPS;
    if (t0 < 0 || t0 + (re - rs) > G) return SLK_PILEUP_POSITION;
    return SLK_PILEUP_DONE;
}

__global__ void __launch_bounds__(64 * PILEUP_WAVES) pileup_columns_kernel(
    const uint8_t *__restrict__ q, long ldq, const int32_t *__restrict__ qlen, const uint8_t *__restrict__ r,
    const int64_t *__restrict__ roff, const int32_t *__restrict__ rows, const uint8_t *__restrict__ ops,
    const int64_t *__restrict__ ops_off, long long ops_bytes, const int32_t *__restrict__ tb_status,
    const int32_t *__restrict__ minus, const uint8_t *__restrict__ keep, const int64_t *__restrict__ t0, long long G, int B,
    int normalise, uint8_t *fcodes, int32_t *__restrict__ status)
{
    const int lane = threadIdx.x & 63;
    const int b = blockIdx.x * PILEUP_WAVES + (threadIdx.x >> 6);
    if (b >= B) return;                                          // (whole waves: nothing below synchronises across waves)
    if (keep[b] == 0 || tb_status[b] != SLK_ALIGN_TB_DONE) {
        if (lane == 0) status[b] = SLK_PILEUP_SKIPPED;
        return;
    }
    int row[9];
#pragma unroll
    for (int k = 0; k < 9; k++) row[k] = rows[(size_t)b * 9 + k];
    const long long o0 = ops_off[b];
    int st = pileup_check_row(row, qlen[b], ldq, roff[b + 1] - roff[b], o0, ops_off[b + 1], ops_bytes, t0[b], G);
    if (st != SLK_PILEUP_DONE) {
        if (lane == 0) status[b] = st;
        return;
    }
    const int ncol = row[5] + row[6] + row[7] + row[8];
    const uint8_t *o = ops + o0;
    // the codes themselves: every byte a code, and as many of each kind as the row says
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
    if (bad) st = SLK_PILEUP_BAD_CODE;
    else if (cnt0 != row[5] || cnt1 != row[6] || cnt2 != row[7] || cnt3 != row[8]) st = SLK_PILEUP_CODE_COUNT;
    if (st != SLK_PILEUP_DONE) {
        if (lane == 0) status[b] = st;
        return;
    }
    const bool rev = minus[b] != 0;
    uint8_t *f = fcodes + o0;
    for (int cb = 0; cb < ncol; cb += 64) {                      // the forward view: '-' back to front
        const int col = cb + lane;
        if (col < ncol) f[col] = o[rev ? ncol - 1 - col : col];
    }
    if (lane == 0) status[b] = SLK_PILEUP_DONE;
    if (!normalise) return;
    __threadfence();                                             // every lane's stores, read by lane 0 below
    // Forward letters: Q(i) and R(j) as stored bytes (equality is the same thing under complement)
    const int n = row[2] - row[1], m = row[4] - row[3];
    const uint8_t *qb = q + (size_t)b * ldq, *rb = r + roff[b];
    const int qfirst = rev ? row[2] - 1 : row[1], rfirst = rev ? row[4] - 1 : row[3], step = rev ? -1 : 1;
    int ibase = 0, jbase = 0, last = -1;                         // letters consumed in front of the chunk; the code of column cb - 1
    for (int cb = 0; cb < ncol; cb += 64) {
        const int col = cb + lane;
        const int c = col < ncol ? (int)o[rev ? ncol - 1 - col : col] : 255;
        const u64 lt = (1ull << lane) - 1;
        const u64 mq = __ballot(c <= SLK_ALIGN_OP_INSERTION), mr = __ballot(c <= SLK_ALIGN_OP_MISMATCH || c == SLK_ALIGN_OP_DELETION);
        const int ci = ibase + __popcll(mq & lt), cj = jbase + __popcll(mr & lt);
        int prev = __shfl_up(c, 1);
        if (lane == 0) prev = last;
        const bool gap = c == SLK_ALIGN_OP_INSERTION || c == SLK_ALIGN_OP_DELETION;
        u64 starts = __ballot(gap && prev != c);
        while (starts) {                                         // at most 64 runs start in a chunk
            const int s = __ffsll((long long)starts) - 1;
            starts &= starts - 1;
            const int K = __shfl(c, s), i0 = __shfl(ci, s), j0 = __shfl(cj, s), a = cb + s;
            const u64 other = __ballot(c != K) & ~((1ull << s) - 1);
            int L;
            if (other) {
                L = __ffsll((long long)other) - 1 - s;
            } else {                                             // the run goes on behind this chunk (a column past the end is no K)
                L = 64 - s;
                for (int c2 = cb + 64; c2 < ncol; c2 += 64) {
                    const int col2 = c2 + lane;
                    const int x = col2 < ncol ? (int)o[rev ? ncol - 1 - col2 : col2] : 255;
                    const u64 o2 = __ballot(x != K);
                    if (o2) {
                        L += __ffsll((long long)o2) - 1;
                        break;
                    }
                    L += 64;
                }
            }
            if (lane == 0) {                                     // move the run: one column per iteration, at most `a` of them
                int aa = a, i = i0, j = j0;
                while (aa > 0 && i > 0 && j > 0) {
                    const int mv = f[aa - 1];
                    if (mv > SLK_ALIGN_OP_MISMATCH) break;
                    bool same;
                    if (K == SLK_ALIGN_OP_DELETION) {
                        if (j + L - 1 >= m) break;
                        same = rb[rfirst + step * (j - 1)] == rb[rfirst + step * (j + L - 1)];
                    } else {
                        if (i + L - 1 >= n) break;
                        same = qb[qfirst + step * (i - 1)] == qb[qfirst + step * (i + L - 1)];
                    }
                    if (!same) break;
                    f[aa - 1] = (uint8_t)K;
                    f[aa + L - 1] = (uint8_t)mv;
                    aa--;
                    i--;
                    j--;
                }
            }
        }
        ibase += __popcll(mq);
        jbase += __popcll(mr);
        last = __shfl(c, 63);
    }
}

// The walk of both count kernels.  WEIGHTED adds each column's weight (design/pileup.md section 9) into wcounts / wins beside the 1
// it adds into counts / ins; everything else is one text, so the plain tables of the two kernels cannot drift apart.
template <bool WEIGHTED>
__device__ __forceinline__ void pileup_count_body(
    const uint8_t *__restrict__ q, long ldq, const int32_t *__restrict__ qlen, const uint8_t *__restrict__ qual,
    const int64_t *__restrict__ roff, const int32_t *__restrict__ rows, const uint8_t *__restrict__ fcodes,
    const int64_t *__restrict__ ops_off, long long ops_bytes, const int32_t *__restrict__ status,
    const int32_t *__restrict__ minus, const int64_t *__restrict__ t0, long long G, int B, long long lo, long long hi, int S,
    const uint8_t *__restrict__ weights, int32_t *counts, int32_t *ins, int32_t *wcounts, int32_t *wins)
{
    const int lane = threadIdx.x & 63;
    const int b = blockIdx.x * PILEUP_WAVES + (threadIdx.x >> 6);
    if (b >= B || status[b] != SLK_PILEUP_DONE) return;
    int row[9];
#pragma unroll
    for (int k = 0; k < 9; k++) row[k] = rows[(size_t)b * 9 + k];
    const long long o0 = ops_off[b], tb = t0[b];
    // the status says the columns kernel accepted the pair; the row is checked again all the same, so that no read depends on it
    if (pileup_check_row(row, qlen[b], ldq, roff[b + 1] - roff[b], o0, ops_off[b + 1], ops_bytes, tb, G) != SLK_PILEUP_DONE) return;
    const int ncol = row[5] + row[6] + row[7] + row[8];
    const int n = row[2] - row[1], m = row[4] - row[3];
    const bool rev = minus[b] != 0;
    const uint8_t *qb = q + (size_t)b * ldq, *f = fcodes + o0;
    const uint8_t *vb = WEIGHTED ? qual + (size_t)b * ldq : nullptr;
    const int qfirst = rev ? row[2] - 1 : row[1], step = rev ? -1 : 1;
    int ibase = 0, jbase = 0, carry = 0;                         // carry: insertion columns at the end of the columns so far
    for (int cb = 0; cb < ncol; cb += 64) {
        const int col = cb + lane, nvalid = ncol - cb < 64 ? ncol - cb : 64;
        const bool in = col < ncol;
        const int c = in ? (int)f[col] : 255;
        const bool isins = c == SLK_ALIGN_OP_INSERTION, isdel = c == SLK_ALIGN_OP_DELETION;
        const bool qc = c <= SLK_ALIGN_OP_INSERTION, rc = c <= SLK_ALIGN_OP_MISMATCH || isdel;
        const u64 lt = (1ull << lane) - 1;
        const u64 mq = __ballot(qc), mr = __ballot(rc), nonins = __ballot(in && !isins), lower = nonins & lt;
        const int i = ibase + __popcll(mq & lt), j = jbase + __popcll(mr & lt);
        const int k = lower ? lane - (63 - __clzll((long long)lower)) - 1 : lane + carry;       // an insertion's slot in its run
        int cls = 4;
        if (qc && i < n) {
            cls = pileup_letter_class(qb[qfirst + step * i]);
            if (rev && cls < 4) cls = 3 - cls;
        }
        int w = 0;                                               // the column's weight (section 9): any byte indexes the table
        if (WEIGHTED) {
            if (qc) {
                if (i < n) w = weights[vb[qfirst + step * i]];
            } else if (isdel) {                                  // the lighter of the query letters on either side, those that exist
                const bool left = i - 1 >= 0 && i - 1 < n, right = i < n;
                const int wl = left ? (int)weights[vb[qfirst + step * (i - 1)]] : 0;
                const int wr = right ? (int)weights[vb[qfirst + step * i]] : 0;
                w = left && right ? (wl < wr ? wl : wr) : left ? wl : wr;
            }
        }
        if (rc && j < m) {
            const long long p = tb + j;
            if (p >= lo && p < hi) {
                int32_t *cp = counts + (size_t)(p - lo) * 8;
                atomicAdd(cp + (isdel ? 5 : cls), 1);
                if (j < m - 1) atomicAdd(cp + 7, 1);
                if (WEIGHTED && w) {
                    int32_t *wp = wcounts + (size_t)(p - lo) * 8;
                    atomicAdd(wp + (isdel ? 5 : cls), w);
                    if (j < m - 1) atomicAdd(wp + 7, w);
                }
            }
        } else if (isins && j > 0) {                             // (an insertion in front of the first reference letter: nowhere)
            const long long p = tb + j - 1;
            if (p >= lo && p < hi) {
                if (k == 0) atomicAdd(counts + (size_t)(p - lo) * 8 + 6, 1);
                if (k < S) atomicAdd(ins + ((size_t)(p - lo) * S + k) * 5 + cls, 1);
                if (WEIGHTED && w) {
                    if (k == 0) atomicAdd(wcounts + (size_t)(p - lo) * 8 + 6, w);
                    if (k < S) atomicAdd(wins + ((size_t)(p - lo) * S + k) * 5 + cls, w);
                }
            }
        }
        carry = nonins ? nvalid - 1 - (63 - __clzll((long long)nonins)) : carry + nvalid;
        ibase += __popcll(mq);
        jbase += __popcll(mr);
    }
}

__global__ void __launch_bounds__(64 * PILEUP_WAVES) pileup_count_kernel(
    const uint8_t *__restrict__ q, long ldq, const int32_t *__restrict__ qlen, const int64_t *__restrict__ roff,
    const int32_t *__restrict__ rows, const uint8_t *__restrict__ fcodes,
    const int64_t *__restrict__ ops_off, long long ops_bytes, const int32_t *__restrict__ status,
    const int32_t *__restrict__ minus, const int64_t *__restrict__ t0, long long G, int B, long long lo, long long hi, int S,
    int32_t *counts, int32_t *ins)
{
    pileup_count_body<false>(q, ldq, qlen, nullptr, roff, rows, fcodes, ops_off, ops_bytes, status, minus, t0, G, B, lo, hi, S, nullptr,
                             counts, ins, nullptr, nullptr);
}

// The same walk with the Phred-weighted tables beside the plain ones.  The 256-byte weight table is read through the cache: every
// wave reads the same 256 bytes, and LDS would cost a barrier in a kernel whose waves otherwise never meet.
__global__ void __launch_bounds__(64 * PILEUP_WAVES) pileup_count_qual_kernel(
    const uint8_t *__restrict__ q, long ldq, const int32_t *__restrict__ qlen, const uint8_t *__restrict__ qual,
    const int64_t *__restrict__ roff, const int32_t *__restrict__ rows, const uint8_t *__restrict__ fcodes,
    const int64_t *__restrict__ ops_off, long long ops_bytes, const int32_t *__restrict__ status,
    const int32_t *__restrict__ minus, const int64_t *__restrict__ t0, long long G, int B, long long lo, long long hi, int S,
    const uint8_t *__restrict__ weights, int32_t *counts, int32_t *ins, int32_t *wcounts, int32_t *wins)
{
    pileup_count_body<true>(q, ldq, qlen, qual, roff, rows, fcodes, ops_off, ops_bytes, status, minus, t0, G, B, lo, hi, S, weights,
                            counts, ins, wcounts, wins);
}

__global__ void __launch_bounds__(PILEUP_CALL_THREADS) pileup_call_kernel(
    const int32_t *__restrict__ counts, const int32_t *__restrict__ ins, const uint8_t *__restrict__ genome, long long lo, long long P,
    int S, int min_depth, uint8_t *__restrict__ letters, uint8_t *__restrict__ nlet, uint8_t *__restrict__ flags)
{
    const long long p = (long long)blockIdx.x * PILEUP_CALL_THREADS + threadIdx.x;
    if (p >= P) return;
    int cn[8];
    {
        const int4 a = reinterpret_cast<const int4 *>(counts)[p * 2], c = reinterpret_cast<const int4 *>(counts)[p * 2 + 1];
        cn[0] = a.x; cn[1] = a.y; cn[2] = a.z; cn[3] = a.w;
        cn[4] = c.x; cn[5] = c.y; cn[6] = c.z; cn[7] = c.w;
    }
    const int refb = genome[lo + p], refc = pileup_letter_class(refb);
    uint8_t *out = letters + (size_t)p * (1 + S);
    const long long depth = (long long)cn[0] + cn[1] + cn[2] + cn[3] + cn[4] + cn[5];
    int nl = 0, fl = 0;
    if (depth < min_depth || (cn[0] | cn[1] | cn[2] | cn[3] | cn[5]) == 0) {
        out[nl++] = (uint8_t)refb;
        fl = SLK_PILEUP_FLAG_LOW;
    } else {
        // candidates in the order A, C, G, T, deletion; the reference letter's class wins a tie it is part of
        int best = -1, w = 0;
#pragma unroll
        for (int k = 0; k < 5; k++) {
            const int v = cn[k < 4 ? k : 5];
            if (v > best) { best = v; w = k; }
        }
        if (refc < 4 && cn[refc] == best) w = refc;
        if (w < 4) out[nl++] = (uint8_t)("ACGT"[w]);
        if (w == 4 || w != refc) fl |= SLK_PILEUP_FLAG_CHANGED;  // (w == 4 is the deletion, refc == 4 a letter that is none of A C G T)
        const int32_t *ip = ins + (size_t)p * S * 5;
        for (int k = 0; k < S; k++) {
            int nk = ip[k * 5 + 4], mx = 0, am = 0;
#pragma unroll
            for (int x = 0; x < 4; x++) {
                const int v = ip[k * 5 + x];
                nk += v;
                if (v > mx) { mx = v; am = x; }
            }
            if (!(2ll * nk > cn[7] && mx > 0)) break;
            out[nl++] = (uint8_t)("ACGT"[am]);
            fl |= SLK_PILEUP_FLAG_INSERTED;
        }
    }
    for (int k = nl; k < 1 + S; k++) out[k] = 0;
    nlet[p] = (uint8_t)nl;
    flags[p] = (uint8_t)fl;
}

// The weighted call of section 9: the winner by weight, a quality per emitted letter.  `depth` is the plain one of 1.4.
__global__ void __launch_bounds__(PILEUP_CALL_THREADS) pileup_call_qual_kernel(
    const int32_t *__restrict__ counts, const int32_t *__restrict__ wcounts, const int32_t *__restrict__ wins,
    const uint8_t *__restrict__ genome, long long lo, long long P, int S, int min_depth, int qmax, uint8_t *__restrict__ letters,
    uint8_t *__restrict__ nlet, uint8_t *__restrict__ flags, uint8_t *__restrict__ letq, uint8_t *__restrict__ posq)
{
    const long long p = (long long)blockIdx.x * PILEUP_CALL_THREADS + threadIdx.x;
    if (p >= P) return;
    int cn[8], wn[8];
    {
        const int4 a = reinterpret_cast<const int4 *>(counts)[p * 2], c = reinterpret_cast<const int4 *>(counts)[p * 2 + 1];
        cn[0] = a.x; cn[1] = a.y; cn[2] = a.z; cn[3] = a.w;
        cn[4] = c.x; cn[5] = c.y; cn[6] = c.z; cn[7] = c.w;
        const int4 d = reinterpret_cast<const int4 *>(wcounts)[p * 2], e = reinterpret_cast<const int4 *>(wcounts)[p * 2 + 1];
        wn[0] = d.x; wn[1] = d.y; wn[2] = d.z; wn[3] = d.w;
        wn[4] = e.x; wn[5] = e.y; wn[6] = e.z; wn[7] = e.w;
    }
    const int refb = genome[lo + p], refc = pileup_letter_class(refb);
    uint8_t *out = letters + (size_t)p * (1 + S), *oq = letq + (size_t)p * (1 + S);
    const long long depth = (long long)cn[0] + cn[1] + cn[2] + cn[3] + cn[4] + cn[5];
    int nl = 0, fl = 0, pq = 0;
    if (depth < min_depth || (wn[0] | wn[1] | wn[2] | wn[3] | wn[5]) == 0) {
        oq[nl] = 0;
        out[nl++] = (uint8_t)refb;
        fl = SLK_PILEUP_FLAG_LOW;
    } else {
        int best = -1, w = 0;
#pragma unroll
        for (int k = 0; k < 5; k++) {
            const int v = wn[k < 4 ? k : 5];
            if (v > best) { best = v; w = k; }
        }
        if (refc < 4 && wn[refc] == best) w = refc;
        int next = wn[4];                                        // the runner-up: the other four candidates and `other`
#pragma unroll
        for (int k = 0; k < 5; k++) {
            const int v = wn[k < 4 ? k : 5];
            if (k != w && v > next) next = v;
        }
        pq = best - next < qmax ? best - next : qmax;            // (both lie in [0, 2^31): the difference cannot wrap)
        if (pq < 0) pq = 0;
        if (w < 4) {
            oq[nl] = (uint8_t)pq;
            out[nl++] = (uint8_t)("ACGT"[w]);
        }
        if (w == 4 || w != refc) fl |= SLK_PILEUP_FLAG_CHANGED;
        const int32_t *ip = wins + (size_t)p * S * 5;
        for (int k = 0; k < S; k++) {
            long long nk = ip[k * 5 + 4];
            int mx = 0, am = 0;
#pragma unroll
            for (int x = 0; x < 4; x++) {
                const int v = ip[k * 5 + x];
                nk += v;
                if (v > mx) { mx = v; am = x; }
            }
            if (!(2ll * nk > (long long)wn[7] && mx > 0)) break;
            const long long lead = 2ll * mx - (long long)wn[7];
            oq[nl] = (uint8_t)(lead < 0 ? 0 : lead > qmax ? qmax : lead);
            out[nl++] = (uint8_t)("ACGT"[am]);
            fl |= SLK_PILEUP_FLAG_INSERTED;
        }
    }
    for (int k = nl; k < 1 + S; k++) {
        out[k] = 0;
        oq[k] = 0;
    }
    nlet[p] = (uint8_t)nl;
    flags[p] = (uint8_t)fl;
    posq[p] = (uint8_t)pq;
}

extern "C" int slk_pileup_columns_u8(const uint8_t *q, long ldq, const int32_t *qlen, const uint8_t *r, const int64_t *roff,
                                     const int32_t *rows, const uint8_t *ops, const int64_t *ops_off, size_t ops_bytes,
                                     const int32_t *tb_status, const int32_t *minus, const uint8_t *keep, const int64_t *t0, long G,
                                     int B, int normalise, uint8_t *fcodes, int32_t *status, slk_stream_t stream)
{
    if (B < 0 || G < 0) return SLK_ERR_INVALID_ARG;
    if (B == 0) return SLK_OK;
    if (!q || !qlen || !r || !roff || !rows || !ops || !ops_off || !tb_status || !minus || !keep || !t0 || !fcodes || !status ||
        ldq < 0 || fcodes == ops)
        return SLK_ERR_INVALID_ARG;
    hipLaunchKernelGGL(pileup_columns_kernel, dim3((B + PILEUP_WAVES - 1) / PILEUP_WAVES), dim3(64 * PILEUP_WAVES), 0,
                       slk_stream(stream), q, ldq, qlen, r, roff, rows, ops, ops_off, (long long)ops_bytes, tb_status, minus, keep, t0,
                       (long long)G, B, normalise, fcodes, status);
    return slk_launch_status();
}

extern "C" int slk_pileup_count_u8(const uint8_t *q, long ldq, const int32_t *qlen, const int64_t *roff, const int32_t *rows,
                                   const uint8_t *fcodes, const int64_t *ops_off, size_t ops_bytes,
                                   const int32_t *status, const int32_t *minus, const int64_t *t0, long G, int B, long lo, long hi,
                                   int max_ins, int32_t *counts, int32_t *ins, slk_stream_t stream)
{
    if (B < 0 || G < 0 || lo < 0 || hi < lo || hi > G || max_ins < 1 || max_ins > SLK_PILEUP_MAX_INS) return SLK_ERR_INVALID_ARG;
    if (B == 0 || hi == lo) return SLK_OK;
    if (!q || !qlen || !roff || !rows || !fcodes || !ops_off || !status || !minus || !t0 || !counts || !ins || ldq < 0)
        return SLK_ERR_INVALID_ARG;
    hipLaunchKernelGGL(pileup_count_kernel, dim3((B + PILEUP_WAVES - 1) / PILEUP_WAVES), dim3(64 * PILEUP_WAVES), 0,
                       slk_stream(stream), q, ldq, qlen, roff, rows, fcodes, ops_off, (long long)ops_bytes, status, minus, t0,
                       (long long)G, B, (long long)lo, (long long)hi, max_ins, counts, ins);
    return slk_launch_status();
}

extern "C" int slk_pileup_call_u8(const int32_t *counts, const int32_t *ins, const uint8_t *genome, long G, long lo, long hi,
                                  int max_ins, int min_depth, uint8_t *letters, uint8_t *nlet, uint8_t *flags, slk_stream_t stream)
{
    if (G < 0 || lo < 0 || hi < lo || hi > G || max_ins < 1 || max_ins > SLK_PILEUP_MAX_INS) return SLK_ERR_INVALID_ARG;
    if (hi == lo) return SLK_OK;
    if (!counts || !ins || !genome || !letters || !nlet || !flags || ((uintptr_t)counts & 15)) return SLK_ERR_INVALID_ARG;
    const long long P = hi - lo;
    hipLaunchKernelGGL(pileup_call_kernel, dim3((unsigned)((P + PILEUP_CALL_THREADS - 1) / PILEUP_CALL_THREADS)),
                       dim3(PILEUP_CALL_THREADS), 0, slk_stream(stream), counts, ins, genome, (long long)lo, P, max_ins, min_depth,
                       letters, nlet, flags);
    return slk_launch_status();
}

extern "C" int slk_pileup_count_qual_u8(const uint8_t *q, long ldq, const int32_t *qlen, const uint8_t *qual, const int64_t *roff,
                                        const int32_t *rows, const uint8_t *fcodes, const int64_t *ops_off, size_t ops_bytes,
                                        const int32_t *status, const int32_t *minus, const int64_t *t0, long G, int B, long lo,
                                        long hi, int max_ins, const uint8_t *weights, int32_t *counts, int32_t *ins,
                                        int32_t *wcounts, int32_t *wins, slk_stream_t stream)
{
    if (B < 0 || G < 0 || lo < 0 || hi < lo || hi > G || max_ins < 1 || max_ins > SLK_PILEUP_MAX_INS) return SLK_ERR_INVALID_ARG;
    if (B == 0 || hi == lo) return SLK_OK;
    if (!q || !qlen || !qual || !roff || !rows || !fcodes || !ops_off || !status || !minus || !t0 || !weights || !counts || !ins ||
        !wcounts || !wins || ldq < 0)
        return SLK_ERR_INVALID_ARG;
    hipLaunchKernelGGL(pileup_count_qual_kernel, dim3((B + PILEUP_WAVES - 1) / PILEUP_WAVES), dim3(64 * PILEUP_WAVES), 0,
                       slk_stream(stream), q, ldq, qlen, qual, roff, rows, fcodes, ops_off, (long long)ops_bytes, status, minus, t0,
                       (long long)G, B, (long long)lo, (long long)hi, max_ins, weights, counts, ins, wcounts, wins);
    return slk_launch_status();
}

extern "C" int slk_pileup_call_qual_u8(const int32_t *counts, const int32_t *ins, const int32_t *wcounts, const int32_t *wins,
                                       const uint8_t *genome, long G, long lo, long hi, int max_ins, int min_depth, int qmax,
                                       uint8_t *letters, uint8_t *nlet, uint8_t *flags, uint8_t *letq, uint8_t *posq,
                                       slk_stream_t stream)
{
    if (G < 0 || lo < 0 || hi < lo || hi > G || max_ins < 1 || max_ins > SLK_PILEUP_MAX_INS || qmax < 1 || qmax > 93)
        return SLK_ERR_INVALID_ARG;
    if (hi == lo) return SLK_OK;
    if (!counts || !ins || !wcounts || !wins || !genome || !letters || !nlet || !flags || !letq || !posq ||
        ((uintptr_t)counts & 15) || ((uintptr_t)wcounts & 15))
        return SLK_ERR_INVALID_ARG;
    const long long P = hi - lo;
    hipLaunchKernelGGL(pileup_call_qual_kernel, dim3((unsigned)((P + PILEUP_CALL_THREADS - 1) / PILEUP_CALL_THREADS)),
                       dim3(PILEUP_CALL_THREADS), 0, slk_stream(stream), counts, wcounts, wins, genome, (long long)lo, P, max_ins,
                       min_depth, qmax, letters, nlet, flags, letq, posq);
    return slk_launch_status();
}
