// align_traceback.hip -- the alignment columns behind a row of align.hip (CIGAR / SAM / error profiles), on the device
// (design/align_traceback.md).
//
// align.hip keeps no traceback: a row says where the alignment starts and ends and how many insertions I and deletions D it has.
// That is enough to find the path again cheaply: relative to its start cell the alignment never leaves the diagonals
// i - j in [-D, +I], so a second DP over that band alone -- anchored at the start cell, H(0,0) = 0, every other border and everything
// outside the band -inf, no max(0, .) clamp, the same tie rules -- gives the cells of the path their full-matrix values and every
// other cell a value that is no greater, and therefore walks back the same operations (the proof is in the design note).
//
// Fill.  One wave per pair, ALIGN_TB_WAVES pairs per workgroup, no LDS, no barrier.  Diagonal d = i - j + D, 0 <= d < W = I + D + 1;
// lane l owns the C consecutive diagonals l C .. l C + C - 1 (H, E, F of the latest cell of each in registers; C = 4, 8, 12 or 16,
// the least with 64 C >= W: W <= 1024).  The cells of an anti-diagonal i + j = s lie on the diagonals of one parity and need only s - 1 (diagonals
// d -+ 1, the other parity) and s - 2 (the same diagonal), so the update is in place: iteration p updates the even diagonals (step
// u = 2 p + ubase, u = s + D, ubase = D & ~1), then the odd ones (u + 1).  Across lanes only the two edge diagonals move (four
// cross-lane moves per iteration).  The letters a lane needs are two sliding byte windows -- the query window slides towards lower
// lanes, the reversed reference window towards higher ones, one byte per iteration -- so one XOR compares all of a lane's pairs
// of letters; lane 63 / lane 0 take their new letter from a register loaded 64 iterations at a time, as align.hip does.
//
// Bits.  Per cell 4 bits: bits 0-1 where H comes from (0 diagonal with equal letters, 3 diagonal with different letters, 1 E, 2 F),
// bit 2 E opened (from H), bit 3 F opened.  A lane packs the nibbles of eight consecutive iterations of one diagonal into one
// register and stores whole dwords (16 bytes at a time): no two lanes ever write the same location.  Dword (p >> 3) * Wst + d of the
// pair's slice, nibble p & 7, Wst = W rounded up to 4.
//
// Walk.  Lane 0 walks back from (n', m') in state H, one column per iteration of a loop bounded by the number of columns, and
// writes the codes from the back.  The row comes from device memory and is not trusted: see slk_align_traceback_batch_u8.
#include "common.h"

#define ALIGN_TB_WAVES 4
#define ALIGN_TB_MAX_BAND 1024                  // 64 lanes * 16 diagonals
#define ALIGN_TB_MAX_LEN 65535
#define ALIGN_TB_MAX_SCORE 16384
#define ALIGN_TB_NEG (-(1 << 30))               // NEG + 65535 * 16384 < 0: a value that started at -inf never reaches a real one

typedef unsigned long long u64;

// iterations of the fill and dwords of a pair's slice; n, m: the spans, D: deletions, W: the band
__host__ __device__ static inline int align_tb_iterations(int n, int m, int D) { return ((n + m + D - (D & ~1)) >> 1) + 1; }
__host__ __device__ static inline int align_tb_wst(int W) { return (W + 3) & ~3; }
__host__ __device__ static inline long long align_tb_dwords(int n, int m, int D, int W)
{
    return (long long)((align_tb_iterations(n, m, D) + 7) >> 3) * align_tb_wst(W);
}

// One fill over the band; returns H(n, m).  qs / rs point at the first aligned letter of either sequence.
template <int C>
__device__ __forceinline__ int align_tb_fill(const uint8_t *__restrict__ qs, const uint8_t *__restrict__ rs, const int n, const int m,
                                             const int D, const int W, const int sa, const int sb, const int oe, const int se,
                                             uint32_t *ws, const int lane)
{
    constexpr int HB = C / 2;                                    // letters per window
    constexpr u64 WMASK = HB == 8 ? ~0ull : ((1ull << (8 * HB)) - 1);
    const int half = (D + 1) >> 1, dlo = D >> 1;                 // lane 0's even cell of iteration p is (p - half, p + dlo)
    const int NP = align_tb_iterations(n, m, D), Wst = align_tb_wst(W);
    const int d0 = lane * C;
    int H[C], E[C], F[C];
    uint32_t acc[C];
#pragma unroll
    for (int c = 0; c < C; c++) {
        H[c] = E[c] = F[c] = ALIGN_TB_NEG;
        acc[c] = 0;
    }
    // byte b of qw: the query letter of row i0 + b; byte b of rw: the reference letter of column j0 - b
    u64 qw = 0, rw = 0;
#pragma unroll
    for (int b = 0; b < HB; b++) {
        const int i = lane * HB + b - half, j = dlo - lane * HB - b;
        qw |= (u64)((unsigned)(i - 1) < (unsigned)n ? qs[i - 1] : 0) << (8 * b);
        rw |= (u64)((unsigned)(j - 1) < (unsigned)m ? rs[j - 1] : 0) << (8 * b);
    }
    int cq = 0, cr = 0;                                          // lane 63's / lane 0's new letters of 64 iterations, one per lane

    // a lane's cells of one phase are b = 0 .. C / 2 - 1 (row rising, column falling with b): the ones inside the rectangle and the
    // band are a range blo <= b <= blo + span, and the origin is one b (or none)
    auto cell = [&](const int c, const int b, const int blo, const unsigned span, const int borg, const int hm, const int fm,
                    const int hp, const int ep, const unsigned x, const int sh) {
        const int eo = hp - oe, ex = ep - se;                    // E: from (i, j - 1), diagonal d + 1
        const bool eopen = eo >= ex;
        int e = eopen ? eo : ex;
        const int fo = hm - oe, fx = fm - se;                    // F: from (i - 1, j), diagonal d - 1
        const bool fopen = fo >= fx;
        int f = fopen ? fo : fx;
        const bool eq = x == 0;
        int h = H[c] + (eq ? sa : -sb);                          // H[c] still holds (i - 1, j - 1)
        unsigned src = eq ? 0u : 3u;
        if (e > h) { h = e; src = 1; }
        if (f > h) { h = f; src = 2; }
        unsigned nib = src | (eopen ? 4u : 0u) | (fopen ? 8u : 0u);
        const bool inside = (unsigned)(b - blo) <= span;
        const int anchor = b == borg ? 0 : ALIGN_TB_NEG;         // borders: -inf except H(0, 0) = 0
        H[c] = inside ? max(h, ALIGN_TB_NEG) : anchor;
        E[c] = inside ? max(e, ALIGN_TB_NEG) : ALIGN_TB_NEG;
        F[c] = inside ? max(f, ALIGN_TB_NEG) : ALIGN_TB_NEG;
        nib = inside ? nib : 0u;
        acc[c] |= nib << sh;
    };

    for (int p = 0; p < NP; p++) {
        if ((p & 63) == 0) {
            const int i = p + lane - half + 64 * HB, j = p + lane + dlo + 1;
            cq = (unsigned)(i - 1) < (unsigned)n ? (int)qs[i - 1] : 0;
            cr = (unsigned)(j - 1) < (unsigned)m ? (int)rs[j - 1] : 0;
        }
        const int fq = __builtin_amdgcn_readlane(cq, p & 63), fr = __builtin_amdgcn_readlane(cr, p & 63);
        const int i0 = p - half + lane * HB, j0 = p + dlo - lane * HB;
        const int sh = 4 * (p & 7);
        {                                                        // even diagonals: cell c at (i0 + c / 2, j0 - c / 2)
            int lH = __shfl_up(H[C - 1], 1), lF = __shfl_up(F[C - 1], 1);
            if (lane == 0) lH = lF = ALIGN_TB_NEG;
            const u64 x = qw ^ rw;
            // 1 <= i0 + b <= n, 1 <= j0 - b <= m, d0 + 2 b <= W - 1
            const int blo = max(1 - i0, j0 - m), bhi = min(min(n - i0, j0 - 1), (W - 1 - d0) >> 1);
            const unsigned span = bhi >= blo ? (unsigned)(bhi - blo) : 0u;
            const int lo = bhi >= blo ? blo : C, borg = i0 + j0 == 0 ? j0 : -1;    // the origin: i0 + b = 0 = j0 - b
#pragma unroll
            for (int c = 0; c < C; c += 2)
                cell(c, c / 2, lo, span, borg, c ? H[c - 1] : lH, c ? F[c - 1] : lF, H[c + 1], E[c + 1],
                     (unsigned)(x >> (8 * (c / 2))) & 0xffu, sh);
        }
        {
            int nq = __shfl_down((int)(qw & 0xff), 1);
            if (lane == 63) nq = fq;
            qw = (qw >> 8) | ((u64)(unsigned)nq << (8 * (HB - 1)));
        }
        {                                                        // odd diagonals: cell c at (i0 + (c + 1) / 2, j0 - (c - 1) / 2)
            int rH = __shfl_down(H[0], 1), rE = __shfl_down(E[0], 1);
            if (lane == 63) rH = rE = ALIGN_TB_NEG;
            const u64 x = qw ^ rw;
            // 1 <= i0 + b + 1 <= n, 1 <= j0 - b <= m, d0 + 2 b + 1 <= W - 1
            const int blo = max(-i0, j0 - m), bhi = min(min(n - i0 - 1, j0 - 1), (W - 2 - d0) >> 1);
            const unsigned span = bhi >= blo ? (unsigned)(bhi - blo) : 0u;
            const int lo = bhi >= blo ? blo : C, borg = i0 + j0 == -1 ? j0 : -1;   // the origin: i0 + b + 1 = 0 = j0 - b
#pragma unroll
            for (int c = 1; c < C; c += 2)
                cell(c, c / 2, lo, span, borg, H[c - 1], F[c - 1], c + 1 < C ? H[c + 1] : rH, c + 1 < C ? E[c + 1] : rE,
                     (unsigned)(x >> (8 * (c / 2))) & 0xffu, sh);
        }
        {
            int nr = __shfl_up((int)((rw >> (8 * (HB - 1))) & 0xff), 1);
            if (lane == 0) nr = fr;
            rw = ((rw << 8) | (u64)(unsigned)nr) & WMASK;
        }
        if ((p & 7) == 7 || p == NP - 1) {                       // eight iterations of every diagonal: whole dwords, 16 bytes a store
            uint32_t *row = ws + (size_t)(p >> 3) * Wst + d0;
#pragma unroll
            for (int g = 0; g < C; g += 4) {
                if (d0 + g < Wst) *reinterpret_cast<uint4 *>(row + g) = make_uint4(acc[g], acc[g + 1], acc[g + 2], acc[g + 3]);
                acc[g] = acc[g + 1] = acc[g + 2] = acc[g + 3] = 0;
            }
        }
    }
    const int dend = n - m + D;                                  // the end cell's diagonal; its last update was the end cell
    int v = 0;
#pragma unroll
    for (int c = 0; c < C; c++)
        if (d0 + c == dend) v = H[c];
    return __shfl(v, dend / C);
}

__global__ void __launch_bounds__(64 * ALIGN_TB_WAVES) align_traceback_kernel(
    const uint8_t *__restrict__ q, long ldq, const int32_t *__restrict__ qlen, const uint8_t *__restrict__ r,
    const int64_t *__restrict__ roff, int B, int sa, int sb, int so, int se, const int32_t *__restrict__ rows, uint8_t *ops,
    const int64_t *__restrict__ ops_off, long long ops_bytes, uint8_t *workspace, const int64_t *__restrict__ ws_off,
    long long workspace_bytes, int32_t *__restrict__ status)
{
    const int lane = threadIdx.x & 63;
    const int b = blockIdx.x * ALIGN_TB_WAVES + (threadIdx.x >> 6);
    if (b >= B) return;                                          // (whole waves: nothing below synchronises across waves)
    int row[9];
#pragma unroll
    for (int k = 0; k < 9; k++) row[k] = rows[(size_t)b * 9 + k];
    int st = SLK_ALIGN_TB_DONE;
    const int qs = row[1], qe = row[2], rs = row[3], re = row[4], I = row[7], D = row[8];
    int n = 0, m = 0, W = 0;
    long long ncol = 0, o0 = 0, w0 = 0;
    if (row[0] <= 0) {
        st = SLK_ALIGN_TB_EMPTY;
    } else {
        const long long nq = qlen[b], nr = roff[b + 1] - roff[b];
        if (nq < 0 || nq > ALIGN_TB_MAX_LEN || nq > ldq || nr < 0 || nr > ALIGN_TB_MAX_LEN || qs < 0 || qe < qs || qe > nq || rs < 0 ||
            re < rs || re > nr) {
            st = SLK_ALIGN_TB_BAD_SPAN;
        } else if (row[5] < 0 || row[6] < 0 || I < 0 || D < 0) {
            st = SLK_ALIGN_TB_BAD_COUNT;
        } else if ((long long)row[5] + row[6] + I != qe - qs || (long long)row[5] + row[6] + D != re - rs) {
            st = SLK_ALIGN_TB_BAD_SUM;                           // (from here on every count is at most 65535)
        } else if (I + D + 1 > ALIGN_TB_MAX_BAND) {
            st = SLK_ALIGN_TB_BAND;
        } else {
            n = qe - qs;
            m = re - rs;
            W = I + D + 1;
            ncol = (long long)row[5] + row[6] + I + D;
            w0 = ws_off[b];
            o0 = ops_off[b];
            const long long w1 = ws_off[b + 1], o1 = ops_off[b + 1];
            if (w0 < 0 || (w0 & 15) || w1 > workspace_bytes || w1 - w0 < 4 * align_tb_dwords(n, m, D, W)) st = SLK_ALIGN_TB_WORKSPACE;
            else if (o0 < 0 || o1 > ops_bytes || o1 - o0 != ncol) st = SLK_ALIGN_TB_OPS;
        }
    }
    if (st != SLK_ALIGN_TB_DONE) {                               // nothing was read but the row and the offsets, nothing is written
        if (lane == 0) status[b] = st;
        return;
    }
    uint32_t *ws = reinterpret_cast<uint32_t *>(workspace + w0);
    const uint8_t *qb = q + (size_t)b * ldq + qs, *rb = r + roff[b] + rs;
    const int oe = so + se;
    int hend;                                                    // the fewest diagonals per lane that cover the band (wave-uniform)
    if (W <= 64 * 4) hend = align_tb_fill<4>(qb, rb, n, m, D, W, sa, sb, oe, se, ws, lane);
    else if (W <= 64 * 8) hend = align_tb_fill<8>(qb, rb, n, m, D, W, sa, sb, oe, se, ws, lane);
    else if (W <= 64 * 12) hend = align_tb_fill<12>(qb, rb, n, m, D, W, sa, sb, oe, se, ws, lane);
    else hend = align_tb_fill<16>(qb, rb, n, m, D, W, sa, sb, oe, se, ws, lane);
    __threadfence();                                             // every lane's stores, read by lane 0
    if (lane != 0) return;
    if (hend != row[0]) {
        status[b] = SLK_ALIGN_TB_SCORE;
        return;
    }
    const int ubase = D & ~1, Wst = align_tb_wst(W);
    uint8_t *o = ops + o0;
    int i = n, j = m, state = 0;                                 // 0 H, 1 E, 2 F
    int cd = -1, cblk = -1;
    uint32_t cw = 0;
    bool ok = true;
    for (long long c = ncol - 1; c >= 0; c--) {                  // one column per iteration
        const int d = i - j + D;
        if (i < 0 || j < 0 || (unsigned)d >= (unsigned)W) { ok = false; break; }
        const int p = (i + j + D - ubase) >> 1, blk = p >> 3;
        if (d != cd || blk != cblk) {                            // a run of diagonal moves stays in one dword for eight columns
            cw = ws[(size_t)blk * Wst + d];
            cd = d;
            cblk = blk;
        }
        const unsigned nib = (cw >> (4 * (p & 7))) & 15u, src = nib & 3u;
        const int mv = state ? state : (src == 3u ? 0 : (int)src);
        if (mv == 0) {
            o[c] = src == 3u ? SLK_ALIGN_OP_MISMATCH : SLK_ALIGN_OP_MATCH;
            i--;
            j--;
        } else if (mv == 1) {
            o[c] = SLK_ALIGN_OP_DELETION;
            state = (nib & 4u) ? 0 : 1;
            j--;
        } else {
            o[c] = SLK_ALIGN_OP_INSERTION;
            state = (nib & 8u) ? 0 : 2;
            i--;
        }
    }
    status[b] = ok && i == 0 && j == 0 && state == 0 ? SLK_ALIGN_TB_DONE : SLK_ALIGN_TB_WALK;
}

__device__ __forceinline__ int align_letter_class(int c) { return c == 'A' ? 0 : c == 'C' ? 1 : c == 'G' ? 2 : c == 'T' ? 3 : 4; }

// maximal runs of the code X that end in this lane's column: their length bin (0..15), or -1; `carry`: the run open at the chunk's start
__device__ __forceinline__ int align_run_bin(bool in, int op, int next, int X, int lane, int nvalid, int &carry)
{
    const bool isx = in && op == X;
    const u64 other = __ballot(in && !isx), lower = other & ((1ull << lane) - 1);
    const int len = lower ? lane - (63 - __clzll((long long)lower)) : lane + 1 + carry;
    carry = other ? nvalid - 1 - (63 - __clzll((long long)other)) : carry + nvalid;
    return isx && next != X ? (len < 16 ? len : 16) - 1 : -1;
}

// One wave per pair.  Lane k holds entry k of the pair's profile (lanes 0..3 also entries 64..67); every count is a ballot's
// population count, so nothing is added in memory.
__global__ void __launch_bounds__(64 * ALIGN_TB_WAVES) align_profile_kernel(
    const uint8_t *__restrict__ q, long ldq, const uint8_t *__restrict__ r, const int64_t *__restrict__ roff,
    const int32_t *__restrict__ rows, const uint8_t *__restrict__ ops, const int64_t *__restrict__ ops_off,
    const int32_t *__restrict__ status, int B, int32_t *__restrict__ profile)
{
    const int lane = threadIdx.x & 63;
    const int b = blockIdx.x * ALIGN_TB_WAVES + (threadIdx.x >> 6);
    if (b >= B) return;
    int acc0 = 0, acc1 = 0;
    const int qs = rows[(size_t)b * 9 + 1], qe = rows[(size_t)b * 9 + 2], rs = rows[(size_t)b * 9 + 3], re = rows[(size_t)b * 9 + 4];
    const long long o0 = ops_off[b], ncol = ops_off[b + 1] - o0, nr = roff[b + 1] - roff[b];
    if (status[b] == SLK_ALIGN_TB_DONE && rows[(size_t)b * 9] > 0 && qs >= 0 && qe >= qs && qe <= ldq && rs >= 0 && re >= rs &&
        re <= nr && o0 >= 0 && ncol >= 0 && ncol <= 2 * ALIGN_TB_MAX_LEN) {
        const uint8_t *qb = q + (size_t)b * ldq + qs, *rb = r + roff[b] + rs, *o = ops + o0;
        const int n = qe - qs, m = re - rs;
        int qbase = 0, rbase = 0, carry_i = 0, carry_d = 0;
        for (int cb = 0; cb < (int)ncol; cb += 64) {
            const int col = cb + lane, nvalid = (int)ncol - cb < 64 ? (int)ncol - cb : 64;
            const bool in = col < (int)ncol;
            const int op = in ? (int)o[col] : 255, next = col + 1 < (int)ncol ? (int)o[col + 1] : 255;
            const bool qc = op == SLK_ALIGN_OP_MATCH || op == SLK_ALIGN_OP_MISMATCH || op == SLK_ALIGN_OP_INSERTION;
            const bool rc = op == SLK_ALIGN_OP_MATCH || op == SLK_ALIGN_OP_MISMATCH || op == SLK_ALIGN_OP_DELETION;
            const u64 mq = __ballot(qc), mr = __ballot(rc), lt = (1ull << lane) - 1;
            const int qi = qbase + __popcll(mq & lt), ri = rbase + __popcll(mr & lt);   // the letters this column consumes
            const int qcls = !qc ? 5 : qi < n ? align_letter_class(qb[qi]) : 4;
            const int rcls = !rc ? 5 : ri < m ? align_letter_class(rb[ri]) : 4;
            const int key = qc || rc ? qcls * 6 + rcls : -1;
#pragma unroll
            for (int k = 0; k < 35; k++) {
                const int cnt = __popcll(__ballot(key == k));
                if (lane == k) acc0 += cnt;
            }
            const int bi = align_run_bin(in, op, next, SLK_ALIGN_OP_INSERTION, lane, nvalid, carry_i);
            const int bd = align_run_bin(in, op, next, SLK_ALIGN_OP_DELETION, lane, nvalid, carry_d);
#pragma unroll
            for (int k = 0; k < 16; k++) {
                const int ci = __popcll(__ballot(bi == k)), cd = __popcll(__ballot(bd == k));
                if (lane == 36 + k) acc0 += ci;
                if (k < 12 && lane == 52 + k) acc0 += cd;
                if (k >= 12 && lane == k - 12) acc1 += cd;
            }
            qbase += __popcll(mq);
            rbase += __popcll(mr);
        }
    }
    profile[(size_t)b * SLK_ALIGN_PROFILE_LEN + lane] = acc0;
    if (lane < SLK_ALIGN_PROFILE_LEN - 64) profile[(size_t)b * SLK_ALIGN_PROFILE_LEN + 64 + lane] = acc1;
}

extern "C" int slk_align_traceback_max_band(void) { return ALIGN_TB_MAX_BAND; }

extern "C" size_t slk_align_traceback_workspace_bytes(int q_span, int r_span, int insertion, int deletion)
{
    if (q_span < 0 || r_span < 0 || insertion < 0 || deletion < 0 || q_span > ALIGN_TB_MAX_LEN || r_span > ALIGN_TB_MAX_LEN ||
        insertion > q_span || deletion > r_span || q_span - insertion != r_span - deletion ||
        insertion + deletion + 1 > ALIGN_TB_MAX_BAND)
        return 0;
    return (size_t)(4 * align_tb_dwords(q_span, r_span, deletion, insertion + deletion + 1));
}

static bool align_tb_scores_ok(int match, int mismatch, int gap_open, int gap_extend)
{
    return match >= 1 && gap_extend >= 1 && mismatch >= 0 && gap_open >= 0 && match <= ALIGN_TB_MAX_SCORE &&
           mismatch <= ALIGN_TB_MAX_SCORE && gap_open <= ALIGN_TB_MAX_SCORE && gap_extend <= ALIGN_TB_MAX_SCORE;
}

extern "C" int slk_align_traceback_batch_u8(const uint8_t *q, long ldq, const int32_t *qlen, const uint8_t *r, const int64_t *roff,
                                            int B, int match, int mismatch, int gap_open, int gap_extend, const int32_t *rows,
                                            uint8_t *ops, const int64_t *ops_off, size_t ops_bytes, void *workspace,
                                            const int64_t *ws_off, size_t workspace_bytes, int32_t *status, slk_stream_t stream)
{
    if (B < 0 || !align_tb_scores_ok(match, mismatch, gap_open, gap_extend)) return SLK_ERR_INVALID_ARG;
    if (B == 0) return SLK_OK;
    if (!q || !qlen || !r || !roff || !rows || !ops || !ops_off || !workspace || !ws_off || !status || ldq < 0)
        return SLK_ERR_INVALID_ARG;
    if ((uintptr_t)workspace & 15) return SLK_ERR_WORKSPACE;
    hipLaunchKernelGGL(align_traceback_kernel, dim3((B + ALIGN_TB_WAVES - 1) / ALIGN_TB_WAVES), dim3(64 * ALIGN_TB_WAVES), 0,
                       slk_stream(stream), q, ldq, qlen, r, roff, B, match, mismatch, gap_open, gap_extend, rows, ops, ops_off,
                       (long long)ops_bytes, (uint8_t *)workspace, ws_off, (long long)workspace_bytes, status);
    return slk_launch_status();
}

extern "C" int slk_align_error_profile_u8(const uint8_t *q, long ldq, const uint8_t *r, const int64_t *roff, const int32_t *rows,
                                          const uint8_t *ops, const int64_t *ops_off, const int32_t *status, int B, int32_t *profile,
                                          slk_stream_t stream)
{
    if (B < 0) return SLK_ERR_INVALID_ARG;
    if (B == 0) return SLK_OK;
    if (!q || !r || !roff || !rows || !ops || !ops_off || !status || !profile || ldq < 0) return SLK_ERR_INVALID_ARG;
    hipLaunchKernelGGL(align_profile_kernel, dim3((B + ALIGN_TB_WAVES - 1) / ALIGN_TB_WAVES), dim3(64 * ALIGN_TB_WAVES), 0,
                       slk_stream(stream), q, ldq, r, roff, rows, ops, ops_off, status, B, profile);
    return slk_launch_status();
}
