// align.hip -- batched local alignment with affine gaps (Smith-Waterman-Gotoh) of called bases against their references, and the
// reverse complement of packed sequences (design/align.md).
//
// Stands for misc/align.py:22 (the scores handed to `bwa mem`: -A 1 -B 2 -O 2 -E 1) and :70-133 (samacc: the counts pysam reads off
// every alignment's CIGAR and NM tag).  This is the OPTIMUM under those scores, not bwa's seed-and-extend heuristic.
//
//     E[i][j] = max(H[i][j-1] - O - E, E[i][j-1] - E)          consumes r[j]: a deletion
//     F[i][j] = max(H[i-1][j] - O - E, F[i-1][j] - E)          consumes q[i]: an insertion
//     H[i][j] = max(0, H[i-1][j-1] + (q[i] == r[j] ? A : -B), E[i][j], F[i][j])
//
// Ties: in E and F the opening wins over the extension; in H the diagonal wins, then E, then F; a best of <= 0 empties the cell;
// the alignment ends in the cell of greatest H, smallest i, then smallest j.
//
// No traceback matrix: every DP value carries one 64-bit word  q_start:16 | r_start:16 | insertions:16 | mismatches:16  inherited
// from the predecessor the rules pick (an empty cell (i, j) carries q_start = i, r_start = j and no counts: whatever passes it starts
// behind it).  Matches and deletions follow from where the alignment ends.  16 bits per field is the packing's limit: 65535 letters.
//
// One wave per pair, ALIGN_WAVES pairs per workgroup, no LDS, no barrier.  Lane l owns ALIGN_C consecutive reference columns (H of
// the row above, F and their carried words in registers); query rows run through the lanes as a systolic pipeline: at step t lane
// l computes row t - l and hands its right-hand column (H, E, carried words, the row's letter) to lane l + 1.  A reference wider
// than one pass of ALIGN_P = 64 * ALIGN_C columns is walked in passes; the column between two passes (H, E and their carried words
// for every query row) lives in the pair's workspace in global memory, written by lane 63 and read back 64 rows at a time.
#include "genome_edits.h"                       // the complement

#define ALIGN_C 8
#define ALIGN_P (64 * ALIGN_C)
#define ALIGN_WAVES 4
#define ALIGN_MAX_LEN 65535
#define ALIGN_MAX_SCORE 16384                  // 65535 * 16384 < 2^30: no int32 score overflows, nor does NEG - extend
#define ALIGN_NEG (-(1 << 30))
#define ALIGN_INS_ONE 0x10000ull
#define ALIGN_MM_ONE 1ull


__device__ __forceinline__ u64 align_fresh(int i, int j) { return (u64)(((unsigned)i << 16) | (unsigned)j) << 32; }

__device__ __forceinline__ u64 align_up1(u64 v)
{
    return ((u64)(unsigned)__shfl_up((int)(v >> 32), 1) << 32) | (unsigned)__shfl_up((int)(unsigned)v, 1);
}

__device__ __forceinline__ u64 align_xor(u64 v, int mask)
{
    return ((u64)(unsigned)__shfl_xor((int)(v >> 32), mask) << 32) | (unsigned)__shfl_xor((int)(unsigned)v, mask);
}

// value of wave-uniform lane `src`
__device__ __forceinline__ int align_lane(int v, int src) { return __builtin_amdgcn_readlane(v, src); }
__device__ __forceinline__ u64 align_lane(u64 v, int src)
{
    return ((u64)(unsigned)align_lane((int)(v >> 32), src) << 32) | (unsigned)align_lane((int)(unsigned)v, src);
}

__global__ void __launch_bounds__(64 * ALIGN_WAVES) align_local_kernel(
    const uint8_t *__restrict__ q, long ldq, const int32_t *__restrict__ qlen, const uint8_t *__restrict__ r,
    const int64_t *__restrict__ roff, int B, int max_qlen, int max_rlen, int sa, int sb, int so, int se,
    int32_t *__restrict__ out, u64 *__restrict__ workspace)
{
    const int lane = threadIdx.x & 63;
    const int b = blockIdx.x * ALIGN_WAVES + (threadIdx.x >> 6);
    if (b >= B) return;                                          // (whole waves: nothing below synchronises across waves)
    const int n = qlen[b];
    const long long r0 = roff[b], mlong = roff[b + 1] - r0;
    int32_t *o = out + (size_t)b * 9;
    if (n < 0 || n > max_qlen || mlong < 0 || mlong > max_rlen) { // refused, never truncated: the caller's bounds were wrong
        if (lane < 9) o[lane] = lane == 0 ? -1 : 0;
        return;
    }
    const int m = (int)mlong;
    const uint8_t *qb = q + (size_t)b * ldq, *rb = r + r0;
    // the boundary column between passes, one entry per query row: [0] H:32|E:32  [1] H's carried word  [2] E's carried word
    u64 *ws = workspace ? workspace + (size_t)b * 3 * max_qlen : nullptr;
    const int oe = so + se;
    const int npass = (m + ALIGN_P - 1) / ALIGN_P;
    const int nstep = n > 0 ? n + 63 : 0;

    u64 bkey = 0xffffffffull, bcar = 0;                          // key = H:32 | 65535 - i:16 | 65535 - j:16; only H >= 1 beats the start

    for (int pass = 0; pass < npass; pass++) {
        const int pb = pass * ALIGN_P, c0 = pb + lane * ALIGN_C;   // 0-based index of this lane's first column
        const bool more = pass + 1 < npass;
        int rl[ALIGN_C], hp[ALIGN_C], ff[ALIGN_C];
        u64 hc[ALIGN_C], fc[ALIGN_C];
#pragma unroll
        for (int k = 0; k < ALIGN_C; k++) {
            rl[k] = c0 + k < m ? (int)rb[c0 + k] : 256;          // no query byte equals 256
            hp[k] = 0;                                           // row 0: H = 0, F = -inf
            hc[k] = align_fresh(0, c0 + k + 1);
            ff[k] = ALIGN_NEG;
            fc[k] = 0;
        }
        const int nv = m - c0;                                   // columns k < nv exist
        int hd = 0;                                              // H[i-1][c0] (1-based column c0: left of this lane's first)
        u64 hdc = align_fresh(0, c0);
        int oh = 0, oE = ALIGN_NEG, oq = 0;                      // what this lane hands to its right-hand neighbour
        u64 ohc = 0, oEc = 0;
        int cq = 0;                                              // 64 rows of lane 0's input, one row per lane
        u64 che = 0, chc = 0, cec = 0;

        for (int t = 0; t < nstep; t++) {
            if ((t & 63) == 0) {
                const int row = t + lane;                        // 0-based query index; its DP row is row + 1
                const bool in = row < n;
                cq = in ? (int)qb[row] : 0;
                if (pass == 0 || !in) {                          // column 0: H = 0, E = -inf
                    che = (u64)(unsigned)ALIGN_NEG;
                    chc = align_fresh(row + 1, 0);
                    cec = 0;
                } else {
                    che = ws[row];
                    chc = ws[(size_t)max_qlen + row];
                    cec = ws[2 * (size_t)max_qlen + row];
                }
            }
            int lh = __shfl_up(oh, 1), lE = __shfl_up(oE, 1), lq = __shfl_up(oq, 1);
            u64 lhc = align_up1(ohc), lEc = align_up1(oEc);
            {
                const int s = t & 63;
                const u64 he = align_lane(che, s), c1 = align_lane(chc, s), c2 = align_lane(cec, s);
                const int q0 = align_lane(cq, s);
                if (lane == 0) {
                    lh = (int)(he >> 32);
                    lE = (int)(unsigned)he;
                    lhc = c1;
                    lEc = c2;
                    lq = q0;
                }
            }
            const int qi = t - lane;
            if ((unsigned)qi < (unsigned)n) {
                const int i = qi + 1;
                const int nhd = lh;                              // next row's diagonal input
                const u64 nhdc = lhc;
                const unsigned pos = ((unsigned)(65535 - i) << 16) | (unsigned)(65535 - (c0 + 1));
#pragma unroll
                for (int k = 0; k < ALIGN_C; k++) {
                    const int eo = lh - oe, ex = lE - se;
                    const bool eopen = eo >= ex;
                    const int E = eopen ? eo : ex;
                    const u64 Ec = eopen ? lhc : lEc;
                    const int fo = hp[k] - oe, fx = ff[k] - se;
                    const bool fopen = fo >= fx;
                    const int F = fopen ? fo : fx;
                    const u64 Fc = (fopen ? hc[k] : fc[k]) + ALIGN_INS_ONE;
                    const bool eq = lq == rl[k];
                    int h = hd + (eq ? sa : -sb);
                    u64 c = hdc + (eq ? 0ull : ALIGN_MM_ONE);
                    if (E > h) { h = E; c = Ec; }
                    if (F > h) { h = F; c = Fc; }
                    if (h <= 0) { h = 0; c = align_fresh(i, c0 + k + 1); }
                    hd = hp[k];
                    hdc = hc[k];
                    hp[k] = h;
                    hc[k] = c;
                    ff[k] = F;
                    fc[k] = Fc;
                    lh = h;
                    lhc = c;
                    lE = E;
                    lEc = Ec;
                    const u64 key = ((u64)(unsigned)h << 32) | (pos - k);
                    if (k < nv && key > bkey) { bkey = key; bcar = c; }
                }
                hd = nhd;
                hdc = nhdc;
                oh = lh;
                ohc = lhc;
                oE = lE;
                oEc = lEc;
                oq = lq;
                if (more && lane == 63) {
                    ws[qi] = ((u64)(unsigned)lh << 32) | (unsigned)lE;
                    ws[(size_t)max_qlen + qi] = lhc;
                    ws[2 * (size_t)max_qlen + qi] = lEc;
                }
            }
        }
        if (more) __threadfence();                               // lane 63's column, read by every lane of the next pass
    }

#pragma unroll
    for (int mask = 32; mask >= 1; mask >>= 1) {
        const u64 ok = align_xor(bkey, mask), oc = align_xor(bcar, mask);
        if (ok > bkey) { bkey = ok; bcar = oc; }
    }
    if (lane == 0) {
        const int score = (int)(bkey >> 32);
        int res[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
        if (score > 0) {
            const int qe = 65535 - (int)((bkey >> 16) & 0xffff), re = 65535 - (int)(bkey & 0xffff);
            const int qs = (int)(bcar >> 48), rs = (int)((bcar >> 32) & 0xffff);
            const int ins = (int)((bcar >> 16) & 0xffff), mm = (int)(bcar & 0xffff);
            const int match = qe - qs - mm - ins;
            res[0] = score; res[1] = qs; res[2] = qe; res[3] = rs; res[4] = re;
            res[5] = match; res[6] = mm; res[7] = ins; res[8] = re - rs - match - mm;
        }
#pragma unroll
        for (int k = 0; k < 9; k++) o[k] = res[k];
    }
}

__global__ void __launch_bounds__(256) revcomp_kernel(const uint8_t *__restrict__ seq, const int64_t *__restrict__ off,
                                                      uint8_t *__restrict__ out)
{
    const long long s = off[blockIdx.x], len = off[blockIdx.x + 1] - s;
    for (long long k = (long long)blockIdx.y * 256 + threadIdx.x; k < len; k += (long long)gridDim.y * 256) {
        const uint8_t c = seq[s + len - 1 - k];
        out[s + k] = (uint8_t)ge_comp(c);
    }
}

extern "C" int slk_align_pass_width(void) { return ALIGN_P; }

static bool align_shape_ok(int B, int max_qlen, int max_rlen)
{
    return B >= 0 && max_qlen >= 0 && max_rlen >= 0 && max_qlen <= ALIGN_MAX_LEN && max_rlen <= ALIGN_MAX_LEN;
}

extern "C" size_t slk_align_local_workspace_bytes(int B, int max_qlen, int max_rlen)
{
    if (!align_shape_ok(B, max_qlen, max_rlen) || max_rlen <= ALIGN_P) return 0;
    return (size_t)B * 3 * sizeof(u64) * (size_t)max_qlen;
}

extern "C" int slk_align_local_batch_u8(const uint8_t *q, long ldq, const int32_t *qlen, const uint8_t *r, const int64_t *roff, int B,
                                        int max_qlen, int max_rlen, int match, int mismatch, int gap_open, int gap_extend,
                                        int32_t *out, void *workspace, size_t workspace_bytes, slk_stream_t stream)
{
    if (!align_shape_ok(B, max_qlen, max_rlen)) return SLK_ERR_INVALID_ARG;           // beyond the packing: refused, not truncated
    if (match < 1 || gap_extend < 1 || mismatch < 0 || gap_open < 0 || match > ALIGN_MAX_SCORE || mismatch > ALIGN_MAX_SCORE ||
        gap_open > ALIGN_MAX_SCORE || gap_extend > ALIGN_MAX_SCORE)
        return SLK_ERR_INVALID_ARG;
    if (B == 0) return SLK_OK;
    if (!q || !qlen || !r || !roff || !out || ldq < max_qlen) return SLK_ERR_INVALID_ARG;
    const size_t need = slk_align_local_workspace_bytes(B, max_qlen, max_rlen);
    if (need && (!workspace || workspace_bytes < need || ((uintptr_t)workspace & 7))) return SLK_ERR_WORKSPACE;
    hipLaunchKernelGGL(align_local_kernel, dim3((B + ALIGN_WAVES - 1) / ALIGN_WAVES), dim3(64 * ALIGN_WAVES), 0, slk_stream(stream), q,
                       ldq, qlen, r, roff, B, max_qlen, max_rlen, match, mismatch, gap_open, gap_extend, out,
                       need ? (u64 *)workspace : nullptr);
    return slk_launch_status();
}

extern "C" int slk_revcomp_u8(const uint8_t *seq, const int64_t *off, int B, long max_len, uint8_t *out, slk_stream_t stream)
{
    if (B < 0 || max_len < 0) return SLK_ERR_INVALID_ARG;
    if (B == 0 || max_len == 0) return SLK_OK;
    if (!seq || !off || !out || seq == out) return SLK_ERR_INVALID_ARG;
    const long blocks = (max_len + 255) / 256;
    hipLaunchKernelGGL(revcomp_kernel, dim3(B, (unsigned)(blocks < 64 ? blocks : 64)), dim3(256), 0, slk_stream(stream), seq, off, out);
    return slk_launch_status();
}
