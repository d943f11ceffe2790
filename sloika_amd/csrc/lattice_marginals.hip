// lattice_marginals.hip -- state marginals over the lattice decode.viterbi maximises over (row f8, design/lattice_marginals.md).
//
// The lattice is sloika/decode.py:60-82: nbase^klen k-mer states, per row a stay (weight p[i][0]), a step (p[i][1+s]) or a skip
// (exp(-skip_pen) p[i][1+s]) into state s.  slk_viterbi_kmer_f32 takes the maximum over its paths; this kernel takes, beside the
// same maximum, the SUM: Z, the share gamma[i][s] of Z that passes through s at row i, and per position of the called path the
// largest gamma of its state over its dwell (conf).  The weights are the float32 values of slk_prepare_post_f32 widened to float64;
// the 1e-10 inside decode.viterbi's log belongs to the max-plus scores only.
//
// One workgroup per chunk, thread j owns the nbase to-states j*nbase .. j*nbase + nbase - 1 (they share their step predecessors
// {a * N/nbase + j}), two passes:
//   pass 1, rows ascending: the float32 max-plus recursion of viterbi_forward_kernel (decode.hip: same operations in the same
//     order, so the same bits) with a traceback byte per state, and beside it the float64 sum recursion.  Both read the group
//     values of a row once: N/nbase step groups (max, argmax, sum), N/nbase^2 skip groups.  The scaled forward row goes to the
//     workspace.
//   pass 2, rows descending: the backward variables stay in the registers of the thread that owns the state (a state's backward
//     value needs its own old value and two group sums: the successors by step are nbase consecutive states, by skip nbase^2);
//     the same loop walks the traceback: the thread that owns the path's state forms its gamma, keeps the dwell's maximum, on a
//     move writes the position and hands the predecessor over through LDS at the row's barrier.
// Scaling (design/forward_score.md 4): exact powers of two, one row late.  Behind the first barrier of row t wave 0 adds up the
// step-group sums it finds in LDS (the total of stored row t - 1) and publishes d[t + 1] = its binary exponent - d[t]; row t + 1
// multiplies its result by 2^-d[t + 1].  Subtracting d[t] accounts for what row t takes off after that total was taken, which keeps
// a stored row's total within two rows' factors of [1/2, 1).  A power of two is exact: the scaling rounds nothing, the exponents
// add up in an integer, and log Z takes one log per chunk.
// A chunk's bits depend on nothing but the chunk: not on the batch, not on whether gamma is written.
//
// Two kernels share the row step (lm_step_groups, lm_row_update): lattice_marginals_kernel keeps every forward row in the workspace,
// lattice_marginals_ckpt_kernel (at the end of the file) every K-th one and recomputes the rows between in LDS -- the same bits.
#include "common.h"
#include "post_transform.h"

#define LM_STAY 255
#define LM_MAX_STATES 1024
#define LM_MAX_GROUPS 256            /* N / nbase */
#define LM_MAX_GROUPS2 64            /* N / nbase^2 */

static bool lm_dims(int nbase, int klen, int *nkmer_out)
{
    if (klen < 3 || (nbase != 4 && nbase != 5)) return false;
    long nk = 1;
    for (int i = 0; i < klen; i++) {
        nk *= nbase;
        if (nk > LM_MAX_STATES) return false;
    }
    *nkmer_out = (int)nk;
    return true;
}

// workspace: [B][T][N] float64 forward rows | [B][T] float64 conf, right aligned | [B][T] int32 row exponents | [B][T] int32 path and
// [B][T] int32 move rows, right aligned | [B][T][N] traceback bytes
struct lm_workspace {
    double *fwd, *conf;
    int32_t *dexp, *path, *row;
    uint8_t *tb;
};

static size_t lm_carve(void *base, int T, int B, int nkmer, lm_workspace *w)
{
    const size_t rows = (size_t)B * T, cells = rows * nkmer;
    uint8_t *p = static_cast<uint8_t *>(base);
    size_t off = 0;
    w->fwd = reinterpret_cast<double *>(p + off);   off += 8 * cells;
    w->conf = reinterpret_cast<double *>(p + off);  off += 8 * rows;
    w->dexp = reinterpret_cast<int32_t *>(p + off); off += 4 * rows;
    w->path = reinterpret_cast<int32_t *>(p + off); off += 4 * rows;
    w->row = reinterpret_cast<int32_t *>(p + off);  off += 4 * rows;
    w->tb = p + off;                                off += cells;
    return (off + 255) & ~(size_t)255;
}

extern "C" size_t slk_viterbi_marginals_workspace_bytes(int T, int B, int nbase, int klen)
{
    int nkmer;
    if (T < 1 || B < 1 || !lm_dims(nbase, klen, &nkmer)) return 0;
    lm_workspace w;
    return lm_carve(nullptr, T, B, nkmer, &w);
}

// the same sum on every lane of wave 0: lane l adds the entries l, l + 64, .., then a butterfly (a + b = b + a at every level)
__device__ __forceinline__ double lm_wave_total(const double *vals, int n, int lane)
{
    double tot = 0.0;
    for (int k = lane; k < n; k += 64) tot += vals[k];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) tot += __shfl_xor(tot, o);
    return tot;
}

// binary exponent of a row total (0 for a total that is zero or not finite: nothing to scale by)
__device__ __forceinline__ int lm_exponent(double tot)
{
    int e = 0;
    if (tot > 0.0 && tot < INFINITY) (void)frexp(tot, &e);
    return e;
}

// ---- the row step of pass 1, shared by the stored-row and the checkpointed kernel (which runs it a second time in pass 2): one text,
// so that both contract and order their floating-point expressions alike and a chunk's bits do not depend on the kernel ----

// In front of the row's first barrier: thread jj's step group of the previous row -- maximum over a (first max wins: np.argmax,
// decode.py:67-68) and sum -- kept, and published for the skip groups.
template <int NB>
__device__ __forceinline__ void lm_step_groups(const float *v, const double *alpha, float *stepmax, int *steparg, double *ssum, int jj,
                                               int nrem1, bool active, float &sstep, int &sarg, double &ss)
{
    sstep = v[jj];
    sarg = 0;
    ss = alpha[jj];
#pragma unroll
    for (int a = 1; a < NB; a++) {
        const float c = v[a * nrem1 + jj];
        if (c > sstep) { sstep = c; sarg = a; }
        ss += alpha[a * nrem1 + jj];
    }
    if (active) { stepmax[jj] = sstep; steparg[jj] = sarg; ssum[jj] = ss; }
}

// Behind it: the skip group -- maximum over ab = a*NB + b (first max in ab order wins, decode.py:72-73) and sum -- then the row's
// max-plus scores and scaled forward values of thread jj's states into v / alpha and, with their traceback codes, to the caller.
// dt: the exponent this row is scaled by.
template <int NB>
__device__ __forceinline__ void lm_row_update(float *v, double *alpha, const float *stepmax, const int *steparg, const double *ssum,
                                              int jj, int j2, int nrem2, bool active, float skip_pen, double eskip, float sstep, int sarg,
                                              double ss, const float (&lp)[NB], float lp0, const double (&pd)[NB], double pd0, int dt,
                                              double (&arow)[NB], uint8_t (&codes)[NB])
{
    float kbest = stepmax[j2];
    int karg = steparg[j2] * NB;
    double ks = ssum[j2];
#pragma unroll
    for (int bb = 1; bb < NB; bb++) {
        const float c = stepmax[bb * nrem2 + j2];
        const int key = steparg[bb * nrem2 + j2] * NB + bb;
        if (c > kbest || (c == kbest && key < karg)) { kbest = c; karg = key; }
        ks += ssum[bb * nrem2 + j2];
    }
    const float sskip = kbest - skip_pen;                       // decode.py:72
    const float mx = fmaxf(sstep, sskip);
    const int code = sstep > sskip ? sarg : NB + karg;          // decode.py:76 (tie -> skip)
    const double inflow = ss + eskip * ks;
    if (active) {
#pragma unroll
        for (int c = 0; c < NB; c++) {
            const int s = jj * NB + c;
            const float nv = lp[c] + mx;                        // decode.py:75
            const float stay = v[s] + lp0;                      // decode.py:80
            const bool move = nv > stay;                        // decode.py:81 (tie -> stay)
            codes[c] = move ? (uint8_t)code : (uint8_t)LM_STAY;
            v[s] = move ? nv : stay;
            const double a = ldexp(alpha[s] * pd0 + pd[c] * inflow, -dt);
            alpha[s] = a;
            arow[c] = a;
        }
    }
}

// thread jj's NB traceback codes of one row, at dst = the row's bytes + jj * NB: one word for nbase 4
template <int NB>
__device__ __forceinline__ void lm_store_codes(uint8_t *dst, const uint8_t (&codes)[NB])
{
    if constexpr (NB == 4) {
        *reinterpret_cast<uint32_t *>(dst) = (uint32_t)codes[0] | ((uint32_t)codes[1] << 8) | ((uint32_t)codes[2] << 16) |
                                             ((uint32_t)codes[3] << 24);
    } else {
#pragma unroll
        for (int c = 0; c < NB; c++) dst[c] = codes[c];
    }
}

template <int NB>
__device__ __forceinline__ void lm_load_codes(const uint8_t *src, int (&codes)[NB])
{
    if constexpr (NB == 4) {
        const uint32_t w = *reinterpret_cast<const uint32_t *>(src);
#pragma unroll
        for (int c = 0; c < NB; c++) codes[c] = (int)((w >> (8 * c)) & 0xff);
    } else {
#pragma unroll
        for (int c = 0; c < NB; c++) codes[c] = (int)src[c];
    }
}

template <int NB>
__global__ void __launch_bounds__(256) lattice_marginals_kernel(const float *__restrict__ post, int T, int B, int nkmer, float skip_pen,
                                                                double eskip, int mode, float min_prob, float one_m,
                                                                const int32_t *__restrict__ lens, lm_workspace ws,
                                                                float *__restrict__ score_out, int32_t *__restrict__ path_out,
                                                                int32_t *__restrict__ len_out, int32_t *__restrict__ move_row,
                                                                double *__restrict__ conf, double *__restrict__ logz,
                                                                float *__restrict__ gamma)
{
    constexpr int NB2 = NB * NB;
    __shared__ double alpha[LM_MAX_STATES];                    // scaled forward values of the previous row
    __shared__ double ssum[LM_MAX_GROUPS];                     // their sums over the step groups
    __shared__ double g1[2][LM_MAX_GROUPS];                    // pass 2: sums over the step successors, by row parity
    __shared__ double g2[2][LM_MAX_GROUPS2];                   //         and over the skip successors
    __shared__ double sh_tot;
    __shared__ float v[LM_MAX_STATES];                         // max-plus scores of the previous row
    __shared__ float stepmax[LM_MAX_GROUPS];
    __shared__ int steparg[LM_MAX_GROUPS];
    __shared__ float redv[4];
    __shared__ int redi[4];
    __shared__ int sh_d[2], sh_cur[2], sh_pos[2];

    const int Tpad = T;                                        // row stride of everything per chunk; T = this chunk's own length
    const int b = blockIdx.x, j = threadIdx.x, nt = blockDim.x;
    if (lens) T = min(max(lens[b], 1), Tpad);
    const int nrem1 = nkmer / NB, nrem2 = nkmer / NB2;
    const bool active = j < nrem1;
    const int jj = active ? j : 0, j2 = jj / NB;
    const size_t ld = (size_t)nkmer + 1;
    const float *pb = post + (size_t)b * ld;
    const size_t tstride = (size_t)B * ld;
    double *fwd = ws.fwd + (size_t)b * Tpad * nkmer;
    uint8_t *tbb = ws.tb + (size_t)b * Tpad * nkmer;
    int32_t *dexp = ws.dexp + (size_t)b * Tpad;

    auto lpx = [&](float r) { return log_post_val(r, mode, min_prob, one_m); };                       // slk_log_post_f32's bits
    auto px = [&](float r) { return (double)(mode == SLK_POST_RAW ? prepare_post_val(r, min_prob, one_m) : r); };

    // ---- pass 1 -------------------------------------------------------------------------------------------------------------------
    float raw[NB], raw0 = 0.0f;
#pragma unroll
    for (int c = 0; c < NB; c++) raw[c] = pb[1 + jj * NB + c];
    if (active) {
#pragma unroll
        for (int c = 0; c < NB; c++) {
            const int s = jj * NB + c;
            const double a = px(raw[c]);                       // row 0: state s weighs p[0][1 + s]
            v[s] = lpx(raw[c]);                                // decode.py:57
            alpha[s] = a;
            fwd[s] = a;
        }
    }
    if (j == 0) {
        dexp[0] = 0;
        sh_d[1] = 0;                                           // row 1 is not scaled: no total is known yet
    }
    if (T > 1) {
#pragma unroll
        for (int c = 0; c < NB; c++) raw[c] = pb[tstride + 1 + jj * NB + c];
        raw0 = pb[tstride];
    }
    __syncthreads();
    int d_cur = 0, d_sum = 0;                                  // wave 0: the exponent row t applies, the sum of those applied
    for (int t = 1; t < T; t++) {
        float nxt[NB], nxt0 = 0.0f;
        if (t + 1 < T) {                                       // the next row, one step ahead of its use
            const float *pn = pb + (size_t)(t + 1) * tstride;
#pragma unroll
            for (int c = 0; c < NB; c++) nxt[c] = pn[1 + jj * NB + c];
            nxt0 = pn[0];
        } else {
#pragma unroll
            for (int c = 0; c < NB; c++) nxt[c] = 0.0f;
        }
        float sstep;
        int sarg;
        double ss;
        lm_step_groups<NB>(v, alpha, stepmax, steparg, ssum, jj, nrem1, active, sstep, sarg, ss);
        float lp[NB];
        double pd[NB];
#pragma unroll
        for (int c = 0; c < NB; c++) { lp[c] = lpx(raw[c]); pd[c] = px(raw[c]); }
        const float lp0 = lpx(raw0);
        const double pd0 = px(raw0);
        const int dt = sh_d[t & 1];                            // written during row t - 1, behind that row's first barrier
        __syncthreads();
        if (j < 64) {
            // wave 0: the total of row t - 1 as it lies in LDS; row t + 1 scales by its exponent less what row t takes off
            d_sum += d_cur;
            d_cur = lm_exponent(lm_wave_total(ssum, nrem1, j)) - d_cur;
            if (j == 0) {
                sh_d[(t + 1) & 1] = d_cur;
                dexp[t] = dt;
            }
        }
        double arow[NB];
        uint8_t codes[NB];
        lm_row_update<NB>(v, alpha, stepmax, steparg, ssum, jj, j2, nrem2, active, skip_pen, eskip, sstep, sarg, ss, lp, lp0, pd, pd0, dt,
                          arow, codes);
        if (active) {
#pragma unroll
            for (int c = 0; c < NB; c++) fwd[(size_t)t * nkmer + jj * NB + c] = arow[c];
            lm_store_codes<NB>(tbb + (size_t)t * nkmer + (size_t)jj * NB, codes);
        }
#pragma unroll
        for (int c = 0; c < NB; c++) raw[c] = nxt[c];
        raw0 = nxt0;
        __syncthreads();
    }
    // ---- first argmax of v (np.argmax, decode.py:85) ----
    float bv = -INFINITY;
    int bi = 0x7fffffff;
    if (active) {
#pragma unroll
        for (int c = 0; c < NB; c++) {
            const float x = v[jj * NB + c];
            if (x > bv) { bv = x; bi = jj * NB + c; }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(bv, o);
        const int oi = __shfl_xor(bi, o);
        if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
    }
    if ((j & 63) == 0) { redv[j >> 6] = bv; redi[j >> 6] = bi; }
    // ---- Z: the total of the last row ----
    {
        double ss = alpha[jj];
#pragma unroll
        for (int a = 1; a < NB; a++) ss += alpha[a * nrem1 + jj];
        if (active) ssum[jj] = ss;
    }
    __syncthreads();
    if (j < 64) {
        const double tot = lm_wave_total(ssum, nrem1, j);
        if (j == 0) {
            for (int w = 1; w < (nt >> 6); w++)
                if (redv[w] > bv || (redv[w] == bv && redi[w] < bi)) { bv = redv[w]; bi = redi[w]; }
            bi = bi == 0x7fffffff ? 0 : bi;                    // no score above -inf: np.argmax's state 0
            score_out[b] = bv;
            logz[b] = log(tot) + 0.6931471805599453 * (double)d_sum;      // d_sum: what rows 1 .. T - 1 took off
            sh_tot = tot;
            sh_cur[(T - 1) & 1] = bi;
            sh_pos[(T - 1) & 1] = T;
        }
    }
    __threadfence_block();                                     // thread 0's row exponents are read by every thread below
    __syncthreads();

    // ---- pass 2 -------------------------------------------------------------------------------------------------------------------
    const double zs = sh_tot;
    int32_t *ptmp = ws.path + (size_t)b * Tpad, *rtmp = ws.row + (size_t)b * Tpad;
    double *ctmp = ws.conf + (size_t)b * Tpad;
    int idx1[NB], idx2[NB];                                    // the step and the skip group that state jj*NB + c feeds as a predecessor
#pragma unroll
    for (int c = 0; c < NB; c++) {
        idx1[c] = (jj * NB + c) % nrem1;
        idx2[c] = (jj * NB + c) % nrem2;
    }
    double y[NB], xr[NB], xn[NB];
    int cd[NB], cn[NB];
    float pr[NB], pr0, pn[NB], pn0 = 0.0f;
    int dn = 0;
    auto load_row = [&](int t, double (&x)[NB], int (&codes)[NB], float (&p)[NB], float &p0, int &d) {
#pragma unroll
        for (int c = 0; c < NB; c++) {
            const size_t at = (size_t)t * nkmer + jj * NB + c;
            x[c] = fwd[at];
            p[c] = pb[(size_t)t * tstride + 1 + jj * NB + c];
        }
        const uint8_t *src = tbb + (size_t)t * nkmer + (size_t)jj * NB;       // (row 0 has no traceback: the path begins there)
        if constexpr (NB == 4) {
            const uint32_t w = t > 0 ? *reinterpret_cast<const uint32_t *>(src) : 0xffffffffu;
#pragma unroll
            for (int c = 0; c < NB; c++) codes[c] = (int)((w >> (8 * c)) & 0xff);
        } else {
#pragma unroll
            for (int c = 0; c < NB; c++) codes[c] = t > 0 ? (int)src[c] : LM_STAY;
        }
        p0 = pb[(size_t)t * tstride];
        d = dexp[t];
    };
    int dt;
    load_row(T - 1, xr, cd, pr, pr0, dt);
#pragma unroll
    for (int c = 0; c < NB; c++) y[c] = 1.0;
    double dwell = 0.0;                                        // largest gamma of the position this thread is collecting
    for (int t = T - 1; t >= 0; t--) {
        if (t > 0) load_row(t - 1, xn, cn, pn, pn0, dn);       // the row below, one step ahead of its use
        const int par = t & 1;
        const int cur = sh_cur[par];
        const bool owner = active && cur / NB == j;
        double g[NB];
        if (gamma || owner) {
#pragma unroll
            for (int c = 0; c < NB; c++) g[c] = xr[c] * y[c] / zs;
        }
        if (gamma && active) {
            float *go = gamma + ((size_t)t * B + b) * nkmer + (size_t)jj * NB;
#pragma unroll
            for (int c = 0; c < NB; c++) go[c] = (float)g[c];
        }
        if (owner) {
            double gc = 0.0;
            int code = LM_STAY;
#pragma unroll
            for (int c = 0; c < NB; c++)
                if (cur - j * NB == c) { gc = g[c]; code = cd[c]; }
            dwell = fmax(dwell, gc);
            int pos = sh_pos[par], ncur = cur;
            if (t == 0 || code != LM_STAY) {                   // the path enters `cur` at row t (decode.py:88-90)
                --pos;
                ptmp[pos] = cur;
                rtmp[pos] = t;
                ctmp[pos] = dwell;
                dwell = 0.0;
                if (t > 0) ncur = code < NB ? code * nrem1 + cur / NB : (code - NB) * nrem2 + cur / NB2;
            }
            sh_cur[par ^ 1] = ncur;                            // read behind this row's barriers
            sh_pos[par ^ 1] = pos;
        }
        if (t > 0) {
            double pd[NB];
#pragma unroll
            for (int c = 0; c < NB; c++) pd[c] = px(pr[c]);
            const double pd0 = px(pr0);
            double s1 = pd[0] * y[0];
#pragma unroll
            for (int c = 1; c < NB; c++) s1 += pd[c] * y[c];
            if (active) g1[par][jj] = s1;
            __syncthreads();
            if (j < nrem2) {
                double s2 = g1[par][j * NB];
#pragma unroll
                for (int c = 1; c < NB; c++) s2 += g1[par][j * NB + c];
                g2[par][j] = s2;
            }
            __syncthreads();
#pragma unroll
            for (int c = 0; c < NB; c++) {
                y[c] = ldexp(pd0 * y[c] + (g1[par][idx1[c]] + eskip * g2[par][idx2[c]]), -dt);
                xr[c] = xn[c];
                cd[c] = cn[c];
                pr[c] = pn[c];
            }
            pr0 = pn0;
            dt = dn;
        }
    }
    __threadfence_block();
    __syncthreads();
    // ---- left aligned results; what lies behind the path, and the rows behind the chunk, read -1 / 0 ----
    const int pos = sh_pos[1], len = T - pos;                  // row 0 wrote the slots of parity 1
    for (int i = j; i < Tpad; i += nt) {
        const bool in = i < len;
        path_out[(size_t)b * Tpad + i] = in ? ptmp[pos + i] : -1;
        move_row[(size_t)b * Tpad + i] = in ? rtmp[pos + i] : -1;
        conf[(size_t)b * Tpad + i] = in ? ctmp[pos + i] : 0.0;
    }
    if (j == 0) len_out[b] = len;
    if (gamma)
        for (int t = T; t < Tpad; t++)
            for (int s = j; s < nkmer; s += nt) gamma[((size_t)t * B + b) * nkmer + s] = 0.0f;
}

extern "C" int slk_viterbi_marginals_f32(const float *post, int T, int B, int nbase, int klen, float skip_pen, int input_mode,
                                         float min_prob, const int32_t *lens, void *workspace, size_t workspace_bytes,
                                         float *score_out, int32_t *path_out, int32_t *len_out, int32_t *move_row, double *conf,
                                         double *logz, float *gamma, slk_stream_t stream)
{
    if (!post || !score_out || !path_out || !len_out || !move_row || !conf || !logz || T < 1 || B < 1 || input_mode < 0 ||
        input_mode > SLK_POST_LN || !(min_prob >= 0.0f && min_prob < 1.0f) || !(skip_pen == skip_pen))
        return SLK_ERR_INVALID_ARG;
    if (input_mode != SLK_POST_RAW && input_mode != SLK_POST_PLAIN) return SLK_ERR_UNSUPPORTED;      // weights, not their logarithms
    int nkmer;
    if (!lm_dims(nbase, klen, &nkmer)) return SLK_ERR_UNSUPPORTED;
    lm_workspace ws;
    const size_t need = lm_carve(workspace, T, B, nkmer, &ws);
    if (!workspace || workspace_bytes < need) return SLK_ERR_WORKSPACE;
    if (reinterpret_cast<uintptr_t>(workspace) & 7) return SLK_ERR_INVALID_ARG;
    const int nrem1 = nkmer / nbase;
    const int threads = nrem1 < 64 ? 64 : ((nrem1 + 63) / 64) * 64;
    const float one_m = one_minus(min_prob, (double)min_prob);
    const double eskip = exp(-(double)skip_pen);
    hipStream_t s = slk_stream(stream);
    if (nbase == 4)
        hipLaunchKernelGGL((lattice_marginals_kernel<4>), dim3(B), dim3(threads), 0, s, post, T, B, nkmer, skip_pen, eskip, input_mode,
                           min_prob, one_m, lens, ws, score_out, path_out, len_out, move_row, conf, logz, gamma);
    else
        hipLaunchKernelGGL((lattice_marginals_kernel<5>), dim3(B), dim3(threads), 0, s, post, T, B, nkmer, skip_pen, eskip, input_mode,
                           min_prob, one_m, lens, ws, score_out, path_out, len_out, move_row, conf, logz, gamma);
    return slk_launch_status();
}

// ---- checkpointed forward rows (design/lattice_marginals.md 8) -----------------------------------------------------------------------
// The same two passes with the forward state kept for every K-th row only.  Pass 1 stores, for rows 0, K, 2K, ..: the scaled forward
// row, the max-plus row and the row's traceback codes -- and for every row its exponent, as the kernel above.  Pass 2 takes the
// segments of K rows from the last to the first: it reloads the checkpoint, runs lm_step_groups / lm_row_update over the segment's
// other rows again -- each row scaled by its STORED exponent, so wave 0 has no reduction here -- and keeps every row's forward
// values and codes in a segment buffer in dynamic LDS; then it walks down the segment as the kernel above walks down the workspace.
// A thread reads back from the buffer only what it wrote itself (the states it owns), so the buffer needs no barrier, and it reads a
// row at the row's own turn, not one row ahead: the walk at a segment's first row needs that row's codes -- kept with the
// checkpoint -- and nothing of the segment below.

// the static LDS of the kernel: what the kernel above declares array by array
struct lm_lds {
    double alpha[LM_MAX_STATES], ssum[LM_MAX_GROUPS], g1[2][LM_MAX_GROUPS], g2[2][LM_MAX_GROUPS2], tot;
    float v[LM_MAX_STATES], stepmax[LM_MAX_GROUPS];
    int steparg[LM_MAX_GROUPS];
    float redv[4];
    int redi[4], d[2], cur[2], pos[2];
};
#define LM_LDS_MAX (160 * 1024)                      /* of a CU */
#define LMC_SEGMENT_BUDGET (36 * 1024)               /* the default segment buffer: K = 4 at N = 1024 (design/lattice_marginals.md 8) */
#define LMC_EVERY_MAX 64

// workspace: [B][C][N] float64 checkpointed forward rows, C = ceil(T / K) | [B][T] float64 conf, right aligned | [B][C][N] float32
// max-plus rows | [B][T] int32 row exponents | [B][T] int32 path and [B][T] int32 move rows, right aligned | [B][C][N] traceback bytes
struct lmc_workspace {
    double *alpha, *conf;
    float *v;
    int32_t *dexp, *path, *row;
    uint8_t *tb;
};

static size_t lmc_carve(void *base, int T, int B, int nkmer, int every, lmc_workspace *w)
{
    const size_t rows = (size_t)B * T, cells = (size_t)B * ((T + every - 1) / every) * nkmer;
    uint8_t *p = static_cast<uint8_t *>(base);
    size_t off = 0;
    w->alpha = reinterpret_cast<double *>(p + off);  off += 8 * cells;
    w->conf = reinterpret_cast<double *>(p + off);   off += 8 * rows;
    w->v = reinterpret_cast<float *>(p + off);       off += 4 * cells;
    w->dexp = reinterpret_cast<int32_t *>(p + off);  off += 4 * rows;
    w->path = reinterpret_cast<int32_t *>(p + off);  off += 4 * rows;
    w->row = reinterpret_cast<int32_t *>(p + off);   off += 4 * rows;
    w->tb = p + off;                                 off += cells;
    return (off + 255) & ~(size_t)255;
}

// rows per checkpoint: the caller's, or for 0 what LMC_SEGMENT_BUDGET holds; -1 for a negative one
static int lmc_every(int every, int nkmer)
{
    if (every < 0) return -1;
    if (every > 0) return every;
    const int k = LMC_SEGMENT_BUDGET / (9 * nkmer);
    return k < 1 ? 1 : (k > LMC_EVERY_MAX ? LMC_EVERY_MAX : k);
}

extern "C" size_t slk_viterbi_marginals_ckpt_workspace_bytes(int T, int B, int nbase, int klen, int every)
{
    int nkmer;
    if (T < 1 || B < 1 || !lm_dims(nbase, klen, &nkmer)) return 0;
    every = lmc_every(every, nkmer);
    if (every < 1) return 0;
    lmc_workspace w;
    return lmc_carve(nullptr, T, B, nkmer, every, &w);
}

template <int NB>
__global__ void __launch_bounds__(256) lattice_marginals_ckpt_kernel(const float *__restrict__ post, int T, int B, int nkmer,
                                                                     float skip_pen, double eskip, int mode, float min_prob, float one_m,
                                                                     const int32_t *__restrict__ lens, int every, lmc_workspace ws,
                                                                     float *__restrict__ score_out, int32_t *__restrict__ path_out,
                                                                     int32_t *__restrict__ len_out, int32_t *__restrict__ move_row,
                                                                     double *__restrict__ conf, double *__restrict__ logz,
                                                                     float *__restrict__ gamma)
{
    constexpr int NB2 = NB * NB;
    __shared__ lm_lds sh;
    extern __shared__ __attribute__((aligned(16))) unsigned char lm_seg[];
    double *alpha = sh.alpha, *ssum = sh.ssum;
    float *v = sh.v, *stepmax = sh.stepmax;
    int *steparg = sh.steparg;

    const int Tpad = T;                                        // row stride of everything per chunk; T = this chunk's own length
    const int b = blockIdx.x, j = threadIdx.x, nt = blockDim.x;
    if (lens) T = min(max(lens[b], 1), Tpad);
    const int nrem1 = nkmer / NB, nrem2 = nkmer / NB2;
    const bool active = j < nrem1;
    const int jj = active ? j : 0, j2 = jj / NB;
    const size_t ld = (size_t)nkmer + 1;
    const float *pb = post + (size_t)b * ld;
    const size_t tstride = (size_t)B * ld;
    const size_t nck = (size_t)((Tpad + every - 1) / every);
    double *cka = ws.alpha + (size_t)b * nck * nkmer;
    float *ckv = ws.v + (size_t)b * nck * nkmer;
    uint8_t *ckt = ws.tb + (size_t)b * nck * nkmer;
    int32_t *dexp = ws.dexp + (size_t)b * Tpad;
    // the segment buffer, private to the thread state by state: forward values [every][NB][nrem1], then the codes [every][nrem1][NB]
    double *segf = reinterpret_cast<double *>(lm_seg);
    uint8_t *segc = lm_seg + (size_t)every * nkmer * sizeof(double);

    auto lpx = [&](float r) { return log_post_val(r, mode, min_prob, one_m); };
    auto px = [&](float r) { return (double)(mode == SLK_POST_RAW ? prepare_post_val(r, min_prob, one_m) : r); };
    // the checkpoint of a row: what the thread's states hold behind the row's update
    auto keep = [&](int k, const double (&arow)[NB], const uint8_t (&codes)[NB]) {
        const size_t at = (size_t)k * nkmer + (size_t)jj * NB;
#pragma unroll
        for (int c = 0; c < NB; c++) {
            cka[at + c] = arow[c];
            ckv[at + c] = v[jj * NB + c];
        }
        lm_store_codes<NB>(ckt + at, codes);
    };

    // ---- pass 1: the kernel above, row for row; what it stores per row is stored here per checkpoint ------------------------------
    float raw[NB], raw0 = 0.0f;
#pragma unroll
    for (int c = 0; c < NB; c++) raw[c] = pb[1 + jj * NB + c];
    if (active) {
        double arow[NB];
        uint8_t codes[NB];
#pragma unroll
        for (int c = 0; c < NB; c++) {
            const int s = jj * NB + c;
            arow[c] = px(raw[c]);                              // row 0: state s weighs p[0][1 + s]
            v[s] = lpx(raw[c]);                                // decode.py:57
            alpha[s] = arow[c];
            codes[c] = (uint8_t)LM_STAY;                       // (row 0 has no traceback: the path begins there)
        }
        keep(0, arow, codes);
    }
    if (j == 0) {
        dexp[0] = 0;
        sh.d[1] = 0;                                           // row 1 is not scaled: no total is known yet
    }
    if (T > 1) {
#pragma unroll
        for (int c = 0; c < NB; c++) raw[c] = pb[tstride + 1 + jj * NB + c];
        raw0 = pb[tstride];
    }
    __syncthreads();
    int d_cur = 0, d_sum = 0;                                  // wave 0: the exponent row t applies, the sum of those applied
    int phase = 0, ck = 0;                                     // t = ck * every + phase
    for (int t = 1; t < T; t++) {
        float nxt[NB], nxt0 = 0.0f;
        if (t + 1 < T) {                                       // the next row, one step ahead of its use
            const float *pn = pb + (size_t)(t + 1) * tstride;
#pragma unroll
            for (int c = 0; c < NB; c++) nxt[c] = pn[1 + jj * NB + c];
            nxt0 = pn[0];
        } else {
#pragma unroll
            for (int c = 0; c < NB; c++) nxt[c] = 0.0f;
        }
        float sstep;
        int sarg;
        double ss;
        lm_step_groups<NB>(v, alpha, stepmax, steparg, ssum, jj, nrem1, active, sstep, sarg, ss);
        float lp[NB];
        double pd[NB];
#pragma unroll
        for (int c = 0; c < NB; c++) { lp[c] = lpx(raw[c]); pd[c] = px(raw[c]); }
        const float lp0 = lpx(raw0);
        const double pd0 = px(raw0);
        const int dt = sh.d[t & 1];                            // written during row t - 1, behind that row's first barrier
        __syncthreads();
        if (j < 64) {
            // wave 0: the total of row t - 1 as it lies in LDS; row t + 1 scales by its exponent less what row t takes off
            d_sum += d_cur;
            d_cur = lm_exponent(lm_wave_total(ssum, nrem1, j)) - d_cur;
            if (j == 0) {
                sh.d[(t + 1) & 1] = d_cur;
                dexp[t] = dt;
            }
        }
        double arow[NB];
        uint8_t codes[NB];
        lm_row_update<NB>(v, alpha, stepmax, steparg, ssum, jj, j2, nrem2, active, skip_pen, eskip, sstep, sarg, ss, lp, lp0, pd, pd0, dt,
                          arow, codes);
        if (++phase == every) {
            phase = 0;
            ++ck;
            if (active) keep(ck, arow, codes);
        }
#pragma unroll
        for (int c = 0; c < NB; c++) raw[c] = nxt[c];
        raw0 = nxt0;
        __syncthreads();
    }
    // ---- first argmax of v (np.argmax, decode.py:85) ----
    float bv = -INFINITY;
    int bi = 0x7fffffff;
    if (active) {
#pragma unroll
        for (int c = 0; c < NB; c++) {
            const float x = v[jj * NB + c];
            if (x > bv) { bv = x; bi = jj * NB + c; }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(bv, o);
        const int oi = __shfl_xor(bi, o);
        if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
    }
    if ((j & 63) == 0) { sh.redv[j >> 6] = bv; sh.redi[j >> 6] = bi; }
    // ---- Z: the total of the last row ----
    {
        double ss = alpha[jj];
#pragma unroll
        for (int a = 1; a < NB; a++) ss += alpha[a * nrem1 + jj];
        if (active) ssum[jj] = ss;
    }
    __syncthreads();
    if (j < 64) {
        const double tot = lm_wave_total(ssum, nrem1, j);
        if (j == 0) {
            for (int w = 1; w < (nt >> 6); w++)
                if (sh.redv[w] > bv || (sh.redv[w] == bv && sh.redi[w] < bi)) { bv = sh.redv[w]; bi = sh.redi[w]; }
            bi = bi == 0x7fffffff ? 0 : bi;                    // no score above -inf: np.argmax's state 0
            score_out[b] = bv;
            logz[b] = log(tot) + 0.6931471805599453 * (double)d_sum;      // d_sum: what rows 1 .. T - 1 took off
            sh.tot = tot;
            sh.cur[(T - 1) & 1] = bi;
            sh.pos[(T - 1) & 1] = T;
        }
    }
    __threadfence_block();                                     // thread 0's row exponents are read by every thread below
    __syncthreads();

    // ---- pass 2: segment by segment, recompute then walk ----------------------------------------------------------------------------
    const double zs = sh.tot;
    int32_t *ptmp = ws.path + (size_t)b * Tpad, *rtmp = ws.row + (size_t)b * Tpad;
    double *ctmp = ws.conf + (size_t)b * Tpad;
    int idx1[NB], idx2[NB];                                    // the step and the skip group that state jj*NB + c feeds as a predecessor
#pragma unroll
    for (int c = 0; c < NB; c++) {
        idx1[c] = (jj * NB + c) % nrem1;
        idx2[c] = (jj * NB + c) % nrem2;
    }
    double y[NB];
    float pr[NB], pr0, pn[NB], pn0 = 0.0f;                     // the walk's posterior row and exponent, fetched one row ahead
    int dt, dn = 0;
    auto load_post = [&](int t, float (&p)[NB], float &p0, int &d) {
#pragma unroll
        for (int c = 0; c < NB; c++) p[c] = pb[(size_t)t * tstride + 1 + jj * NB + c];
        p0 = pb[(size_t)t * tstride];
        d = dexp[t];
    };
    load_post(T - 1, pr, pr0, dt);
#pragma unroll
    for (int c = 0; c < NB; c++) y[c] = 1.0;
    double dwell = 0.0;                                        // largest gamma of the position this thread is collecting
    ck = (T - 1) / every;
    for (int s0 = ck * every; s0 >= 0; s0 -= every, --ck) {
        const int s1 = min(s0 + every, T);                     // the segment: rows s0 .. s1 - 1
        // ---- the checkpoint: row s0 as pass 1 left it ----
        if (active) {
            const size_t at = (size_t)ck * nkmer + (size_t)jj * NB;
#pragma unroll
            for (int c = 0; c < NB; c++) {
                const double a = cka[at + c];
                alpha[jj * NB + c] = a;
                v[jj * NB + c] = ckv[at + c];
                segf[c * nrem1 + jj] = a;
            }
            if constexpr (NB == 4) {
                *reinterpret_cast<uint32_t *>(segc + (size_t)jj * NB) = *reinterpret_cast<const uint32_t *>(ckt + at);
            } else {
#pragma unroll
                for (int c = 0; c < NB; c++) segc[jj * NB + c] = ckt[at + c];
            }
        }
        int dr = 0;                                            // the stored exponent of the row to recompute, one row ahead
        if (s0 + 1 < s1) {
            const float *pq = pb + (size_t)(s0 + 1) * tstride;
#pragma unroll
            for (int c = 0; c < NB; c++) raw[c] = pq[1 + jj * NB + c];
            raw0 = pq[0];
            dr = dexp[s0 + 1];
        }
        __syncthreads();
        // ---- rows s0 + 1 .. s1 - 1 again, into the segment buffer ----
        for (int t = s0 + 1; t < s1; t++) {
            float nxt[NB], nxt0 = 0.0f;
            int dnx = 0;
            if (t + 1 < s1) {
                const float *pq = pb + (size_t)(t + 1) * tstride;
#pragma unroll
                for (int c = 0; c < NB; c++) nxt[c] = pq[1 + jj * NB + c];
                nxt0 = pq[0];
                dnx = dexp[t + 1];
            } else {
#pragma unroll
                for (int c = 0; c < NB; c++) nxt[c] = 0.0f;
            }
            float sstep;
            int sarg;
            double ss;
            lm_step_groups<NB>(v, alpha, stepmax, steparg, ssum, jj, nrem1, active, sstep, sarg, ss);
            float lp[NB];
            double pd[NB];
#pragma unroll
            for (int c = 0; c < NB; c++) { lp[c] = lpx(raw[c]); pd[c] = px(raw[c]); }
            const float lp0 = lpx(raw0);
            const double pd0 = px(raw0);
            __syncthreads();
            double arow[NB];
            uint8_t codes[NB];
            lm_row_update<NB>(v, alpha, stepmax, steparg, ssum, jj, j2, nrem2, active, skip_pen, eskip, sstep, sarg, ss, lp, lp0, pd, pd0,
                              dr, arow, codes);
            if (active) {
                const int r = t - s0;
#pragma unroll
                for (int c = 0; c < NB; c++) segf[((size_t)r * NB + c) * nrem1 + jj] = arow[c];
                lm_store_codes<NB>(segc + (size_t)r * nkmer + (size_t)jj * NB, codes);
            }
#pragma unroll
            for (int c = 0; c < NB; c++) raw[c] = nxt[c];
            raw0 = nxt0;
            dr = dnx;
            __syncthreads();
        }
        // ---- the walk down the segment: the kernel above's loop, its forward rows and codes out of the segment buffer ----
        for (int t = s1 - 1; t >= s0; t--) {
            if (t > 0) load_post(t - 1, pn, pn0, dn);          // the row below, one step ahead of its use
            const int r = t - s0;
            double xr[NB];
            int cd[NB];
#pragma unroll
            for (int c = 0; c < NB; c++) xr[c] = segf[((size_t)r * NB + c) * nrem1 + jj];
            lm_load_codes<NB>(segc + (size_t)r * nkmer + (size_t)jj * NB, cd);
            const int par = t & 1;
            const int cur = sh.cur[par];
            const bool owner = active && cur / NB == j;
            double g[NB];
            if (gamma || owner) {
#pragma unroll
                for (int c = 0; c < NB; c++) g[c] = xr[c] * y[c] / zs;
            }
            if (gamma && active) {
                float *go = gamma + ((size_t)t * B + b) * nkmer + (size_t)jj * NB;
#pragma unroll
                for (int c = 0; c < NB; c++) go[c] = (float)g[c];
            }
            if (owner) {
                double gc = 0.0;
                int code = LM_STAY;
#pragma unroll
                for (int c = 0; c < NB; c++)
                    if (cur - j * NB == c) { gc = g[c]; code = cd[c]; }
                dwell = fmax(dwell, gc);
                int pos = sh.pos[par], ncur = cur;
                if (t == 0 || code != LM_STAY) {               // the path enters `cur` at row t (decode.py:88-90)
                    --pos;
                    ptmp[pos] = cur;
                    rtmp[pos] = t;
                    ctmp[pos] = dwell;
                    dwell = 0.0;
                    if (t > 0) ncur = code < NB ? code * nrem1 + cur / NB : (code - NB) * nrem2 + cur / NB2;
                }
                sh.cur[par ^ 1] = ncur;                        // read behind this row's barriers
                sh.pos[par ^ 1] = pos;
            }
            if (t > 0) {
                double pd[NB];
#pragma unroll
                for (int c = 0; c < NB; c++) pd[c] = px(pr[c]);
                const double pd0 = px(pr0);
                double s1v = pd[0] * y[0];
#pragma unroll
                for (int c = 1; c < NB; c++) s1v += pd[c] * y[c];
                if (active) sh.g1[par][jj] = s1v;
                __syncthreads();
                if (j < nrem2) {
                    double s2 = sh.g1[par][j * NB];
#pragma unroll
                    for (int c = 1; c < NB; c++) s2 += sh.g1[par][j * NB + c];
                    sh.g2[par][j] = s2;
                }
                __syncthreads();
#pragma unroll
                for (int c = 0; c < NB; c++) {
                    y[c] = ldexp(pd0 * y[c] + (sh.g1[par][idx1[c]] + eskip * sh.g2[par][idx2[c]]), -dt);
                    pr[c] = pn[c];
                }
                pr0 = pn0;
                dt = dn;
            }
        }
    }
    __threadfence_block();
    __syncthreads();
    // ---- left aligned results; what lies behind the path, and the rows behind the chunk, read -1 / 0 ----
    const int pos = sh.pos[1], len = T - pos;                  // row 0 wrote the slots of parity 1
    for (int i = j; i < Tpad; i += nt) {
        const bool in = i < len;
        path_out[(size_t)b * Tpad + i] = in ? ptmp[pos + i] : -1;
        move_row[(size_t)b * Tpad + i] = in ? rtmp[pos + i] : -1;
        conf[(size_t)b * Tpad + i] = in ? ctmp[pos + i] : 0.0;
    }
    if (j == 0) len_out[b] = len;
    if (gamma)
        for (int t = T; t < Tpad; t++)
            for (int s = j; s < nkmer; s += nt) gamma[((size_t)t * B + b) * nkmer + s] = 0.0f;
}

extern "C" int slk_viterbi_marginals_ckpt_f32(const float *post, int T, int B, int nbase, int klen, float skip_pen, int input_mode,
                                              float min_prob, const int32_t *lens, int every, void *workspace, size_t workspace_bytes,
                                              float *score_out, int32_t *path_out, int32_t *len_out, int32_t *move_row, double *conf,
                                              double *logz, float *gamma, slk_stream_t stream)
{
    if (!post || !score_out || !path_out || !len_out || !move_row || !conf || !logz || T < 1 || B < 1 || input_mode < 0 ||
        input_mode > SLK_POST_LN || !(min_prob >= 0.0f && min_prob < 1.0f) || !(skip_pen == skip_pen) || every < 0)
        return SLK_ERR_INVALID_ARG;
    if (input_mode != SLK_POST_RAW && input_mode != SLK_POST_PLAIN) return SLK_ERR_UNSUPPORTED;      // weights, not their logarithms
    int nkmer;
    if (!lm_dims(nbase, klen, &nkmer)) return SLK_ERR_UNSUPPORTED;
    every = lmc_every(every, nkmer);
    const size_t seg = 9 * (size_t)nkmer * every;              // float64 forward value and traceback byte per state and row
    if (sizeof(lm_lds) + seg > LM_LDS_MAX) return SLK_ERR_UNSUPPORTED;
    lmc_workspace ws;
    const size_t need = lmc_carve(workspace, T, B, nkmer, every, &ws);
    if (!workspace || workspace_bytes < need) return SLK_ERR_WORKSPACE;
    if (reinterpret_cast<uintptr_t>(workspace) & 7) return SLK_ERR_INVALID_ARG;
    const int nrem1 = nkmer / nbase;
    const int threads = nrem1 < 64 ? 64 : ((nrem1 + 63) / 64) * 64;
    const float one_m = one_minus(min_prob, (double)min_prob);
    const double eskip = exp(-(double)skip_pen);
    hipStream_t s = slk_stream(stream);
    auto launch = [&](auto kernel) {
        // a request above 64 KB needs the function attribute raised once per device
        const bool ok = SLK_PER_DEVICE(bool, hipFuncSetAttribute(reinterpret_cast<const void *>(kernel),
                                                                 hipFuncAttributeMaxDynamicSharedMemorySize,
                                                                 (int)(LM_LDS_MAX - sizeof(lm_lds))) == hipSuccess);
        if (!ok) return (int)SLK_ERR_UNSUPPORTED;
        hipLaunchKernelGGL(kernel, dim3(B), dim3(threads), seg, s, post, T, B, nkmer, skip_pen, eskip, input_mode, min_prob, one_m, lens,
                           every, ws, score_out, path_out, len_out, move_row, conf, logz, gamma);
        return slk_launch_status();
    };
    return nbase == 4 ? launch(lattice_marginals_ckpt_kernel<4>) : launch(lattice_marginals_ckpt_kernel<5>);
}
