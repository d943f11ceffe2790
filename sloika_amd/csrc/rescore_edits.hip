// rescore_edits.hip -- the forward score of EDITED sequences on gfx950: for a ragged batch of (posterior, sequence) pairs and, per
// pair, any number of candidate edits (a, d, c[0..m)) -- replace positions [a, a + d) by m new symbols -- the log-likelihood of each
// edited sequence under the pair's posterior, summed over all alignments, full length (design/rescore_edits.md).
//
//     F_0 = e_0      F_t[j]     = F_{t-1}[j] p_t[blank] + F_{t-1}[j-1] p_t[seq[j-1]]
//     B_T = e_L      B_{t-1}[j] = B_t[j] p_t[blank] + B_t[j+1] p_t[seq[j]]
//     g_t[0] = F_t[a], g_0[i > 0] = 0, g_t[i] = g_{t-1}[i] p_t[blank] + g_{t-1}[i-1] p_t[c[i-1]]          (i = 1 .. m)
//     a + d < L:  Z' = sum_{t=0}^{T-1} g_t[m] p_{t+1}[seq[a+d]] B_{t+1}[a+d+1]        a + d = L:  Z' = g_T[m]
//
// Column a of F depends on seq[0..a) alone and column a + d + 1 of B on seq[a+d+1..) alone, so neither is changed by the edit; every
// full path of the edited sequence leaves its state a + m exactly once, or ends in it.  A candidate costs T (m + 1) cells, not T L.
//
// Lattice kernel: one workgroup of 256 threads per pair with the ownership of forward_score.hip (thread i holds the ppt consecutive
// states from i * ppt, ppt by the pair alone, one barrier per row).  Pass 1 is that file's row step and stores every scaled row F_t
// and its running binary exponent EF_t; pass 2 is forward_backward.hip's b recursion and stores every B_t and EB_t.  A row is scaled by
// the exact power of two of the previous row's total, so F_t = stored * 2^EF_t with no rounding from the scaling.  The pair's slice of
// the workspace is  F [T+1][ldj] | B [T+1][ldj] | EF [T+1] | EB [T+1]  (float64, int64), ldj = L + 1 rounded up to 2.
//
// Candidate kernel: one lane per candidate, a workgroup holds up to 256 candidates of ONE pair (workgroup (b, y) takes candidates
// cand_off[b] + 256 y ..; cand_off is built on the host from cand_pair).  The workgroup walks the rows together: row t + 1 of the
// posterior is staged into LDS once per workgroup (two buffers on the row's parity, one barrier per row, 16-byte loads issued one row
// ahead into registers), each lane gathers its m + 1 emissions and p[seq[a+d]] from LDS and reads F_t[a], B_{t+1}[a+d+1] from the
// workspace one row ahead.  g lives in registers, unrolled to SLK_RESCORE_MAX_NEW: a lane's chain takes the last m + 1 slots,
// the slots in front of it hold zeros.  g is rescaled with its row's EF_t - EF_{t-1}; the terms of the cut sum carry the exponent EF_{t+1} + EB_t (the same for the
// whole workgroup) and are added in ascending t as (mantissa, integer exponent).  One log per candidate.  Nothing a lane computes
// depends on another lane, on the workgroup it sits in or on the launch.
#include <cstdlib>
#include <vector>

#include "rescore_common.h"

struct re_args {
    fs_args f;                                                // (full = 1; score_out = the pairs' scores)
    double *ws;                                               // the workspace; ws_off[b]: where pair b's slice begins, in doubles
    const int64_t *ws_off;
    const int64_t *cand_off;                                  // [nread + 1]: pair b owns candidates cand_off[b] .. cand_off[b + 1]
    const int32_t *cand_start, *cand_ndel, *cand_new;
    const int64_t *cand_new_off;
    int64_t nnew;                                             // cand_new_off[ncand]
    double *ll;
};

__host__ __device__ static inline int re_ldj(int L) { return (L + 2) & ~1; }

struct re_view {
    double *F, *B;
    int64_t *EF, *EB;
    int ldj;
};
__device__ __forceinline__ re_view re_pair_view(double *base, int L, int nr)
{
    re_view v;
    v.ldj = re_ldj(L);
    const size_t n = (size_t)(nr + 1) * v.ldj;
    v.F = base;
    v.B = base + n;
    v.EF = reinterpret_cast<int64_t *>(base + 2 * n);
    v.EB = v.EF + (nr + 1);
    return v;
}

// the states j0 .. j0 + PPT - 1 of one row; columns past ldj do not exist (ldj is even, so a pair of columns is whole or absent)
template <int PPT>
__device__ __forceinline__ void re_store_row(double *row, int j0, int ldj, const double (&f)[PPT])
{
    if constexpr (PPT == 1) {
        if (j0 < ldj) row[j0] = f[0];
    } else {
#pragma unroll
        for (int k = 0; k < PPT; k += 2)
            if (j0 + k < ldj) *reinterpret_cast<double2 *>(row + j0 + k) = make_double2(f[k], f[k + 1]);
    }
}

template <typename T, int PPT>
__device__ __forceinline__ void re_lattice(const re_args &A, int b, int L, int nr, double (*wsum)[FS_WAVES], double (*edge)[FS_THREADS],
                                           double *endv)
{
    const fs_args &a = A.f;
    constexpr int D = fs_ahead<PPT>::value;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int j0 = tid * PPT;
    const bool raw = a.min_prob > 0.0f;
    const int32_t *seq = a.seq + a.pos_off[b];
    const T *rows = static_cast<const T *>(a.post) + (size_t)a.row_off[b] * (size_t)a.ld;
    const size_t rstride = (size_t)a.row_step * (size_t)a.ld;

    // col[k]: the emission of the move into state j0 + k; col[PPT]: into the right neighbour's first state.  -1: no such move
    int col[PPT + 1];
    bool bad = false;
#pragma unroll
    for (int k = 0; k < PPT; k++) {
        const int j = j0 + k;
        int c = -1;
        if (j >= 1 && j <= L) {
            c = seq[j - 1];
            if (c < 0 || c >= a.nstate) { bad = true; c = -1; }
        }
        col[k] = c;
    }
    if (__syncthreads_or(bad ? 1 : 0)) {                      // a symbol that is no column: NaN, nothing else is written
        if (tid == 0) a.score_out[b] = RE_NAN;
        return;
    }
    col[PPT] = (j0 + PPT <= L) ? seq[j0 + PPT - 1] : -1;      // (its owner has checked it)
    const re_view v = re_pair_view(A.ws + A.ws_off[b], L, nr);

    T eb[D], ee[D][PPT + 1];
    auto fetch = [&](int slot, int p) {
        const T *r = rows + (size_t)p * rstride;
        eb[slot] = r[a.blank];
#pragma unroll
        for (int k = 0; k <= PPT; k++) ee[slot][k] = col[k] >= 0 ? r[col[k]] : (T)0;
    };
    auto fill = [&](bool down) {
#pragma unroll
        for (int d = 0; d < D; d++) {
            if (d < nr) fetch(d, down ? nr - 1 - d : d);
            else {
                eb[d] = (T)0;
#pragma unroll
                for (int k = 0; k <= PPT; k++) ee[d][k] = (T)0;
            }
        }
    };

    // ---- pass 1: F_0 .. F_T, the row step of forward_row.h
    fill(false);
    double f[PPT];
    {
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < PPT; k++) {
            f[k] = j0 + k == 0 ? 1.0 : 0.0;
            s += f[k];
        }
        s = fs_wave_sum(s);
        if (lane == 0) wsum[1][wave] = s;
        edge[1][tid] = f[PPT - 1];
        re_store_row<PPT>(v.F, j0, v.ldj, f);
        if (tid == 0) v.EF[0] = 0;
    }
    __syncthreads();
    int64_t esum = 0;
    for (int p0 = 0; p0 < nr; p0 += D) {
#pragma unroll
        for (int d = 0; d < D; d++) {
            const int p = p0 + d;
            if (p >= nr) break;                               // (the same for the whole workgroup)
            const int par = p & 1;
            const double pb = fs_widen(eb[d], raw, a.min_prob, a.one_m);
            double pe[PPT];
#pragma unroll
            for (int k = 0; k < PPT; k++) pe[k] = col[k] >= 0 ? fs_widen(ee[d][k], raw, a.min_prob, a.one_m) : 0.0;
            if (p + D < nr) fetch(d, p + D);
            const double m = re_sum4(wsum[par ^ 1]);
            int e = 0;
            if (m > 0.0 && m < INFINITY) (void)frexp(m, &e);
            esum += e;
            double prev = tid > 0 ? edge[par ^ 1][tid - 1] : 0.0;
            double s = 0.0;
#pragma unroll
            for (int k = 0; k < PPT; k++) {
                const double g = fma(prev, pe[k], f[k] * pb);
                prev = f[k];
                f[k] = ldexp(g, -e);                          // exact: a power of two
                s += f[k];
            }
            re_store_row<PPT>(v.F + (size_t)(p + 1) * v.ldj, j0, v.ldj, f);
            if (tid == 0) v.EF[p + 1] = esum;
            s = fs_wave_sum(s);
            if (lane == 0) wsum[par][wave] = s;
            edge[par][tid] = f[PPT - 1];
            __syncthreads();
        }
    }
#pragma unroll
    for (int k = 0; k < PPT; k++)
        if (j0 + k == L) *endv = f[k];
    __syncthreads();                                          // (wsum and edge are free again behind it)
    if (tid == 0) a.score_out[b] = log(*endv) + (double)esum * FS_LN2;

    // ---- pass 2: B_T .. B_0, downwards
    fill(true);
    double bb[PPT];
    {
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < PPT; k++) {
            bb[k] = j0 + k == L ? 1.0 : 0.0;
            s += bb[k];
        }
        s = fs_wave_sum(s);
        if (lane == 0) wsum[nr & 1][wave] = s;
        edge[nr & 1][tid] = bb[0];
        re_store_row<PPT>(v.B + (size_t)nr * v.ldj, j0, v.ldj, bb);
        if (tid == 0) v.EB[nr] = 0;
    }
    __syncthreads();
    esum = 0;
    for (int i0 = 0; i0 < nr; i0 += D) {
#pragma unroll
        for (int d = 0; d < D; d++) {
            if (i0 + d >= nr) break;
            const int p = nr - 1 - (i0 + d);
            const int par = p & 1;
            const double pb = fs_widen(eb[d], raw, a.min_prob, a.one_m);
            double pe[PPT + 1];
#pragma unroll
            for (int k = 1; k <= PPT; k++) pe[k] = col[k] >= 0 ? fs_widen(ee[d][k], raw, a.min_prob, a.one_m) : 0.0;
            if (p - D >= 0) fetch(d, p - D);
            const double m = re_sum4(wsum[par ^ 1]);
            int e = 0;
            if (m > 0.0 && m < INFINITY) (void)frexp(m, &e);
            esum += e;
            const double right = tid < FS_THREADS - 1 ? edge[par ^ 1][tid + 1] : 0.0;
            double s = 0.0;
#pragma unroll
            for (int k = 0; k < PPT; k++) {
                const double nb = k + 1 < PPT ? bb[(k + 1) % PPT] : right;
                const double g = fma(nb, pe[k + 1], bb[k] * pb);
                bb[k] = ldexp(g, -e);
                s += bb[k];
            }
            re_store_row<PPT>(v.B + (size_t)p * v.ldj, j0, v.ldj, bb);
            if (tid == 0) v.EB[p] = esum;
            s = fs_wave_sum(s);
            if (lane == 0) wsum[par][wave] = s;
            edge[par][tid] = bb[0];
            __syncthreads();
        }
    }
}

template <typename T, int MAXPPT>
__global__ void __launch_bounds__(FS_THREADS) rescore_lattice_kernel(re_args A)
{
    __shared__ double wsum[2][FS_WAVES];
    __shared__ double edge[2][FS_THREADS];
    __shared__ double endv;
    const fs_args &a = A.f;
    const int b = blockIdx.x;
    const int64_t np = a.pos_off[b + 1] - a.pos_off[b];
    const int nr = a.nrow[b];
    if (np < 0 || np >= (int64_t)FS_THREADS * MAXPPT || nr < 0) {       // longer than the caller said (max_npos): NaN, nothing else
        if (threadIdx.x == 0) a.score_out[b] = RE_NAN;
        return;
    }
    const int L = (int)np;
    const int states = L + 1;
    if (states <= FS_THREADS) re_lattice<T, 1>(A, b, L, nr, wsum, edge, &endv);
    else if (states <= 2 * FS_THREADS) re_lattice<T, 2>(A, b, L, nr, wsum, edge, &endv);
    else if constexpr (MAXPPT >= 8) {
        if (states <= 4 * FS_THREADS) re_lattice<T, 4>(A, b, L, nr, wsum, edge, &endv);
        else if (states <= 8 * FS_THREADS) re_lattice<T, 8>(A, b, L, nr, wsum, edge, &endv);
        else if constexpr (MAXPPT >= 32) {
            if (states <= 16 * FS_THREADS) re_lattice<T, 16>(A, b, L, nr, wsum, edge, &endv);
            else re_lattice<T, 32>(A, b, L, nr, wsum, edge, &endv);
        }
    }
}

// ---- the candidates ------------------------------------------------------------------------------------------------------------

// STAGED = false (the diagnostic build only, design/rescore_edits.md 7): no LDS and no barrier, every lane gathers its emissions of
// the next row from global memory into registers instead.  The same arithmetic on the same values: the same bits.
template <typename T, int NCH, bool STAGED>
__global__ void __launch_bounds__(RE_CAND) rescore_cand_kernel(re_args A, int gran)
{
    extern __shared__ uint4 re_rows[];                        // [2][gran] granules of 16 bytes
    constexpr int M = SLK_RESCORE_MAX_NEW;
    const fs_args &a = A.f;
    const int b = blockIdx.x, tid = threadIdx.x;
    const int64_t c0 = A.cand_off[b] + (int64_t)blockIdx.y * RE_CAND, c1 = A.cand_off[b + 1];
    if (c0 >= c1) return;                                     // (the same for the whole workgroup, as every exit below)
    const bool live = c0 + tid < c1;
    const int64_t ci = c0 + tid;
    const double sc = a.score_out[b];
    if (sc != sc) {                                           // the pair was refused (or scores NaN): so do its candidates
        if (live) A.ll[ci] = RE_NAN;
        return;
    }
    const int L = (int)(a.pos_off[b + 1] - a.pos_off[b]);
    const int nr = a.nrow[b];
    const int32_t *seq = a.seq + a.pos_off[b];
    const bool raw = a.min_prob > 0.0f;
    const T *rows = static_cast<const T *>(a.post) + (size_t)a.row_off[b] * (size_t)a.ld;
    const size_t rstride = (size_t)a.row_step * (size_t)a.ld;
    const re_view v = re_pair_view(A.ws + A.ws_off[b], L, nr);

    // the lane's candidate
    bool ok = live;
    int ca = 0, cd = 0, m = 0, nxt = -1;
    int sym[M];
#pragma unroll
    for (int i = 0; i < M; i++) sym[i] = -1;
    if (live) {
        ca = A.cand_start[ci];
        cd = A.cand_ndel[ci];
        const int64_t o0 = A.cand_new_off[ci], o1 = A.cand_new_off[ci + 1];
        ok = ca >= 0 && cd >= 0 && (int64_t)ca + cd <= L && o0 >= 0 && o1 >= o0 && o1 - o0 <= M && o1 <= A.nnew;
        if (ok) {
            m = (int)(o1 - o0);
#pragma unroll
            for (int i = 0; i < M; i++)
                if (i >= M - m) {                             // (the chain's last m slots, see g below)
                    sym[i] = A.cand_new[o0 + (i - (M - m))];
                    if (sym[i] < 0 || sym[i] >= a.nstate) ok = false;
                }
        }
        if (ok && ca + cd < L) nxt = seq[ca + cd];            // (the lattice kernel has checked the pair's symbols)
        if (!ok) A.ll[ci] = RE_NAN;
    }
    if (!ok) {                                                // a lane without a candidate walks along with zeros and writes nothing
        ca = cd = m = 0;
        nxt = -1;
#pragma unroll
        for (int i = 0; i < M; i++) sym[i] = -1;
    }
    const bool cut = nxt >= 0;
    const double *Fa = v.F + ca, *Bd = v.B + (ca + cd + 1);   // (Bd is read only with a + d < L)

    // The chain sits at the END of g: slot inj = M - m takes F_t[a], slot i > inj is g_t[i - inj] and is entered with sym[i - 1], and
    // g[M] is always g_t[m].  Every slot has a fixed register; the slots below inj hold 0 and are entered with 0.
    const int inj = M - m;
    double g[M + 1];
    {
        const double f0 = ok ? Fa[0] : 0.0;
#pragma unroll
        for (int i = 0; i <= M; i++) g[i] = i == inj ? f0 : 0.0;
    }

    re_stage<T, NCH> st;
    T qb = (T)0, qn = (T)0, qc[M];                            // (not STAGED: the emissions of the next row)
    auto gather = [&](const T *r) {
        qb = r[a.blank];
        qn = cut ? r[nxt] : (T)0;
#pragma unroll
        for (int i = 0; i < M; i++) qc[i] = sym[i] >= 0 ? r[sym[i]] : (T)0;
    };
    if (nr > 0) {
        if constexpr (STAGED) {
            st.load(rows, a.nstate);
            st.store(re_rows, rows, a.nstate);
        } else gather(rows);
    }
    double fnext = (ok && nr >= 1) ? Fa[(size_t)v.ldj] : 0.0;
    double bnext = (cut && nr >= 1) ? Bd[(size_t)v.ldj] : 0.0;
    int64_t ef = 0, efn = nr >= 1 ? v.EF[1] : 0, ebc = v.EB[0], ebn = nr >= 1 ? v.EB[1] : 0;
    double acc = 0.0;
    int64_t acce = 0;
    if constexpr (STAGED) __syncthreads();

    for (int t = 0; t < nr; t++) {
        // one row ahead: the posterior row into registers, F, B and the exponents
        const T *rnext = rows + (size_t)(t + 1) * rstride;
        T vb, vn, vc[M];
        if constexpr (STAGED) {
            if (t + 1 < nr) st.load(rnext, a.nstate);
        } else {
            vb = qb;
            vn = qn;
#pragma unroll
            for (int i = 0; i < M; i++) vc[i] = qc[i];
            if (t + 1 < nr) gather(rnext);
        }
        double f2 = 0.0, b2 = 0.0;
        int64_t ef2 = 0, eb2 = 0;
        if (t + 2 <= nr) {
            if (ok) f2 = Fa[(size_t)(t + 2) * v.ldj];
            if (cut) b2 = Bd[(size_t)(t + 2) * v.ldj];
            ef2 = v.EF[t + 2];
            eb2 = v.EB[t + 2];
        }
        // row t + 1 of the posterior (index t), from LDS
        if constexpr (STAGED) {
            const T *rcur = rows + (size_t)t * rstride;
            const T *cur = reinterpret_cast<const T *>(re_rows + (size_t)(t & 1) * gran) + re_stage<T, NCH>::mis(rcur);
            vb = cur[a.blank];
            vn = cut ? cur[nxt] : (T)0;
#pragma unroll
            for (int i = 0; i < M; i++) vc[i] = sym[i] >= 0 ? cur[sym[i]] : (T)0;
        }
        const double pb = fs_widen(vb, raw, a.min_prob, a.one_m);
        const double pn = cut ? fs_widen(vn, raw, a.min_prob, a.one_m) : 0.0;
        double pc[M];
#pragma unroll
        for (int i = 0; i < M; i++) pc[i] = sym[i] >= 0 ? fs_widen(vc[i], raw, a.min_prob, a.one_m) : 0.0;
        // the cut term of t: paths that leave state a + m with row t + 1.  g carries the scale of row t of F, 2^(EF_{t+1} - EF_t) times
        // a value below 1, B_{t+1} that of its own row, 2^(EB_t - EB_{t+1}): the product of both and of the emission leaves the normal
        // range when neighbouring rows differ in scale, so B_{t+1} gives both scales up first (exact) and the exponent is EF_{t+1} + EB_t
        {
            const double term = (g[M] * pn) * ldexp(bnext, re_clamp_shift((ef - efn) + (ebn - ebc)));
            const int64_t e = efn + ebc;
            if (t == 0 || e > acce) {
                acc = ldexp(acc, re_clamp_shift(acce - e)) + term;
                acce = e;
            } else acc += ldexp(term, re_clamp_shift(e - acce));
        }
        // g_t -> g_{t+1}, scaled like row t + 1 of F
        const int de = re_clamp_shift(efn - ef);
#pragma unroll
        for (int i = M; i >= 1; i--) g[i] = i == inj ? fnext : ldexp(fma(g[i - 1], pc[i - 1], g[i] * pb), -de);
        g[0] = inj == 0 ? fnext : 0.0;
        fnext = f2;
        bnext = b2;
        ef = efn;
        efn = ef2;
        ebc = ebn;
        ebn = eb2;
        if constexpr (STAGED) {
            if (t + 1 < nr) st.store(re_rows + (size_t)((t + 1) & 1) * gran, rnext, a.nstate);
            __syncthreads();
        }
    }
    if (ok) {
        if (cut) A.ll[ci] = log(acc) + (double)acce * FS_LN2;
        else A.ll[ci] = log(g[M]) + (double)ef * FS_LN2;     // a + d = L: Z' = g_T[m]
    }
}

// doubles of workspace of one pair (host values): nothing for a pair the device refuses by its lengths
static inline size_t re_pair_doubles(int64_t np, int nr)
{
    if (np < 0 || np > FS_MAX_POSITIONS || nr < 0) return 0;
    return 2 * (size_t)(nr + 1) * (size_t)(re_ldj((int)np) + 1);
}

extern "C" size_t slk_rescore_edits_workspace_bytes(int nread, const int32_t *nrow, const int64_t *pos_off)
{
    if (nread < 1 || !nrow || !pos_off) return 0;
    size_t n = re_head_bytes(nread);
    for (int b = 0; b < nread; b++) n += sizeof(double) * re_pair_doubles(pos_off[b + 1] - pos_off[b], nrow[b]);
    return n;
}

extern "C" int slk_rescore_edits_max_new(void) { return SLK_RESCORE_MAX_NEW; }

template <typename T>
static int re_launch(const T *post, long ld, const int64_t *row_off, long row_step, const int32_t *nrow, int nstate, const int32_t *seq,
                     const int64_t *pos_off, int nread, int max_npos, int blank, float min_prob, const int32_t *cand_pair,
                     const int32_t *cand_start, const int32_t *cand_ndel, const int64_t *cand_new_off, const int32_t *cand_new,
                     int64_t ncand, double *score, double *ll_edit, void *workspace, size_t workspace_bytes, slk_stream_t stream)
{
    if (!post || !row_off || !nrow || !pos_off || !score || nread < 1 || nstate < 1 || ld < nstate || row_step < 1 || max_npos < 0 ||
        blank < 0 || blank >= nstate || !(min_prob >= 0.0f) || !(min_prob < 1.0f) || (!seq && max_npos > 0) || ncand < 0 ||
        (ncand > 0 && (!cand_pair || !cand_start || !cand_ndel || !cand_new_off || !ll_edit)))
        return SLK_ERR_INVALID_ARG;
    if (max_npos > FS_MAX_POSITIONS || nstate > RE_MAX_STATES) return SLK_ERR_UNSUPPORTED;
    if (!workspace || (reinterpret_cast<uintptr_t>(workspace) & 15)) return SLK_ERR_WORKSPACE;
    hipStream_t s = slk_stream(stream);
    // the lengths and the candidates' pairs live on the device: they come to the host once, for the exact size and the offsets
    std::vector<int32_t> h_nrow(nread), h_pair((size_t)ncand);
    std::vector<int64_t> h_pos(nread + 1), h_head(2 * (size_t)(nread + 1));
    int64_t nnew = 0;
    if (hipStreamSynchronize(s) != hipSuccess || hipMemcpy(h_nrow.data(), nrow, sizeof(int32_t) * nread, hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(h_pos.data(), pos_off, sizeof(int64_t) * (nread + 1), hipMemcpyDeviceToHost) != hipSuccess)
        return SLK_ERR_LAUNCH;
    if (ncand > 0 && (hipMemcpy(h_pair.data(), cand_pair, sizeof(int32_t) * (size_t)ncand, hipMemcpyDeviceToHost) != hipSuccess ||
                      hipMemcpy(&nnew, cand_new_off + ncand, sizeof(int64_t), hipMemcpyDeviceToHost) != hipSuccess))
        return SLK_ERR_LAUNCH;
    if (nnew < 0 || (nnew > 0 && !cand_new)) return SLK_ERR_INVALID_ARG;
    if (workspace_bytes < slk_rescore_edits_workspace_bytes(nread, h_nrow.data(), h_pos.data())) return SLK_ERR_WORKSPACE;
    // candidates come grouped by pair, pairs ascending: cand_off[b] is the first candidate of pair b
    int64_t *h_off = h_head.data(), *h_coff = h_head.data() + (nread + 1);
    int64_t most = 0;
    {
        int64_t i = 0;
        for (int b = 0; b < nread; b++) {
            h_coff[b] = i;
            while (i < ncand && h_pair[(size_t)i] == b) i++;
            if (i - h_coff[b] > most) most = i - h_coff[b];
        }
        h_coff[nread] = i;
        if (i != ncand) return SLK_ERR_INVALID_ARG;           // a pair outside 0 .. nread - 1, or pairs out of order
    }
    const int64_t ygrid = (most + RE_CAND - 1) / RE_CAND;
    if (ygrid > 65535) return SLK_ERR_UNSUPPORTED;
    h_off[0] = (int64_t)(re_head_bytes(nread) / sizeof(double));
    for (int b = 0; b < nread; b++) h_off[b + 1] = h_off[b] + (int64_t)re_pair_doubles(h_pos[b + 1] - h_pos[b], h_nrow[b]);
    if (hipMemcpy(workspace, h_head.data(), sizeof(int64_t) * h_head.size(), hipMemcpyHostToDevice) != hipSuccess) return SLK_ERR_LAUNCH;

    re_args A;
    fs_args &a = A.f;
    a.post = post; a.ld = ld; a.row_step = row_step; a.row_off = row_off; a.nrow = nrow; a.seq = seq; a.pos_off = pos_off;
    a.score_out = score; a.nstate = nstate; a.blank = blank; a.full = 1;
    a.min_prob = min_prob; a.one_m = one_minus(min_prob, (double)min_prob);
    A.ws = static_cast<double *>(workspace); A.ws_off = static_cast<const int64_t *>(workspace);
    A.cand_off = A.ws_off + (nread + 1);
    A.cand_start = cand_start; A.cand_ndel = cand_ndel; A.cand_new = cand_new; A.cand_new_off = cand_new_off; A.nnew = nnew;
    A.ll = ll_edit;

    if (max_npos < 2 * FS_THREADS) hipLaunchKernelGGL((rescore_lattice_kernel<T, 2>), dim3(nread), dim3(FS_THREADS), 0, s, A);
    else if (max_npos < 8 * FS_THREADS) hipLaunchKernelGGL((rescore_lattice_kernel<T, 8>), dim3(nread), dim3(FS_THREADS), 0, s, A);
    else hipLaunchKernelGGL((rescore_lattice_kernel<T, 32>), dim3(nread), dim3(FS_THREADS), 0, s, A);
    int rc = slk_launch_status();
    if (rc != SLK_OK || ygrid == 0) return rc;

    // granules of 16 bytes per staged row: the row's bytes and one more for its alignment
    const int gran = (int)(((size_t)nstate * sizeof(T) + 15) / 16) + 1;
    const size_t lds = 2 * sizeof(uint4) * (size_t)gran;
    auto launch = [&](auto kernel) {
        if (lds > 64 * 1024) {
            const bool ok = SLK_PER_DEVICE(bool, hipFuncSetAttribute(reinterpret_cast<const void *>(kernel),
                                                                     hipFuncAttributeMaxDynamicSharedMemorySize,
                                                                     (int)(2 * sizeof(uint4) * (RE_MAX_STATES * sizeof(T) / 16 + 1))) == hipSuccess);
            if (!ok) return (int)SLK_ERR_UNSUPPORTED;
        }
        hipLaunchKernelGGL(kernel, dim3(nread, (unsigned)ygrid), dim3(RE_CAND), lds, s, A, gran);
        return slk_launch_status();
    };
    const int per = (gran + RE_CAND - 1) / RE_CAND;
#ifdef SLK_DIAG
    if (const char *env = getenv("SLK_DIAG_RESCORE_GATHER"); env && env[0] == '1') {
        hipLaunchKernelGGL((rescore_cand_kernel<T, 1, false>), dim3(nread, (unsigned)ygrid), dim3(RE_CAND), 0, s, A, gran);
        return slk_launch_status();
    }
#endif
    if (per <= 2) return launch(rescore_cand_kernel<T, 2, true>);
    if (per <= 5) return launch(rescore_cand_kernel<T, 5, true>);
    return launch(rescore_cand_kernel<T, 17, true>);
}

extern "C" int slk_rescore_edits_batch_f32(const float *post, long ld, const int64_t *row_off, long row_step, const int32_t *nrow,
                                           int nstate, const int32_t *seq, const int64_t *pos_off, int nread, int max_npos, int blank,
                                           float min_prob, const int32_t *cand_pair, const int32_t *cand_start, const int32_t *cand_ndel,
                                           const int64_t *cand_new_off, const int32_t *cand_new, int64_t ncand, double *score,
                                           double *ll_edit, void *workspace, size_t workspace_bytes, slk_stream_t stream)
{
    return re_launch<float>(post, ld, row_off, row_step, nrow, nstate, seq, pos_off, nread, max_npos, blank, min_prob, cand_pair,
                            cand_start, cand_ndel, cand_new_off, cand_new, ncand, score, ll_edit, workspace, workspace_bytes, stream);
}

extern "C" int slk_rescore_edits_batch_f64(const double *post, long ld, const int64_t *row_off, long row_step, const int32_t *nrow,
                                           int nstate, const int32_t *seq, const int64_t *pos_off, int nread, int max_npos, int blank,
                                           const int32_t *cand_pair, const int32_t *cand_start, const int32_t *cand_ndel,
                                           const int64_t *cand_new_off, const int32_t *cand_new, int64_t ncand, double *score,
                                           double *ll_edit, void *workspace, size_t workspace_bytes, slk_stream_t stream)
{
    return re_launch<double>(post, ld, row_off, row_step, nrow, nstate, seq, pos_off, nread, max_npos, blank, 0.0f, cand_pair, cand_start,
                             cand_ndel, cand_new_off, cand_new, ncand, score, ll_edit, workspace, workspace_bytes, stream);
}
