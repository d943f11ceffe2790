// rescore_band.hip -- rescore_edits.hip for whole reads: the same forward score of EDITED sequences, from lattices that keep a band
// of W states per row instead of all L + 1 (design/rescore_band.md).  A pair carries lo[0 .. T]: state j exists in row t when
// lo[t] <= j < lo[t] + W and 0 <= j <= L; F and B follow the dense recursions with every other state equal to 0, the scaling is
// the dense one with the row total taken over the band, and a candidate's chain and cut sum run over the rows in which its columns
// a and a + d + 1 exist.  With lo all 0 and W >= L + 1 every bit is rescore_edits.hip's.
//
// Lattice kernel: one workgroup of 256 threads per pair, W = 256 * PPT, RING ownership: state j lives in slot j mod W and thread i
// holds slots i * PPT .. i * PPT + PPT - 1 in registers for the whole pass.  The state of slot s in row t is lo[t] + ((s - lo[t]) mod W);
// when lo passes a slot's state the slot's value counts as 0 and the slot takes the state W above.  Nothing moves between threads but
// the one neighbour value per row of the dense kernel (the left neighbour of thread 0 is thread 255); whether a slot's own value and
// its neighbour's belong to the states the recursion asks for is decided from lo[t] and lo[t + 1] alone.  Rows are stored
// ring-indexed:  F [T+1][W] | B [T+1][W] | EF [T+1] | EB [T+1]  (float64, int64).
//
// Candidate kernel: rescore_edits.hip's (one lane per candidate, the posterior row staged in LDS, the chain in the fixed slots
// g[0..8]).  Each lane finds the first row of column a and the last row of column a + d + 1 by binary search in lo; the workgroup
// walks from the smallest first row to the largest end of its lanes; a lattice read checks lo[t] <= j < lo[t] + W and yields 0
// outside (the ring slot holds another state's value there); a lane adds terms in its own range only, and its own first term
// initialises its sum, so nothing a lane computes depends on its neighbours.
#include <vector>

#include "rescore_common.h"

#define RB_MAX_WIDTH 2048                                     // (256 * 8; wider rings are not built: design/rescore_band.md 3)
#define RB_MAX_POSITIONS (INT32_MAX - 2 * 8192 - 2)           // (state arithmetic stays inside int32)

struct rb_args {
    fs_args f;                                                // (full = 1; score_out = the pairs' scores)
    double *ws;
    const int64_t *ws_off;
    const int64_t *cand_off;
    const int32_t *band_lo;                                   // pair b's lo[0 .. nrow[b]] begins at band_off[b]
    const int64_t *band_off;
    int width;
    const int32_t *cand_start, *cand_ndel, *cand_new;
    const int64_t *cand_new_off;
    int64_t nnew;
    double *ll;
};

struct rb_view {
    double *F, *B;
    int64_t *EF, *EB;
};
__device__ __forceinline__ rb_view rb_pair_view(double *base, int W, int nr)
{
    rb_view v;
    const size_t n = (size_t)(nr + 1) * (size_t)W;
    v.F = base;
    v.B = base + n;
    v.EF = reinterpret_cast<int64_t *>(base + 2 * n);
    v.EB = v.EF + (nr + 1);
    return v;
}

// lo[t] as the kernels use it: a row whose band begins behind state L has no state at all, wherever it begins
__device__ __forceinline__ int rb_lo(const int32_t *lo, int t, int L)
{
    const int v = lo[t];
    return v > L ? L + 1 : v;
}

template <int PPT>
__device__ __forceinline__ void rb_store_row(double *row, int j0, const double (&f)[PPT])
{
    if constexpr (PPT == 1) row[j0] = f[0];
    else {
#pragma unroll
        for (int k = 0; k < PPT; k += 2) *reinterpret_cast<double2 *>(row + j0 + k) = make_double2(f[k], f[k + 1]);
    }
}

template <typename T, int PPT>
__global__ void __launch_bounds__(FS_THREADS) rescore_band_lattice_kernel(rb_args A)
{
    __shared__ double wsum[2][FS_WAVES];
    __shared__ double edge[2][FS_THREADS];
    __shared__ double endv;
    constexpr int W = FS_THREADS * PPT, MASK = W - 1;
    constexpr int D = fs_ahead<PPT>::value;
    const fs_args &a = A.f;
    const int b = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int64_t np = a.pos_off[b + 1] - a.pos_off[b];
    const int nr = a.nrow[b];
    if (np < 0 || np > RB_MAX_POSITIONS || nr < 0) {
        if (tid == 0) a.score_out[b] = RE_NAN;
        return;
    }
    const int L = (int)np;
    const int j0 = tid * PPT;
    const bool raw = a.min_prob > 0.0f;
    const int32_t *seq = a.seq + a.pos_off[b];
    const int32_t *lo = A.band_lo + A.band_off[b];
    const T *rows = static_cast<const T *>(a.post) + (size_t)a.row_off[b] * (size_t)a.ld;
    const size_t rstride = (size_t)a.row_step * (size_t)a.ld;

    // the band and the symbols, before anything is written
    {
        bool bad = false;
        for (int t = tid; t <= nr; t += FS_THREADS) {
            const int v = lo[t];
            if (v < 0 || (t == 0 ? v != 0 : v < lo[t - 1])) bad = true;
            if (t == nr && (int64_t)v + W <= (int64_t)L) bad = true;
        }
        for (int j = tid; j < L; j += FS_THREADS) {
            const int c = seq[j];
            if (c < 0 || c >= a.nstate) bad = true;
        }
        if (tid == 0) endv = 0.0;
        if (__syncthreads_or(bad ? 1 : 0)) {                  // an invalid band, a symbol that is no column: NaN, nothing else is written
            if (tid == 0) a.score_out[b] = RE_NAN;
            return;
        }
    }
    const rb_view v = rb_pair_view(A.ws + A.ws_off[b], W, nr);

    // eb, ee: the emissions of posterior row p, fetched D rows ahead for the states the slots hold in the row they are fetched FOR;
    // lrow: that row's lo
    T eb[D], ee[D][PPT];
    int lrow[D];
    auto clear = [&](int slot) {
        eb[slot] = (T)0;
        lrow[slot] = 0;
#pragma unroll
        for (int k = 0; k < PPT; k++) ee[slot][k] = (T)0;
    };
    auto fetch_up = [&](int slot, int p) {                    // pass 1: row p + 1 is made; slot s holds state j, entered with seq[j - 1]
        const T *r = rows + (size_t)p * rstride;
        const int ln = rb_lo(lo, p + 1, L);
        lrow[slot] = ln;
        eb[slot] = r[a.blank];
#pragma unroll
        for (int k = 0; k < PPT; k++) {
            const int j = ln + ((j0 + k - ln) & MASK);
            ee[slot][k] = (j >= 1 && j <= L) ? r[seq[j - 1]] : (T)0;
        }
    };
    auto fetch_down = [&](int slot, int p) {                  // pass 2: row p is made; state j is left with seq[j]
        const T *r = rows + (size_t)p * rstride;
        const int lc = rb_lo(lo, p, L);
        lrow[slot] = lc;
        eb[slot] = r[a.blank];
#pragma unroll
        for (int k = 0; k < PPT; k++) {
            const int j = lc + ((j0 + k - lc) & MASK);
            ee[slot][k] = j < L ? r[seq[j]] : (T)0;
        }
    };

    // ---- pass 1: F_0 .. F_T.  lo[0] = 0: slot s holds state s
#pragma unroll
    for (int d = 0; d < D; d++) {
        if (d < nr) fetch_up(d, d);
        else clear(d);
    }
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
        rb_store_row<PPT>(v.F, j0, f);
        if (tid == 0) v.EF[0] = 0;
    }
    __syncthreads();
    int64_t esum = 0;
    int lcur = 0;                                             // lo of the row the registers hold
    for (int p0 = 0; p0 < nr; p0 += D) {
#pragma unroll
        for (int d = 0; d < D; d++) {
            const int p = p0 + d;
            if (p >= nr) break;                               // (the same for the whole workgroup)
            const int par = p & 1;
            const int ln = lrow[d];
            const double pb = fs_widen(eb[d], raw, a.min_prob, a.one_m);
            int jn[PPT];
            double pe[PPT];
#pragma unroll
            for (int k = 0; k < PPT; k++) {
                jn[k] = ln + ((j0 + k - ln) & MASK);
                pe[k] = (jn[k] >= 1 && jn[k] <= L) ? fs_widen(ee[d][k], raw, a.min_prob, a.one_m) : 0.0;
            }
            if (p + D < nr) fetch_up(d, p + D);
            const double m = re_sum4(wsum[par ^ 1]);
            int e = 0;
            if (m > 0.0 && m < INFINITY) (void)frexp(m, &e);
            esum += e;
            double prev = edge[par ^ 1][(tid - 1) & (FS_THREADS - 1)];
            double s = 0.0;
#pragma unroll
            for (int k = 0; k < PPT; k++) {
                // the slot's value is F_p[jn] when jn was in row p's band already; its neighbour's is F_p[jn - 1] when that was
                const double own = jn[k] - lcur < W ? f[k] : 0.0;
                const double left = (jn[k] - 1 >= lcur && jn[k] - 1 - lcur < W) ? prev : 0.0;
                const double g = fma(left, pe[k], own * pb);
                prev = f[k];
                f[k] = ldexp(g, -e);                          // exact: a power of two
                s += f[k];
            }
            lcur = ln;
            rb_store_row<PPT>(v.F + (size_t)(p + 1) * W, j0, f);
            if (tid == 0) v.EF[p + 1] = esum;
            s = fs_wave_sum(s);
            if (lane == 0) wsum[par][wave] = s;
            edge[par][tid] = f[PPT - 1];
            __syncthreads();
        }
    }
    const int lT = rb_lo(lo, nr, L);
    if (lT <= L) {                                            // (otherwise state L is outside the last row: endv stays 0)
#pragma unroll
        for (int k = 0; k < PPT; k++)
            if (j0 + k == (L & MASK)) endv = f[k];
    }
    __syncthreads();                                          // (wsum and edge are free again behind it)
    if (tid == 0) a.score_out[b] = log(endv) + (double)esum * FS_LN2;

    // ---- pass 2: B_T .. B_0, down the same ring: a slot now hands its state BACK when lo falls below it
#pragma unroll
    for (int d = 0; d < D; d++) {
        if (d < nr) fetch_down(d, nr - 1 - d);
        else clear(d);
    }
    double bb[PPT];
    {
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < PPT; k++) {
            bb[k] = lT + ((j0 + k - lT) & MASK) == L ? 1.0 : 0.0;
            s += bb[k];
        }
        s = fs_wave_sum(s);
        if (lane == 0) wsum[nr & 1][wave] = s;
        edge[nr & 1][tid] = bb[0];
        rb_store_row<PPT>(v.B + (size_t)nr * W, j0, bb);
        if (tid == 0) v.EB[nr] = 0;
    }
    __syncthreads();
    esum = 0;
    int lup = lT;                                             // lo of the row the registers hold
    for (int i0 = 0; i0 < nr; i0 += D) {
#pragma unroll
        for (int d = 0; d < D; d++) {
            if (i0 + d >= nr) break;
            const int p = nr - 1 - (i0 + d);
            const int par = p & 1;
            const int lc = lrow[d];
            const double pb = fs_widen(eb[d], raw, a.min_prob, a.one_m);
            int jc[PPT];
            double pe[PPT];
#pragma unroll
            for (int k = 0; k < PPT; k++) {
                jc[k] = lc + ((j0 + k - lc) & MASK);
                pe[k] = jc[k] < L ? fs_widen(ee[d][k], raw, a.min_prob, a.one_m) : 0.0;
            }
            if (p - D >= 0) fetch_down(d, p - D);
            const double m = re_sum4(wsum[par ^ 1]);
            int e = 0;
            if (m > 0.0 && m < INFINITY) (void)frexp(m, &e);
            esum += e;
            const double right = edge[par ^ 1][(tid + 1) & (FS_THREADS - 1)];
            double s = 0.0;
#pragma unroll
            for (int k = 0; k < PPT; k++) {
                const double nb = k + 1 < PPT ? bb[(k + 1) % PPT] : right;
                // the slot's value is B_{p+1}[jc] when jc is in row p + 1's band; its right neighbour's is B_{p+1}[jc + 1] when that is
                const double own = jc[k] >= lup ? bb[k] : 0.0;
                const double rv = (jc[k] + 1 >= lup && jc[k] + 1 - lup < W) ? nb : 0.0;
                const double g = fma(rv, pe[k], own * pb);
                bb[k] = ldexp(g, -e);
                s += bb[k];
            }
            lup = lc;
            rb_store_row<PPT>(v.B + (size_t)p * W, j0, bb);
            if (tid == 0) v.EB[p] = esum;
            s = fs_wave_sum(s);
            if (lane == 0) wsum[par][wave] = s;
            edge[par][tid] = bb[0];
            __syncthreads();
        }
    }
}

// ---- the candidates ------------------------------------------------------------------------------------------------------------

// the first t of 0 .. nr with lo[t] > x (nr + 1: none); lo does not decrease
__device__ __forceinline__ int rb_first_above(const int32_t *lo, int nr, int x)
{
    int l = 0, h = nr + 1;
    while (l < h) {
        const int mid = (l + h) >> 1;
        if (lo[mid] > x) h = mid;
        else l = mid + 1;
    }
    return l;
}

template <typename T, int NCH>
__global__ void __launch_bounds__(RE_CAND) rescore_band_cand_kernel(rb_args A, int gran)
{
    extern __shared__ __attribute__((aligned(16))) uint4 rb_rows[];      // [2][gran] granules of 16 bytes, then the workgroup's row range
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
    const int W = A.width, MASK = W - 1;
    const int L = (int)(a.pos_off[b + 1] - a.pos_off[b]);
    const int nr = a.nrow[b];
    const int32_t *seq = a.seq + a.pos_off[b];
    const int32_t *lo = A.band_lo + A.band_off[b];
    const bool raw = a.min_prob > 0.0f;
    const T *rows = static_cast<const T *>(a.post) + (size_t)a.row_off[b] * (size_t)a.ld;
    const size_t rstride = (size_t)a.row_step * (size_t)a.ld;
    const rb_view v = rb_pair_view(A.ws + A.ws_off[b], W, nr);
    int *range = reinterpret_cast<int *>(rb_rows + 2 * (size_t)gran);

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
    const int cb = ca + cd + 1;                               // (column of B; read only with a + d < L)

    // the lane's rows: column a exists from row t0 on; the terms t run to t1(a + d + 1) - 1, a chain that ends the sequence to row T
    int t0 = 0, tend = 0;
    if (ok) {
        t0 = rb_first_above(lo, nr, ca - W);
        tend = cut ? rb_first_above(lo, nr, cb) - 1 : nr;
        if (t0 > nr) t0 = nr;                                 // (cannot happen in a valid band)
    }
    if (tid == 0) {
        range[0] = nr;
        range[1] = 0;
    }
    __syncthreads();
    if (ok) {
        atomicMin(&range[0], t0);
        atomicMax(&range[1], tend);
    }
    __syncthreads();
    const int tmin = range[0], tmax = range[1];               // (tmin = nr without any candidate)

    auto readF = [&](int t) {
        const int l = lo[t];
        return (ok && ca >= l && ca - l < W) ? v.F[(size_t)t * W + (ca & MASK)] : 0.0;
    };
    auto readB = [&](int t) {
        const int l = lo[t];
        return (cut && cb >= l && cb - l < W) ? v.B[(size_t)t * W + (cb & MASK)] : 0.0;
    };

    // The chain sits at the END of g: slot inj = M - m takes F_t[a], slot i > inj is g_t[i - inj] and is entered with sym[i - 1], and
    // g[M] is always g_t[m].  Every slot has a fixed register; the slots below inj hold 0 and are entered with 0.
    const int inj = M - m;
    double g[M + 1];
    {
        const double f0 = readF(tmin);
#pragma unroll
        for (int i = 0; i <= M; i++) g[i] = i == inj ? f0 : 0.0;
    }

    re_stage<T, NCH> st;
    if (tmin < tmax) {
        const T *r0 = rows + (size_t)tmin * rstride;
        st.load(r0, a.nstate);
        st.store(rb_rows + (size_t)(tmin & 1) * gran, r0, a.nstate);
    }
    double fnext = tmin + 1 <= nr ? readF(tmin + 1) : 0.0;
    double bnext = tmin + 1 <= nr ? readB(tmin + 1) : 0.0;
    int64_t ef = v.EF[tmin], efn = tmin + 1 <= nr ? v.EF[tmin + 1] : 0, ebc = v.EB[tmin], ebn = tmin + 1 <= nr ? v.EB[tmin + 1] : 0;
    double acc = 0.0;
    int64_t acce = 0;
    __syncthreads();

    for (int t = tmin; t < tmax; t++) {
        // one row ahead: the posterior row into registers, F, B and the exponents
        const T *rnext = rows + (size_t)(t + 1) * rstride;
        if (t + 1 < tmax) st.load(rnext, a.nstate);
        double f2 = 0.0, b2 = 0.0;
        int64_t ef2 = 0, eb2 = 0;
        if (t + 2 <= nr) {
            f2 = readF(t + 2);
            b2 = readB(t + 2);
            ef2 = v.EF[t + 2];
            eb2 = v.EB[t + 2];
        }
        // row t + 1 of the posterior (index t), from LDS
        T vb, vn, vc[M];
        {
            const T *rcur = rows + (size_t)t * rstride;
            const T *cur = reinterpret_cast<const T *>(rb_rows + (size_t)(t & 1) * gran) + re_stage<T, NCH>::mis(rcur);
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
        // the cut term of t (design/rescore_edits.md 5, step 1), in the lane's own range only; its first term initialises the sum
        if (t >= t0 && t < tend) {
            const double term = (g[M] * pn) * ldexp(bnext, re_clamp_shift((ef - efn) + (ebn - ebc)));
            const int64_t e = efn + ebc;
            if (t == t0 || e > acce) {
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
        if (t + 1 < tmax) st.store(rb_rows + (size_t)((t + 1) & 1) * gran, rnext, a.nstate);
        __syncthreads();
    }
    if (ok) {
        if (cut) A.ll[ci] = log(acc) + (double)acce * FS_LN2;
        else A.ll[ci] = log(g[M]) + (double)ef * FS_LN2;     // a + d = L: Z' = g_T[m]
    }
}

// ---- the entry -------------------------------------------------------------------------------------------------------------------

static inline bool rb_width_built(int width)
{
    return width == 256 || width == 512 || width == 1024 || width == 2048;
}

// doubles of workspace of one pair (host values)
static inline size_t rb_pair_doubles(int nr, int width) { return nr < 0 ? 0 : 2 * (size_t)(nr + 1) * (size_t)(width + 1); }

extern "C" int slk_rescore_band_max_width(void) { return RB_MAX_WIDTH; }

extern "C" size_t slk_rescore_edits_banded_workspace_bytes(int nread, const int32_t *nrow, int width)
{
    if (nread < 1 || !nrow || !rb_width_built(width)) return 0;
    size_t n = re_head_bytes(nread);
    for (int b = 0; b < nread; b++) n += sizeof(double) * rb_pair_doubles(nrow[b], width);
    return n;
}

template <typename T>
static int rb_launch(const T *post, long ld, const int64_t *row_off, long row_step, const int32_t *nrow, int nstate, const int32_t *seq,
                     const int64_t *pos_off, int nread, int blank, float min_prob, const int32_t *band_lo, const int64_t *band_off,
                     int width, const int32_t *cand_pair, const int32_t *cand_start, const int32_t *cand_ndel,
                     const int64_t *cand_new_off, const int32_t *cand_new, int64_t ncand, double *score, double *ll_edit,
                     void *workspace, size_t workspace_bytes, slk_stream_t stream)
{
    if (!post || !row_off || !nrow || !pos_off || !score || nread < 1 || nstate < 1 || ld < nstate || row_step < 1 || blank < 0 ||
        blank >= nstate || !(min_prob >= 0.0f) || !(min_prob < 1.0f) || !band_lo || !band_off || !rb_width_built(width) || ncand < 0 ||
        (ncand > 0 && (!cand_pair || !cand_start || !cand_ndel || !cand_new_off || !ll_edit)))
        return SLK_ERR_INVALID_ARG;
    if (nstate > RE_MAX_STATES) return SLK_ERR_UNSUPPORTED;
    if (!workspace || (reinterpret_cast<uintptr_t>(workspace) & 15)) return SLK_ERR_WORKSPACE;
    hipStream_t s = slk_stream(stream);
    // the lengths, the band's offsets and the candidates' pairs live on the device: they come to the host once
    std::vector<int32_t> h_nrow(nread), h_pair((size_t)ncand);
    std::vector<int64_t> h_pos(nread + 1), h_band(nread + 1), h_head(2 * (size_t)(nread + 1));
    int64_t nnew = 0;
    if (hipStreamSynchronize(s) != hipSuccess || hipMemcpy(h_nrow.data(), nrow, sizeof(int32_t) * nread, hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(h_pos.data(), pos_off, sizeof(int64_t) * (nread + 1), hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(h_band.data(), band_off, sizeof(int64_t) * (nread + 1), hipMemcpyDeviceToHost) != hipSuccess)
        return SLK_ERR_LAUNCH;
    if (ncand > 0 && (hipMemcpy(h_pair.data(), cand_pair, sizeof(int32_t) * (size_t)ncand, hipMemcpyDeviceToHost) != hipSuccess ||
                      hipMemcpy(&nnew, cand_new_off + ncand, sizeof(int64_t), hipMemcpyDeviceToHost) != hipSuccess))
        return SLK_ERR_LAUNCH;
    if (nnew < 0 || (nnew > 0 && !cand_new)) return SLK_ERR_INVALID_ARG;
    bool any_seq = false;
    for (int b = 0; b < nread; b++) {                         // pair b's nrow[b] + 1 entries of lo, one pair behind the other
        if (h_nrow[b] < 0 || h_band[b] < 0 || h_band[b + 1] - h_band[b] != (int64_t)h_nrow[b] + 1) return SLK_ERR_INVALID_ARG;
        const int64_t np = h_pos[b + 1] - h_pos[b];
        if (np > RB_MAX_POSITIONS) return SLK_ERR_UNSUPPORTED;
        any_seq = any_seq || np > 0;
    }
    if (any_seq && !seq) return SLK_ERR_INVALID_ARG;
    if (workspace_bytes < slk_rescore_edits_banded_workspace_bytes(nread, h_nrow.data(), width)) return SLK_ERR_WORKSPACE;
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
    for (int b = 0; b < nread; b++) h_off[b + 1] = h_off[b] + (int64_t)rb_pair_doubles(h_nrow[b], width);
    if (hipMemcpy(workspace, h_head.data(), sizeof(int64_t) * h_head.size(), hipMemcpyHostToDevice) != hipSuccess) return SLK_ERR_LAUNCH;

    rb_args A;
    fs_args &a = A.f;
    a.post = post; a.ld = ld; a.row_step = row_step; a.row_off = row_off; a.nrow = nrow; a.seq = seq; a.pos_off = pos_off;
    a.score_out = score; a.nstate = nstate; a.blank = blank; a.full = 1;
    a.min_prob = min_prob; a.one_m = one_minus(min_prob, (double)min_prob);
    A.ws = static_cast<double *>(workspace); A.ws_off = static_cast<const int64_t *>(workspace);
    A.cand_off = A.ws_off + (nread + 1);
    A.band_lo = band_lo; A.band_off = band_off; A.width = width;
    A.cand_start = cand_start; A.cand_ndel = cand_ndel; A.cand_new = cand_new; A.cand_new_off = cand_new_off; A.nnew = nnew;
    A.ll = ll_edit;

    switch (width) {
    case 256: hipLaunchKernelGGL((rescore_band_lattice_kernel<T, 1>), dim3(nread), dim3(FS_THREADS), 0, s, A); break;
    case 512: hipLaunchKernelGGL((rescore_band_lattice_kernel<T, 2>), dim3(nread), dim3(FS_THREADS), 0, s, A); break;
    case 1024: hipLaunchKernelGGL((rescore_band_lattice_kernel<T, 4>), dim3(nread), dim3(FS_THREADS), 0, s, A); break;
    default: hipLaunchKernelGGL((rescore_band_lattice_kernel<T, 8>), dim3(nread), dim3(FS_THREADS), 0, s, A); break;
    }
    int rc = slk_launch_status();
    if (rc != SLK_OK || ygrid == 0) return rc;

    // granules of 16 bytes per staged row: the row's bytes and one more for its alignment; one granule more for the row range
    const int gran = (int)(((size_t)nstate * sizeof(T) + 15) / 16) + 1;
    const size_t lds = sizeof(uint4) * (2 * (size_t)gran + 1);
    auto launch = [&](auto kernel) {
        if (lds > 64 * 1024) {
            const bool ok = SLK_PER_DEVICE(bool, hipFuncSetAttribute(reinterpret_cast<const void *>(kernel),
                                                                     hipFuncAttributeMaxDynamicSharedMemorySize,
                                                                     (int)(sizeof(uint4) * (2 * (RE_MAX_STATES * sizeof(T) / 16 + 1) + 1))) == hipSuccess);
            if (!ok) return (int)SLK_ERR_UNSUPPORTED;
        }
        hipLaunchKernelGGL(kernel, dim3(nread, (unsigned)ygrid), dim3(RE_CAND), lds, s, A, gran);
        return slk_launch_status();
    };
    const int per = (gran + RE_CAND - 1) / RE_CAND;
    if (per <= 2) return launch(rescore_band_cand_kernel<T, 2>);
    if (per <= 5) return launch(rescore_band_cand_kernel<T, 5>);
    return launch(rescore_band_cand_kernel<T, 17>);
}

extern "C" int slk_rescore_edits_banded_batch_f32(const float *post, long ld, const int64_t *row_off, long row_step, const int32_t *nrow,
                                                  int nstate, const int32_t *seq, const int64_t *pos_off, int nread, int blank,
                                                  float min_prob, const int32_t *band_lo, const int64_t *band_off, int width,
                                                  const int32_t *cand_pair, const int32_t *cand_start, const int32_t *cand_ndel,
                                                  const int64_t *cand_new_off, const int32_t *cand_new, int64_t ncand, double *score,
                                                  double *ll_edit, void *workspace, size_t workspace_bytes, slk_stream_t stream)
{
    return rb_launch<float>(post, ld, row_off, row_step, nrow, nstate, seq, pos_off, nread, blank, min_prob, band_lo, band_off, width,
                            cand_pair, cand_start, cand_ndel, cand_new_off, cand_new, ncand, score, ll_edit, workspace, workspace_bytes,
                            stream);
}

extern "C" int slk_rescore_edits_banded_batch_f64(const double *post, long ld, const int64_t *row_off, long row_step, const int32_t *nrow,
                                                  int nstate, const int32_t *seq, const int64_t *pos_off, int nread, int blank,
                                                  const int32_t *band_lo, const int64_t *band_off, int width, const int32_t *cand_pair,
                                                  const int32_t *cand_start, const int32_t *cand_ndel, const int64_t *cand_new_off,
                                                  const int32_t *cand_new, int64_t ncand, double *score, double *ll_edit,
                                                  void *workspace, size_t workspace_bytes, slk_stream_t stream)
{
    return rb_launch<double>(post, ld, row_off, row_step, nrow, nstate, seq, pos_off, nread, blank, 0.0f, band_lo, band_off, width,
                             cand_pair, cand_start, cand_ndel, cand_new_off, cand_new, ncand, score, ll_edit, workspace, workspace_bytes,
                             stream);
}
