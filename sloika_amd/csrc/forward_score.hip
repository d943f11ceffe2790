// forward_score.hip -- the sum-product score of a sequence under a transducer posterior on gfx950:
//
//   decode.score / decode.forwards          sloika/decode.py:96-139
//
//     f[0..L] = 1                      (full: f = e_0)
//     per row p:   g[j] = f[j] * p[blank] + (j >= 1) f[j-1] * p[seq[j-1]]
//                  m = sum g ;  f = g / m ;  score += log m
//     return score (+ log f[L] if full)
//
// for a ragged batch of (posterior, sequence) pairs, one workgroup of 256 threads per pair, float64 throughout (numpy 2 runs the
// reference in float64 from the first product on, for float32 rows too; widening a float32 value is exact).
//
// Ownership.  A pair of L positions has L + 1 states.  Thread i owns the `ppt` consecutive states i * ppt .. i * ppt + ppt - 1, in
// registers, where ppt is the smallest of 1, 2, 4, 8, 16, 32 with 256 * ppt >= L + 1: it depends on the pair alone, never on the
// batch.  Hence the limit: L <= 256 * 32 - 1 = 8191 (slk_forward_score_max_positions).  States past L are zero and stay zero.
//
// Scaling (design/forward_score.md).  The score does not depend on the scaling mathematically, and the reference's division by the
// row's own total would put a reduction, a division and a log on the chain of every row.  Here a row is scaled by a POWER OF TWO:
// 2^-e with e the binary exponent (frexp) of the PREVIOUS row's total, which every thread reads behind the one barrier a row needs
// anyway.  That scaling is exact, so it adds no rounding at all; the exponents add up in an integer and the score is
//     log(total of the last row) + ln 2 * sum e        (full: log of the end state's value instead of the total).
// One log per pair, none per row.  The running total stays within a row's factor of [1/2, 1), as in the reference, so a `full` score
// whose end state holds less than the smallest float64 of the mass is -inf here as there; with L > T the end state is exactly 0.
//
// A row, per thread:  g[j] = fma(f[j-1], p[seq[j-1]], f[j] * p[blank]) for its states in ascending order (f[j-1] of its first state
// is the left neighbour's last, through LDS), scaled, and summed in the same order; the 64 sums of a wave combine by DPP (pairs,
// quads, eights, sixteens), the four rows of 16 as (r0 + r1) + (r2 + r3), and the four waves as ((w0 + w1) + w2) + w3 by every thread.
// All of it depends on the pair alone: a pair's score has the same bits alone, in any batch, in either layout and in any launch.
//
// The emission values of a row do not depend on the state: they are fetched fs_ahead rows ahead of their use into a register ring
// (gathers from global memory; with min_prob > 0 each float32 value goes through prepare_post_val first).
// No MFMA and no inline asm: plain C++, DPP and lane builtins.
#include "post_transform.h"

#define FS_THREADS 256
#define FS_WAVES (FS_THREADS / 64)
#define FS_MAX_PPT 32
#define FS_MAX_POSITIONS (FS_THREADS * FS_MAX_PPT - 1)
#define FS_LN2 0.6931471805599453

template <int CTL>
__device__ __forceinline__ double fs_dpp(double x)
{
    const int hi = __double2hiint(x), lo = __double2loint(x);
    return __hiloint2double(__builtin_amdgcn_update_dpp(hi, hi, CTL, 0xf, 0xf, false),
                            __builtin_amdgcn_update_dpp(lo, lo, CTL, 0xf, 0xf, false));
}
__device__ __forceinline__ double fs_readlane(double x, int l)
{
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(x), l), __builtin_amdgcn_readlane(__double2loint(x), l));
}
// sum of the wave's 64 values, the same bits in every lane (each step adds two values that both partners hold: a + b == b + a)
__device__ __forceinline__ double fs_wave_sum(double x)
{
    x += fs_dpp<0xB1>(x);                     // quad_perm [1,0,3,2]
    x += fs_dpp<0x4E>(x);                     // quad_perm [2,3,0,1]
    x += fs_dpp<0x141>(x);                    // row_half_mirror
    x += fs_dpp<0x140>(x);                    // row_mirror: every lane holds the sum of its row of 16
    return (fs_readlane(x, 0) + fs_readlane(x, 16)) + (fs_readlane(x, 32) + fs_readlane(x, 48));
}

__device__ __forceinline__ double fs_widen(float v, bool raw, float min_prob, float one_m)
{
    return (double)(raw ? prepare_post_val(v, min_prob, one_m) : v);
}
__device__ __forceinline__ double fs_widen(double v, bool, float, float) { return v; }

struct fs_args {
    const void *post;
    long ld, row_step;
    const int64_t *row_off;
    const int32_t *nrow;
    const int32_t *seq;
    const int64_t *pos_off;
    double *score_out;
    int nstate, blank, full;
    float min_prob, one_m;
};

// rows of emissions in flight per thread: 4 up to four states per thread, then fewer (the ring is PPT * fs_ahead values)
template <int PPT>
struct fs_ahead { static constexpr int value = PPT <= 4 ? 4 : (PPT <= 8 ? 2 : 1); };

template <typename T, int PPT>
__device__ __forceinline__ void fs_pair(const fs_args &a, int b, int L, int nr, double (*wsum)[FS_WAVES], double (*edge)[FS_THREADS],
                                        double *endv)
{
    constexpr int D = fs_ahead<PPT>::value;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int j0 = tid * PPT;
    const bool raw = a.min_prob > 0.0f;
    const int32_t *seq = a.seq + a.pos_off[b];
    const T *rows = static_cast<const T *>(a.post) + (size_t)a.row_off[b] * (size_t)a.ld;
    const size_t rstride = (size_t)a.row_step * (size_t)a.ld;

    // the column of each owned state's emission (state j emits seq[j-1]); -1: no move into this state (j = 0, or past the end)
    int col[PPT];
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
    if (__syncthreads_or(bad ? 1 : 0)) {                      // a symbol that is no column: nothing is read for it, the score is NaN
        if (tid == 0) a.score_out[b] = __longlong_as_double(0x7ff8000000000000LL);
        return;
    }

    T eb[D], ee[D][PPT];
    auto fetch = [&](int slot, int p) {
        const T *r = rows + (size_t)p * rstride;
        eb[slot] = r[a.blank];
#pragma unroll
        for (int k = 0; k < PPT; k++) ee[slot][k] = col[k] >= 0 ? r[col[k]] : (T)0;
    };
#pragma unroll
    for (int d = 0; d < D; d++) {
        if (d < nr) fetch(d, d);
        else {
            eb[d] = (T)0;
#pragma unroll
            for (int k = 0; k < PPT; k++) ee[d][k] = (T)0;
        }
    }

    // decode.py:120-124
    double f[PPT];
    {
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < PPT; k++) {
            const int j = j0 + k;
            f[k] = a.full ? (j == 0 ? 1.0 : 0.0) : (j <= L ? 1.0 : 0.0);
            s += f[k];
        }
        s = fs_wave_sum(s);
        if (lane == 0) wsum[1][wave] = s;
        edge[1][tid] = f[PPT - 1];
    }
    __syncthreads();

    long esum = 0;
    auto row = [&](int p, int slot) {
        const int par = p & 1;
        const double pb = fs_widen(eb[slot], raw, a.min_prob, a.one_m);
        double pe[PPT];
#pragma unroll
        for (int k = 0; k < PPT; k++) pe[k] = col[k] >= 0 ? fs_widen(ee[slot][k], raw, a.min_prob, a.one_m) : 0.0;
        if (p + D < nr) fetch(slot, p + D);
        // the previous row's total, in wave order, and its binary exponent
        const double m = ((wsum[par ^ 1][0] + wsum[par ^ 1][1]) + wsum[par ^ 1][2]) + wsum[par ^ 1][3];
        int e = 0;
        if (m > 0.0 && m < INFINITY) (void)frexp(m, &e);
        esum += e;
        double prev = tid > 0 ? edge[par ^ 1][tid - 1] : 0.0;
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < PPT; k++) {
            const double g = fma(prev, pe[k], f[k] * pb);     // decode.py:131-133
            prev = f[k];
            f[k] = ldexp(g, -e);                              // exact: a power of two
            s += f[k];
        }
        s = fs_wave_sum(s);
        if (lane == 0) wsum[par][wave] = s;
        edge[par][tid] = f[PPT - 1];
        __syncthreads();
    };
    for (int p0 = 0; p0 < nr; p0 += D) {
#pragma unroll
        for (int d = 0; d < D; d++)
            if (p0 + d < nr) row(p0 + d, d);                  // (the same for the whole workgroup)
    }

    if (a.full) {                                             // decode.py:139: the end state's share
#pragma unroll
        for (int k = 0; k < PPT; k++)
            if (j0 + k == L) *endv = f[k];
        __syncthreads();
    }
    if (tid == 0) {
        const int par = (nr - 1) & 1;
        const double m = ((wsum[par][0] + wsum[par][1]) + wsum[par][2]) + wsum[par][3];
        a.score_out[b] = log(a.full ? *endv : m) + (double)esum * FS_LN2;
    }
}

template <typename T, int MAXPPT>
__global__ void __launch_bounds__(FS_THREADS) forward_score_kernel(fs_args a)
{
    __shared__ double wsum[2][FS_WAVES];
    __shared__ double edge[2][FS_THREADS];
    __shared__ double endv;
    const int b = blockIdx.x;
    const int64_t np = a.pos_off[b + 1] - a.pos_off[b];
    const int nr = a.nrow[b];
    if (np < 0 || np >= (int64_t)FS_THREADS * MAXPPT || nr < 0) {       // longer than the caller said (max_npos): refused, NaN
        if (threadIdx.x == 0) a.score_out[b] = __longlong_as_double(0x7ff8000000000000LL);
        return;
    }
    const int L = (int)np;
    if (nr == 0) {                                                      // no rows: the empty sum, and log f[L] of the start vector
        if (threadIdx.x == 0) a.score_out[b] = (a.full && L > 0) ? -INFINITY : 0.0;
        return;
    }
    const int states = L + 1;
    if (states <= FS_THREADS) fs_pair<T, 1>(a, b, L, nr, wsum, edge, &endv);
    else if (states <= 2 * FS_THREADS) fs_pair<T, 2>(a, b, L, nr, wsum, edge, &endv);
    else if constexpr (MAXPPT >= 8) {
        if (states <= 4 * FS_THREADS) fs_pair<T, 4>(a, b, L, nr, wsum, edge, &endv);
        else if (states <= 8 * FS_THREADS) fs_pair<T, 8>(a, b, L, nr, wsum, edge, &endv);
        else if constexpr (MAXPPT >= 32) {
            if (states <= 16 * FS_THREADS) fs_pair<T, 16>(a, b, L, nr, wsum, edge, &endv);
            else fs_pair<T, 32>(a, b, L, nr, wsum, edge, &endv);
        }
    }
}

// One arithmetic, three register budgets: the kernel is picked by the longest sequence of the launch (max_npos), the states per
// thread inside it by the pair alone, so the choice changes the occupancy and never a bit of a score.
template <typename T>
static int fs_launch(const T *post, long ld, const int64_t *row_off, long row_step, const int32_t *nrow, int nstate, const int32_t *seq,
                     const int64_t *pos_off, int nread, int max_npos, int blank, int full, float min_prob, double *score_out,
                     slk_stream_t stream)
{
    if (!post || !row_off || !nrow || !pos_off || !score_out || nread < 1 || nstate < 1 || ld < nstate || row_step < 1 || max_npos < 0 ||
        blank < 0 || blank >= nstate || !(min_prob >= 0.0f) || !(min_prob < 1.0f) || (!seq && max_npos > 0))
        return SLK_ERR_INVALID_ARG;
    if (max_npos > FS_MAX_POSITIONS) return SLK_ERR_UNSUPPORTED;
    fs_args a;
    a.post = post; a.ld = ld; a.row_step = row_step; a.row_off = row_off; a.nrow = nrow; a.seq = seq; a.pos_off = pos_off;
    a.score_out = score_out; a.nstate = nstate; a.blank = blank; a.full = full ? 1 : 0;
    a.min_prob = min_prob; a.one_m = one_minus(min_prob, (double)min_prob);
    hipStream_t s = slk_stream(stream);
    if (max_npos < 2 * FS_THREADS) hipLaunchKernelGGL((forward_score_kernel<T, 2>), dim3(nread), dim3(FS_THREADS), 0, s, a);
    else if (max_npos < 8 * FS_THREADS) hipLaunchKernelGGL((forward_score_kernel<T, 8>), dim3(nread), dim3(FS_THREADS), 0, s, a);
    else hipLaunchKernelGGL((forward_score_kernel<T, 32>), dim3(nread), dim3(FS_THREADS), 0, s, a);
    return slk_launch_status();
}

extern "C" int slk_forward_score_max_positions(void) { return FS_MAX_POSITIONS; }

extern "C" int slk_forward_score_batch_f32(const float *post, long ld, const int64_t *row_off, long row_step, const int32_t *nrow,
                                           int nstate, const int32_t *seq, const int64_t *pos_off, int nread, int max_npos, int blank,
                                           int full, float min_prob, double *score_out, slk_stream_t stream)
{
    return fs_launch<float>(post, ld, row_off, row_step, nrow, nstate, seq, pos_off, nread, max_npos, blank, full, min_prob, score_out,
                            stream);
}

extern "C" int slk_forward_score_batch_f64(const double *post, long ld, const int64_t *row_off, long row_step, const int32_t *nrow,
                                           int nstate, const int32_t *seq, const int64_t *pos_off, int nread, int max_npos, int blank,
                                           int full, double *score_out, slk_stream_t stream)
{
    return fs_launch<double>(post, ld, row_off, row_step, nrow, nstate, seq, pos_off, nread, max_npos, blank, full, 0.0f, score_out,
                             stream);
}
