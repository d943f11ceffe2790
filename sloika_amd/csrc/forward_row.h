// forward_row.h -- the row step of the forward (sum-product) recursion: the register ownership, the fixed-order reductions, the
// power-of-two scaling and the emission ring of forward_score.hip (whose head comment describes them), shared with
// forward_backward.hip so that its first pass gives the bits of the forward score by construction.
#pragma once
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

// no row is kept: the forward score
struct fs_keep_none {
    template <int PPT>
    __device__ __forceinline__ void operator()(int, const double (&)[PPT]) const {}
};

// -> false when the pair was refused (NaN).  keep(p, f) sees the scaled state in front of every row p, off the chain.
template <typename T, int PPT, typename Keep>
__device__ __forceinline__ bool fs_pair(const fs_args &a, int b, int L, int nr, double (*wsum)[FS_WAVES], double (*edge)[FS_THREADS],
                                        double *endv, const Keep &keep)
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
        return false;
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
        keep(p, f);
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
    return true;
}
