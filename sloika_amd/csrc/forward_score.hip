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
#include "forward_row.h"

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
    if (states <= FS_THREADS) fs_pair<T, 1>(a, b, L, nr, wsum, edge, &endv, fs_keep_none());
    else if (states <= 2 * FS_THREADS) fs_pair<T, 2>(a, b, L, nr, wsum, edge, &endv, fs_keep_none());
    else if constexpr (MAXPPT >= 8) {
        if (states <= 4 * FS_THREADS) fs_pair<T, 4>(a, b, L, nr, wsum, edge, &endv, fs_keep_none());
        else if (states <= 8 * FS_THREADS) fs_pair<T, 8>(a, b, L, nr, wsum, edge, &endv, fs_keep_none());
        else if constexpr (MAXPPT >= 32) {
            if (states <= 16 * FS_THREADS) fs_pair<T, 16>(a, b, L, nr, wsum, edge, &endv, fs_keep_none());
            else fs_pair<T, 32>(a, b, L, nr, wsum, edge, &endv, fs_keep_none());
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
