// event_features.hip -- the event front end (sloika/features.py:6-32 with sloika/maths.py:48-58) on gfx950.
//
//   from_events      features.py:16-25    rows [mean, stdv, length, |mean[e+1] - mean[e]|], the last row's delta 0
//   studentise       maths.py:55-58       (x - mean) / std per column, population std, a std that is not > 0 replaced by 1
//   nanonet          features.py:27-30    fourth column = signed delta over ITS standard deviation (uncentred)
//
// A ragged set of segments in one launch: a segment is a whole read (features.from_events, batch.chunkify 'none' / 'per-read',
// basecall.events_worker) or one chunk's window of a read (batch.chunkify 'per-chunk', batch.py:37-49: chunk_len + 1 events where the
// read has one more, chunk_len rows kept).  One workgroup of 256 lanes per segment, three passes over the segment's events: column
// sums, sums of squared deviations, output.  The feature VALUES are the float32 numbers the reference stores into its float32 matrix
// before it studentises (features.py:17-22); their moments are accumulated in float64 in a fixed order (lane-strided partial sums, a
// shuffle tree, four wave partials added in order), so a segment gets the same bits whatever else shares the launch, and the
// result is rounded to float32 once.  12-24 B in and 16 B out per event: nothing here is worth tuning.
#include "common.h"

#define EVF_THREADS 256

struct EvfSums {
    double c[4];
};

// Sum over the workgroup, the same value in every lane; `part` holds one EvfSums per wave.
__device__ __forceinline__ EvfSums evf_block_sum(EvfSums v, EvfSums *part)
{
#pragma unroll
    for (int k = 0; k < 4; k++)
#pragma unroll
        for (int off = SLK_WAVE / 2; off > 0; off >>= 1) v.c[k] += __shfl_down(v.c[k], off, SLK_WAVE);
    const int wave = threadIdx.x / SLK_WAVE;
    __syncthreads();                                     // (the previous round's readers are done with `part`)
    if ((threadIdx.x & (SLK_WAVE - 1)) == 0) part[wave] = v;
    __syncthreads();
    EvfSums r = part[0];
#pragma unroll
    for (int w = 1; w < EVF_THREADS / SLK_WAVE; w++)
#pragma unroll
        for (int k = 0; k < 4; k++) r.c[k] += part[w].c[k];
    return r;
}

// The four float32 features of event e (segment-local index i of n) as the reference stores them, as doubles.  SIGNED: the fourth is
// the signed delta (features.py:29), otherwise its magnitude (features.py:22).  The difference is taken in the table's own precision
// and rounded to float32 once, like numpy's ediff1d followed by the store into the float32 matrix.
template <typename T, bool SIGNED>
__device__ __forceinline__ EvfSums evf_row(const T *__restrict__ mean, const T *__restrict__ stdv, const T *__restrict__ length,
                                           long long e, long long i, long long n)
{
    EvfSums x;
    const T m = mean[e];
    x.c[0] = (double)(float)m;
    x.c[1] = (double)(float)stdv[e];
    x.c[2] = (double)(float)length[e];
    T d = (T)0;
    if (i + 1 < n) d = mean[e + 1] - m;
    if (!SIGNED) d = d < (T)0 ? -d : d;
    x.c[3] = (double)(float)d;
    return x;
}

template <typename T, bool NANONET>
__global__ void __launch_bounds__(EVF_THREADS) event_features_kernel(const T *__restrict__ mean, const T *__restrict__ stdv,
                                                                     const T *__restrict__ length,
                                                                     const long long *__restrict__ seg_start,
                                                                     const long long *__restrict__ seg_len,
                                                                     const long long *__restrict__ seg_keep, int normalise,
                                                                     float *__restrict__ out, const long long *__restrict__ out_row,
                                                                     long long ld_out)
{
    __shared__ EvfSums part[EVF_THREADS / SLK_WAVE];
    const long long s = blockIdx.x;
    const long long e0 = seg_start[s], n = seg_len[s];
    const long long keep = min(seg_keep[s], n);
    if (n < 1 || keep < 1) return;                       // (uniform over the workgroup)
    float *dst = out + 4 * out_row[s];

    EvfSums mu = {{0.0, 0.0, 0.0, 0.0}}, sd = {{1.0, 1.0, 1.0, 1.0}};
    if (normalise || NANONET) {
        EvfSums acc = {{0.0, 0.0, 0.0, 0.0}};
        for (long long i = threadIdx.x; i < n; i += EVF_THREADS) {
            const EvfSums x = evf_row<T, NANONET>(mean, stdv, length, e0 + i, i, n);
#pragma unroll
            for (int k = 0; k < 4; k++) acc.c[k] += x.c[k];
        }
        mu = evf_block_sum(acc, part);
#pragma unroll
        for (int k = 0; k < 4; k++) mu.c[k] /= (double)n;
        acc = {{0.0, 0.0, 0.0, 0.0}};
        for (long long i = threadIdx.x; i < n; i += EVF_THREADS) {
            const EvfSums x = evf_row<T, NANONET>(mean, stdv, length, e0 + i, i, n);
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const double dv = x.c[k] - mu.c[k];
                acc.c[k] += dv * dv;
            }
        }
        sd = evf_block_sum(acc, part);
#pragma unroll
        for (int k = 0; k < 4; k++) {
            sd.c[k] = sqrt(sd.c[k] / (double)n);
            // maths.py:57; the nanonet column divides by its deviation as it is (features.py:30)
            if (!(NANONET && k == 3) && !(sd.c[k] > 0.0)) sd.c[k] = 1.0;
        }
        if (NANONET) mu.c[3] = 0.0;                      // uncentred
        if (!normalise)
#pragma unroll
            for (int k = 0; k < 3; k++) {
                mu.c[k] = 0.0;
                sd.c[k] = 1.0;
            }
    }
    for (long long i = threadIdx.x; i < keep; i += EVF_THREADS) {
        const EvfSums x = evf_row<T, NANONET>(mean, stdv, length, e0 + i, i, n);
        f32x4 y;
        y.x = (float)((x.c[0] - mu.c[0]) / sd.c[0]);
        y.y = (float)((x.c[1] - mu.c[1]) / sd.c[1]);
        y.z = (float)((x.c[2] - mu.c[2]) / sd.c[2]);
        y.w = (float)((x.c[3] - mu.c[3]) / sd.c[3]);
        *reinterpret_cast<f32x4 *>(dst + i * ld_out) = y;
    }
}

extern "C" int slk_event_features_f32(const void *mean, const void *stdv, const void *length, int columns_f64,
                                      const int64_t *seg_start, const int64_t *seg_len, const int64_t *seg_keep, int64_t nseg,
                                      int normalise, int nanonet, float *out, const int64_t *out_row, int64_t ld_out,
                                      slk_stream_t stream)
{
    if (!mean || !stdv || !length || !seg_start || !seg_len || !seg_keep || !out || !out_row || nseg < 0 || ld_out < 4 ||
        (ld_out & 3) || (reinterpret_cast<uintptr_t>(out) & 15))
        return SLK_ERR_INVALID_ARG;
    if (nseg == 0) return SLK_OK;
    if (nseg > 0x7fffffffLL) return SLK_ERR_UNSUPPORTED;
    const dim3 grid((unsigned)nseg), block(EVF_THREADS);
    const long long *ss = reinterpret_cast<const long long *>(seg_start), *sl = reinterpret_cast<const long long *>(seg_len),
                    *sk = reinterpret_cast<const long long *>(seg_keep), *orow = reinterpret_cast<const long long *>(out_row);
#define EVF_LAUNCH(T, NN)                                                                                                       \
    hipLaunchKernelGGL((event_features_kernel<T, NN>), grid, block, 0, slk_stream(stream), static_cast<const T *>(mean),        \
                       static_cast<const T *>(stdv), static_cast<const T *>(length), ss, sl, sk, normalise ? 1 : 0, out, orow,  \
                       (long long)ld_out)
    if (columns_f64) {
        if (nanonet) EVF_LAUNCH(double, true);
        else EVF_LAUNCH(double, false);
    } else {
        if (nanonet) EVF_LAUNCH(float, true);
        else EVF_LAUNCH(float, false);
    }
#undef EVF_LAUNCH
    return slk_launch_status();
}
