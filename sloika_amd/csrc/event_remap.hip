// event_remap.hip -- the two device steps `chunkify remap` (sloika/batch.py:143-190) needs beside the network and the remap DP.
//
//   pack + prepare + log    batch.py:146 prepare_post(calc_post(inMat)) and transducer.py:30 np.log(trans), for a ragged batch:
//                           the network-layout posterior [T'][B][S] -> the concatenated log-posterior rows the batched DP reads
//   labels + strand fields  batch.py:69-78 with model_kmer_len == kmer_len (what remap leaves in the table), and
//                           tools/chunkify_with_remap.py:57-58, straight from the DP's paths
//
// Both are HBM-bound.  The first moves 8 bytes per (step, state) instead of the 24 of slice-and-copy, prepare and log as three
// passes; the second is integer work on a few bytes per event.
#include "common.h"
#include "post_transform.h"

// One wave per posterior row: row t of read b -> row ev_off[b] + t of `out`, S floats.  S = 4^k + 1 is odd, so an output row starts
// on any 4-byte boundary: the lanes store a scalar head up to the first 16-byte boundary of the OUTPUT row, then 16 bytes per lane,
// then a scalar tail.  The loads are 16 bytes too where the input row happens to share the output row's alignment (one row in
// four of a dense tensor), four dwords otherwise -- the wave still reads one contiguous span.
__global__ void __launch_bounds__(256) remap_pack_log_post_kernel(const float *__restrict__ post, long row_stride, long batch_stride,
                                                                  int T, int S, const int32_t *__restrict__ nstep,
                                                                  const int64_t *__restrict__ ev_off, float min_prob, float one_m,
                                                                  float *__restrict__ out)
{
    const int b = blockIdx.y;
    const int lane = threadIdx.x & (SLK_WAVE - 1);
    const int t = blockIdx.x * (int)(blockDim.x / SLK_WAVE) + (int)(threadIdx.x / SLK_WAVE);
    const int64_t e0 = ev_off[b];
    int n = nstep[b];                                     // never more rows than the read owns in `out`, nor than the tensor has
    if ((int64_t)n > ev_off[b + 1] - e0) n = (int)(ev_off[b + 1] - e0);
    if (n > T) n = T;
    if (t >= n) return;
    const float *src = post + (size_t)t * row_stride + (size_t)b * batch_stride;
    float *dst = out + (size_t)(e0 + t) * S;
    auto f = [&](float p) { return log_post_val(prepare_post_val(p, min_prob, one_m), SLK_POST_LN, 0.0f, 0.0f); };
    int head = (int)((16 - (reinterpret_cast<uintptr_t>(dst) & 15)) & 15) >> 2;
    if (head > S) head = S;
    if (lane < head) dst[lane] = f(src[lane]);
    const int nvec = (S - head) >> 2;
    const float *s4 = src + head;
    float *d4 = dst + head;
    if ((reinterpret_cast<uintptr_t>(s4) & 15) == 0) {
        for (int i = lane; i < nvec; i += SLK_WAVE) {
            const f32x4 v = *reinterpret_cast<const f32x4 *>(s4 + 4 * i);
            const f32x4 r = {f(v.x), f(v.y), f(v.z), f(v.w)};
            *reinterpret_cast<f32x4 *>(d4 + 4 * i) = r;
        }
    } else {
        for (int i = lane; i < nvec; i += SLK_WAVE) {
            const float *p = s4 + 4 * i;
            const f32x4 r = {f(p[0]), f(p[1]), f(p[2]), f(p[3])};
            *reinterpret_cast<f32x4 *>(d4 + 4 * i) = r;
        }
    }
    const int done = head + 4 * nvec;
    if (lane < S - done) dst[done + lane] = f(src[done + lane]);
}

// One workgroup per read.  Event e of read b sits at position p = path[ev_off[b] + e] of its reference:
//   label = seq[pos_off[b] + p], 0 where the position repeats the previous event's inside a chunk      batch.py:73-78
//   nstay = #{e >= 1 : path[e] == path[e-1]}, min(path), max(path) over ALL events                      chunkify_with_remap.py:57-58
// stats:[B][3] int32.  status bit 1: a path entry outside [0, npos_b) (its label is -1, nothing is read through it); bit 2: a
// read's label rows would leave labels_out (nothing of that read is written).
__global__ void __launch_bounds__(256) event_remap_labels_kernel(const int32_t *__restrict__ path, const int64_t *__restrict__ ev_off,
                                                                 const int32_t *__restrict__ seq, const int64_t *__restrict__ pos_off,
                                                                 int chunk_len, const int64_t *__restrict__ row_off, int64_t total_rows,
                                                                 int32_t *__restrict__ labels, int32_t *__restrict__ stats,
                                                                 int *__restrict__ status)
{
    __shared__ int red[3][4];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & (SLK_WAVE - 1), wave = tid / SLK_WAVE;
    const int64_t e0 = ev_off[b], p0 = pos_off[b], r0 = row_off[b];
    const int64_t nev = ev_off[b + 1] - e0, npos = pos_off[b + 1] - p0;
    const int64_t nlab = (nev / chunk_len) * chunk_len;
    const bool rows_ok = r0 >= 0 && r0 + nlab <= total_rows;
    int nstay = 0, lo = INT32_MAX, hi = INT32_MIN, bits = rows_ok ? 0 : 4;
    for (int64_t e = tid; e < nev; e += blockDim.x) {
        const int p = path[e0 + e];
        const bool stay = e >= 1 && path[e0 + e - 1] == p;
        nstay += stay ? 1 : 0;
        lo = min(lo, p);
        hi = max(hi, p);
        const bool inside = p >= 0 && p < npos;
        if (!inside) bits |= 2;
        if (e < nlab && rows_ok) {
            int lab = inside ? seq[p0 + p] : -1;
            if (stay && e % chunk_len != 0) lab = 0;          // (ediff1d(..., to_begin=1): a chunk's first event keeps its label)
            labels[r0 + e] = lab;
        }
    }
#pragma unroll
    for (int d = SLK_WAVE / 2; d >= 1; d >>= 1) {
        nstay += __shfl_xor(nstay, d);
        lo = min(lo, __shfl_xor(lo, d));
        hi = max(hi, __shfl_xor(hi, d));
        bits |= __shfl_xor(bits, d);
    }
    if (lane == 0) {
        red[0][wave] = nstay;
        red[1][wave] = lo;
        red[2][wave] = hi;
        if (bits) atomicOr(status, bits);
    }
    __syncthreads();
    if (tid == 0) {
        stats[3 * b + 0] = red[0][0] + red[0][1] + red[0][2] + red[0][3];
        stats[3 * b + 1] = min(min(red[1][0], red[1][1]), min(red[1][2], red[1][3]));
        stats[3 * b + 2] = max(max(red[2][0], red[2][1]), max(red[2][2], red[2][3]));
    }
}

extern "C" int slk_remap_pack_log_post_f32(const float *post, long row_stride, long batch_stride, int T, int B, int S,
                                           const int32_t *nstep, const int64_t *ev_off, float min_prob, float *out,
                                           slk_stream_t stream)
{
    if (!post || !nstep || !ev_off || !out || T < 0 || B < 1 || S < 1 || batch_stride < S || row_stride < 0) return SLK_ERR_INVALID_ARG;
    if (B > 65535) return SLK_ERR_UNSUPPORTED;
    if (T == 0) return SLK_OK;
    const int rows_per_block = 256 / SLK_WAVE;
    hipLaunchKernelGGL(remap_pack_log_post_kernel, dim3((unsigned)((T + rows_per_block - 1) / rows_per_block), B), dim3(256), 0,
                       slk_stream(stream), post, row_stride, batch_stride, T, S, nstep, ev_off, min_prob,
                       one_minus(min_prob, (double)min_prob), out);
    return slk_launch_status();
}

extern "C" int slk_event_remap_labels_i32(const int32_t *path, const int64_t *ev_off, const int32_t *seq, const int64_t *pos_off,
                                          int nread, int chunk_len, const int64_t *row_off, int64_t total_rows, int32_t *labels_out,
                                          int32_t *stats_out, int *status, slk_stream_t stream)
{
    if (!path || !ev_off || !seq || !pos_off || !row_off || !labels_out || !stats_out || !status || nread < 1 || chunk_len < 1 ||
        total_rows < 0)
        return SLK_ERR_INVALID_ARG;
    hipLaunchKernelGGL(event_remap_labels_kernel, dim3(nread), dim3(256), 0, slk_stream(stream), path, ev_off, seq, pos_off, chunk_len,
                       row_off, total_rows, labels_out, stats_out, status);
    return slk_launch_status();
}
