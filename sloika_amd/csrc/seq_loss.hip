// seq_loss.hip -- the sequence loss of a training step: d loss / d logits from the occupancies of forward-backward
// (csrc/forward_backward.hip, design/forward_backward.md section 6; design/sequence_loss.md).
//
// With ll_b the forward score of chunk b under post = min_prob + (1 - min_prob) softmax(x) and loss = -sum_b c_b ll_b,
//     p_k = exp(x_k - max) * inv_sum ; p'_k = min_prob + (1 - min_prob) p_k ; w_k = occ_k (1 - min_prob) p_k / p'_k ; W = sum_k w_k
//     d loss / d x_k = -c_b (w_k - p_k W)
// per row m = t*B + b, in place over the logits.  Where occ_k is 0 so is w_k, whatever p'_k (no 0/0 at min_prob = 0 when p
// underflows).  A chunk whose score is not finite (NaN: refused by forward-backward, which then wrote nothing of its occ; -inf: no
// alignment exists) gets rows of exact zeros by a branch that never reads its occ.
//
// One wave per row, four rows per workgroup, like softmax_xent_grad_kernel (csrc/train.hip).  Lane l owns the column groups
// 4 (l + 64 k) .. + 3, k = 0, 1, ..: a 16-byte access where the row pitch and the base allow it, four dword accesses of the same
// columns otherwise -- so which columns a lane sums, and in which order, does not depend on the alignment.  W: every lane adds its
// w_k in ascending column order starting from 0, then the xor butterfly 32, 16, .. 1 of the row kernels of csrc/train.hip; a row has
// one wave, so there are no wave totals to add.  A row's bits depend on that row, score[b] and chunk_scale[b] alone.
//
// Rows of up to 2048 floats (the 1025 states of a 5-mer model at ld = 1056 among them) are held in registers: logits and occ are
// each read once and the logits written once, all loads of a row in flight before the first store.  Wider rows take two passes
// (W, then the gradient: the logits and occ are read twice).
#include "common.h"
#include "post_transform.h"

namespace {

struct SeqGradArgs {
    float *logits; long ld;
    const float *stats;
    const float *occ; long occ_ld;
    const double *score; const float *chunk_scale;
    size_t M; int B, nstate;
    float min_prob, one_m;
    int lvec, ovec;                       // 16-byte accesses of the logits / of occ
};

// columns 4 j4 .. 4 j4 + 3 of a row of `width` floats.  vec: one 16-byte load at a clamped index (the loads stay back to back);
// what a clamped index or a column >= width brings is never used: the caller masks by the true column index.
__device__ __forceinline__ float4 load4(const float *row, int vec, int j4, int width)
{
    if (vec) return reinterpret_cast<const float4 *>(row)[min(j4, (width >> 2) - 1)];
    const int j = 4 * j4;
    return make_float4(j < width ? row[j] : 0.0f, j + 1 < width ? row[j + 1] : 0.0f, j + 2 < width ? row[j + 2] : 0.0f,
                       j + 3 < width ? row[j + 3] : 0.0f);
}

__device__ __forceinline__ void store4(float *row, int vec, int j4, int width, float4 v)
{
    const int j = 4 * j4;
    if (vec) {
        if (j < width) reinterpret_cast<float4 *>(row)[j4] = v;         // (width is a multiple of 4 here)
        return;
    }
    if (j < width) row[j] = v.x;
    if (j + 1 < width) row[j + 1] = v.y;
    if (j + 2 < width) row[j + 2] = v.z;
    if (j + 3 < width) row[j + 3] = v.w;
}

// x (a logit) -> p, o (an occupancy) -> w, both 0 for a column outside the states
__device__ __forceinline__ void seq_term(float &x, float &o, bool in, float mx, float inv, float min_prob, float one_m)
{
    const float p = in ? __expf(x - mx) * inv : 0.0f;
    const float pp = prepare_post_val(p, min_prob, one_m);
    const float w = (in && o != 0.0f) ? o * ((one_m * p) / pp) : 0.0f;
    x = p;
    o = w;
}

__device__ __forceinline__ void seq_terms(float4 &x, float4 &o, int j4, const SeqGradArgs &a, float mx, float inv, float &acc)
{
    const int j = 4 * j4;
    seq_term(x.x, o.x, j < a.nstate, mx, inv, a.min_prob, a.one_m);
    seq_term(x.y, o.y, j + 1 < a.nstate, mx, inv, a.min_prob, a.one_m);
    seq_term(x.z, o.z, j + 2 < a.nstate, mx, inv, a.min_prob, a.one_m);
    seq_term(x.w, o.w, j + 3 < a.nstate, mx, inv, a.min_prob, a.one_m);
    acc += o.x;
    acc += o.y;
    acc += o.z;
    acc += o.w;
}

__device__ __forceinline__ float4 seq_grad4(float4 p, float4 w, float W, float c)
{
    // (columns outside the states hold p = w = 0: -c * 0 would be -0, they are to be +0)
    const float4 g = make_float4(-c * (w.x - p.x * W), -c * (w.y - p.y * W), -c * (w.z - p.z * W), -c * (w.w - p.w * W));
    return make_float4(g.x + 0.0f, g.y + 0.0f, g.z + 0.0f, g.w + 0.0f);
}

__device__ __forceinline__ float wave_total(float v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// NV > 0: the row's column groups fit in NV per lane and stay in registers; NV == 0: any width, two passes
template <int NV>
__global__ void __launch_bounds__(256) softmax_seq_grad_kernel(const SeqGradArgs a)
{
    const int lane = threadIdx.x & 63;
    const size_t m = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (m >= a.M) return;
    const int b = (int)(m % (size_t)a.B);
    const int ld = (int)a.ld, occ_ld = (int)a.occ_ld;
    float *row = a.logits + m * (size_t)a.ld;
    const float *orow = a.occ + m * (size_t)a.occ_ld;
    const int n4 = (ld + 3) >> 2;
    const double sc = a.score[b];
    if (!(sc - sc == 0.0)) {                               // NaN or +-inf: zeros, and this chunk's occ is not read
        for (int j4 = lane; j4 < n4; j4 += 64) store4(row, a.lvec, j4, ld, make_float4(0.0f, 0.0f, 0.0f, 0.0f));
        return;
    }
    const float mx = a.stats[2 * m], inv = a.stats[2 * m + 1];
    const float c = a.chunk_scale[b];
    float acc = 0.0f;
    if (NV > 0) {
        float4 x[NV > 0 ? NV : 1], o[NV > 0 ? NV : 1];
#pragma unroll
        for (int k = 0; k < NV; k++) x[k] = load4(row, a.lvec, lane + 64 * k, ld);
#pragma unroll
        for (int k = 0; k < NV; k++) o[k] = load4(orow, a.ovec, lane + 64 * k, occ_ld);
#pragma unroll
        for (int k = 0; k < NV; k++) seq_terms(x[k], o[k], lane + 64 * k, a, mx, inv, acc);
        const float W = wave_total(acc);
#pragma unroll
        for (int k = 0; k < NV; k++)
            if (lane + 64 * k < n4) store4(row, a.lvec, lane + 64 * k, ld, seq_grad4(x[k], o[k], W, c));
    } else {
        for (int j4 = lane; j4 < n4; j4 += 64) {
            float4 x = load4(row, a.lvec, j4, ld), o = load4(orow, a.ovec, j4, occ_ld);
            seq_terms(x, o, j4, a, mx, inv, acc);
        }
        const float W = wave_total(acc);
        for (int j4 = lane; j4 < n4; j4 += 64) {
            float4 x = load4(row, a.lvec, j4, ld), o = load4(orow, a.ovec, j4, occ_ld);
            float unused = 0.0f;
            seq_terms(x, o, j4, a, mx, inv, unused);
            store4(row, a.lvec, j4, ld, seq_grad4(x, o, W, c));
        }
    }
}

}  // namespace

extern "C" int slk_softmax_seq_grad_f32(float *logits, long ld, const float *stats, const float *occ, long occ_ld, const double *score,
                                        const float *chunk_scale, int T, int B, int nstate, float min_prob, slk_stream_t stream)
{
    if (!logits || !stats || !occ || !score || !chunk_scale || T < 1 || B < 1 || nstate < 2 || ld < nstate || occ_ld < nstate ||
        !(min_prob >= 0.0f && min_prob < 1.0f))
        return SLK_ERR_INVALID_ARG;
    const size_t M = (size_t)T * B;
    if (ld > SLK_SEQ_GRAD_MAX_LD || occ_ld > SLK_SEQ_GRAD_MAX_LD || (M + 3) / 4 > 0x7fffffffUL) return SLK_ERR_UNSUPPORTED;
    SeqGradArgs a;
    a.logits = logits; a.ld = ld; a.stats = stats; a.occ = occ; a.occ_ld = occ_ld; a.score = score; a.chunk_scale = chunk_scale;
    a.M = M; a.B = B; a.nstate = nstate;
    a.min_prob = min_prob; a.one_m = one_minus(min_prob, (double)min_prob);
    a.lvec = (ld & 3) == 0 && (reinterpret_cast<uintptr_t>(logits) & 15) == 0;
    a.ovec = (occ_ld & 3) == 0 && (reinterpret_cast<uintptr_t>(occ) & 15) == 0;
    const dim3 grid((unsigned)((M + 3) / 4)), block(256);
    hipStream_t s = slk_stream(stream);
    const long groups = (ld + 3) / 4;
    if (groups <= 64 * 2) hipLaunchKernelGGL(softmax_seq_grad_kernel<2>, grid, block, 0, s, a);
    else if (groups <= 64 * 5) hipLaunchKernelGGL(softmax_seq_grad_kernel<5>, grid, block, 0, s, a);
    else if (groups <= 64 * 8) hipLaunchKernelGGL(softmax_seq_grad_kernel<8>, grid, block, 0, s, a);
    else hipLaunchKernelGGL(softmax_seq_grad_kernel<0>, grid, block, 0, s, a);
    return slk_launch_status();
}
