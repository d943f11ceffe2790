// forward_backward.hip -- forward-backward over the recursion of decode.forwards (sloika/decode.py:108-139) on gfx950: for a ragged
// batch of (posterior, sequence) pairs, with what probability each row emits each symbol, summed over all alignments.
//
//     f_0 = 1 (full: e_0)      f_t[j]   = f_{t-1}[j] p_t[blank] + f_{t-1}[j-1] p_t[seq[j-1]]          (forward_row.h)
//     b_T = 1 (full: e_L)      b_{t-1}[j] = b_t[j] p_t[blank] + b_t[j+1] p_t[seq[j]]
//     stay_t[j] = f_{t-1}[j] p_t[blank] b_t[j]      move_t[j] = f_{t-1}[j-1] p_t[seq[j-1]] b_t[j]      z_t = sum stay + sum move
//     occ[t, blank] += sum_j stay_t[j] / z_t        occ[t, seq[j-1]] += move_t[j] / z_t
//     emit_prob[j-1] = max_t move_t[j] / z_t        emit_row[j-1] = the lowest t that attains it
//
// One workgroup of 256 threads per pair and the ownership of forward_score.hip: thread i holds the ppt consecutive states from i * ppt
// in registers, ppt chosen by the pair alone, the register budget by the launch's longest sequence (design/forward_backward.md).
//
// Pass 1 is fs_pair, the row step of the forward score, so the score has that entry's bits; in front of every row it stores the
// scaled state as float64 into the pair's slice of the workspace (256 * ppt doubles per row), off the chain.
//
// Pass 2 walks the rows downwards with b in registers.  b is scaled like f, by the exact power of two of the previous row's total;
// the right neighbour's first state comes through LDS behind the row's one barrier.  f_{t-1} (own states and the left neighbour's
// last) and the emissions are fetched fs_ahead rows ahead.  Because a row is divided by its own z_t no scaling enters the result.
// The three sums of a row (b, stay, move) are reduced like the forward total: per thread ascending, fs_wave_sum, waves as
// ((w0 + w1) + w2) + w3.  They are read behind the row's barrier, so a row's terms are finished one iteration later and leave one
// iteration after that:
//     iteration p:   row p + 2 leaves its table  |  row p + 1: terms / z, added into its table, emit_* updated  |  row p: the chain
// A term is a fixed-point number, round(q * 2^62), added into the 64-bit slot of its column with an integer LDS atomic: integer
// addition commutes, so positions that share a symbol add up to the same bits in any order.  The stay sum goes the same way into the
// blank's slot.  Every thread that added something swaps its slot for 0: exactly one of them gets the column's sum, and stores it;
// the others get 0, and the slot is clean for the row after next.  Two tables on the row's parity keep all of this off the chain.
// occ is zero-filled by a kernel of its own in front (the rows and columns of accepted pairs only); a row whose z_t is 0 or not finite
// adds nothing.
#include <vector>

#include "forward_row.h"

#define FB_MAX_STATES 8192
#define FB_ONE 4611686018427387904.0                          // 2^62
#define FB_ZERO_SPLIT 32

struct fb_args {
    fs_args f;
    void *occ;
    long occ_ld;
    int32_t *emit_row;
    double *emit_prob;
    double *ws;                                               // the workspace; ws_off[b]: where pair b's rows begin, in doubles
    const int64_t *ws_off;
};

__host__ __device__ static inline int fb_ppt(int states)
{
    int ppt = 1;
    while (FS_THREADS * ppt < states) ppt *= 2;
    return ppt;
}

// the scaled state in front of every row, PPT consecutive doubles per thread
struct fb_keep_rows {
    double *base;
    template <int PPT>
    __device__ __forceinline__ void operator()(int p, const double (&f)[PPT]) const
    {
        double *w = base + (size_t)p * (FS_THREADS * PPT);
        if constexpr (PPT == 1) w[0] = f[0];
        else {
#pragma unroll
            for (int k = 0; k < PPT; k += 2) *reinterpret_cast<double2 *>(w + k) = make_double2(f[k], f[k + 1]);
        }
    }
};

__device__ __forceinline__ double fb_sum4(const double *w) { return ((w[0] + w[1]) + w[2]) + w[3]; }

template <typename T, typename O, int PPT>
__device__ __forceinline__ void fb_pair(const fb_args &A, int b, int L, int nr, double (*wsum)[FS_WAVES], double (*edge)[FS_THREADS],
                                        double *endv, double (*bsum)[3][FS_WAVES], unsigned long long *table)
{
    const fs_args &a = A.f;
    constexpr int D = fs_ahead<PPT>::value;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int j0 = tid * PPT;
    double *wsrows = A.ws + A.ws_off[b];

    if (!fs_pair<T, PPT>(a, b, L, nr, wsum, edge, endv, fb_keep_rows{wsrows + j0})) return;
    __syncthreads();                                          // every row of f is stored; edge is free again

    const bool raw = a.min_prob > 0.0f;
    const int32_t *seq = a.seq + a.pos_off[b];
    const T *rows = static_cast<const T *>(a.post) + (size_t)a.row_off[b] * (size_t)a.ld;
    const size_t rstride = (size_t)a.row_step * (size_t)a.ld;
    O *occ = A.occ ? static_cast<O *>(A.occ) + (size_t)a.row_off[b] * (size_t)A.occ_ld : nullptr;
    const size_t ostride = (size_t)a.row_step * (size_t)A.occ_ld;

    // col[k]: the emission of the move into state j0 + k (pass 1 has checked them); col[PPT]: into the right neighbour's first state
    int col[PPT + 1];
#pragma unroll
    for (int k = 0; k <= PPT; k++) {
        const int j = j0 + k;
        col[k] = (j >= 1 && j <= L) ? seq[j - 1] : -1;
    }

    T eb[D], ee[D][PPT + 1];
    double fr[D][PPT + 1];                                    // f in front of the row: [0] state j0 - 1, [k + 1] state j0 + k
    auto fetch = [&](int slot, int p) {
        const T *r = rows + (size_t)p * rstride;
        eb[slot] = r[a.blank];
#pragma unroll
        for (int k = 0; k <= PPT; k++) ee[slot][k] = col[k] >= 0 ? r[col[k]] : (T)0;
        const double *w = wsrows + (size_t)p * (FS_THREADS * PPT) + j0;
        fr[slot][0] = tid > 0 ? w[-1] : 0.0;
#pragma unroll
        for (int k = 0; k < PPT; k++) fr[slot][k + 1] = w[k];
    };
#pragma unroll
    for (int d = 0; d < D; d++) {
        if (d < nr) fetch(d, nr - 1 - d);
        else {
            eb[d] = (T)0;
#pragma unroll
            for (int k = 0; k <= PPT; k++) { ee[d][k] = (T)0; fr[d][k] = 0.0; }
        }
    }

    double bb[PPT], mv[PPT], ep[PPT];
    int er[PPT];
    unsigned added = 0;                                       // bit k: this thread added into col[k]'s slot
    bool added_blank = false;                                 // (thread 0) ... into the blank's
    {
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < PPT; k++) {
            const int j = j0 + k;
            bb[k] = a.full ? (j == L ? 1.0 : 0.0) : (j <= L ? 1.0 : 0.0);
            mv[k] = 0.0;
            ep[k] = 0.0;
            er[k] = -1;
            s += bb[k];
        }
        s = fs_wave_sum(s);
        if (lane == 0) bsum[nr & 1][0][wave] = s;
        edge[nr & 1][tid] = bb[0];
    }
    __syncthreads();

    // row r leaves its table
    auto leave = [&](int r) {
        if (!occ) return;
        unsigned long long *tb = table + (size_t)(r & 1) * a.nstate;
        O *orow = occ + (size_t)r * ostride;
#pragma unroll
        for (int k = 0; k < PPT; k++)
            if (added & (1u << k)) {
                const unsigned long long v = atomicExch(&tb[col[k]], 0ULL);
                if (v) orow[col[k]] = (O)((double)v * (1.0 / FB_ONE));
            }
        if (added_blank) {
            const unsigned long long v = atomicExch(&tb[a.blank], 0ULL);
            if (v) orow[a.blank] = (O)((double)v * (1.0 / FB_ONE));
        }
    };
    // row r's terms, now that its sums are behind a barrier
    auto terms = [&](int r) {
        const int par = r & 1;
        const double zs = fb_sum4(bsum[par][1]), z = zs + fb_sum4(bsum[par][2]);
        added = 0;
        added_blank = false;
        if (!(z > 0.0 && z < INFINITY)) return;
        unsigned long long *tb = table + (size_t)par * a.nstate;
#pragma unroll
        for (int k = 0; k < PPT; k++) {
            if (col[k] < 0) continue;
            const double q = mv[k] / z;
            if (!(q > 0.0)) continue;
            if (q >= ep[k]) { ep[k] = q; er[k] = r; }         // descending rows: the lowest row wins a tie
            if (occ) {
                const unsigned long long v = __double2ull_rn(q * FB_ONE);
                if (v) { atomicAdd(&tb[col[k]], v); added |= 1u << k; }
            }
        }
        if (tid == 0 && occ) {
            const unsigned long long v = __double2ull_rn((zs / z) * FB_ONE);
            if (v) { atomicAdd(&tb[a.blank], v); added_blank = true; }
        }
    };
    // row p's chain: b in front of the row from b behind it, and the row's stay and move
    auto row = [&](int p, int slot) {
        const int par = p & 1;
        const double pb = fs_widen(eb[slot], raw, a.min_prob, a.one_m);
        double pe[PPT + 1], fl[PPT + 1];
#pragma unroll
        for (int k = 0; k <= PPT; k++) {
            pe[k] = col[k] >= 0 ? fs_widen(ee[slot][k], raw, a.min_prob, a.one_m) : 0.0;
            fl[k] = fr[slot][k];
        }
        if (p - D >= 0) fetch(slot, p - D);
        const double m = fb_sum4(bsum[par ^ 1][0]);
        int e = 0;
        if (m > 0.0 && m < INFINITY) (void)frexp(m, &e);
        const double right = tid < FS_THREADS - 1 ? edge[par ^ 1][tid + 1] : 0.0;
        double ss = 0.0, sm = 0.0, sb = 0.0;
#pragma unroll
        for (int k = 0; k < PPT; k++) {
            ss += (fl[k + 1] * pb) * bb[k];
            mv[k] = (fl[k] * pe[k]) * bb[k];
            sm += mv[k];
            const double nb = k + 1 < PPT ? bb[(k + 1) % PPT] : right;
            const double g = fma(nb, pe[k + 1], bb[k] * pb);
            bb[k] = ldexp(g, -e);                             // exact: a power of two
            sb += bb[k];
        }
        sb = fs_wave_sum(sb);
        ss = fs_wave_sum(ss);
        sm = fs_wave_sum(sm);
        if (lane == 0) { bsum[par][0][wave] = sb; bsum[par][1][wave] = ss; bsum[par][2][wave] = sm; }
        edge[par][tid] = bb[0];
    };
    for (int i0 = 0; i0 < nr; i0 += D) {
#pragma unroll
        for (int d = 0; d < D; d++)
            if (i0 + d < nr) {                                // (the same for the whole workgroup)
                const int p = nr - 1 - (i0 + d);
                if (p + 2 < nr) leave(p + 2);
                if (p + 1 < nr) terms(p + 1);
                row(p, d);
                __syncthreads();
            }
    }
    if (nr > 1) leave(1);
    terms(0);
    __syncthreads();
    leave(0);

#pragma unroll
    for (int k = 0; k < PPT; k++)
        if (col[k] >= 0) {
            if (A.emit_row) A.emit_row[a.pos_off[b] + j0 + k - 1] = er[k];
            if (A.emit_prob) A.emit_prob[a.pos_off[b] + j0 + k - 1] = ep[k];
        }
}

// which pairs the device refuses by their lengths (the symbols are checked where they are read)
__device__ __forceinline__ bool fb_refused(const fs_args &a, int b, int maxppt)
{
    const int64_t np = a.pos_off[b + 1] - a.pos_off[b];
    return np < 0 || np >= (int64_t)FS_THREADS * maxppt || a.nrow[b] < 0;
}

template <typename T, typename O, int MAXPPT>
__global__ void __launch_bounds__(FS_THREADS) forward_backward_kernel(fb_args A)
{
    extern __shared__ unsigned long long fb_table[];          // [2][nstate]
    __shared__ double wsum[2][FS_WAVES];
    __shared__ double edge[2][FS_THREADS];
    __shared__ double bsum[2][3][FS_WAVES];
    __shared__ double endv;
    const fs_args &a = A.f;
    const int b = blockIdx.x;
    if (fb_refused(a, b, MAXPPT)) {                           // longer than the caller said (max_npos): NaN, nothing else is written
        if (threadIdx.x == 0) a.score_out[b] = __longlong_as_double(0x7ff8000000000000LL);
        return;
    }
    const int L = (int)(a.pos_off[b + 1] - a.pos_off[b]);
    const int nr = a.nrow[b];
    if (nr == 0) {                                            // no rows: the forward score's value, and no position was ever emitted
        if (threadIdx.x == 0) a.score_out[b] = (a.full && L > 0) ? -INFINITY : 0.0;
        for (int j = threadIdx.x; j < L; j += FS_THREADS) {
            if (A.emit_row) A.emit_row[a.pos_off[b] + j] = -1;
            if (A.emit_prob) A.emit_prob[a.pos_off[b] + j] = 0.0;
        }
        return;
    }
    for (int c = threadIdx.x; c < 2 * a.nstate; c += FS_THREADS) fb_table[c] = 0ULL;      // (pass 1's barriers stand behind this)
    const int states = L + 1;
    if (states <= FS_THREADS) fb_pair<T, O, 1>(A, b, L, nr, wsum, edge, &endv, bsum, fb_table);
    else if (states <= 2 * FS_THREADS) fb_pair<T, O, 2>(A, b, L, nr, wsum, edge, &endv, bsum, fb_table);
    else if constexpr (MAXPPT >= 8) {
        if (states <= 4 * FS_THREADS) fb_pair<T, O, 4>(A, b, L, nr, wsum, edge, &endv, bsum, fb_table);
        else if (states <= 8 * FS_THREADS) fb_pair<T, O, 8>(A, b, L, nr, wsum, edge, &endv, bsum, fb_table);
        else if constexpr (MAXPPT >= 32) {
            if (states <= 16 * FS_THREADS) fb_pair<T, O, 16>(A, b, L, nr, wsum, edge, &endv, bsum, fb_table);
            else fb_pair<T, O, 32>(A, b, L, nr, wsum, edge, &endv, bsum, fb_table);
        }
    }
}

// zero-fill of the occ rows of every pair the main kernel accepts: rows 0 .. nrow - 1, columns 0 .. nstate - 1, nothing else
template <typename O>
__global__ void __launch_bounds__(FS_THREADS) forward_backward_zero_kernel(fb_args A, int maxppt)
{
    const fs_args &a = A.f;
    const int b = blockIdx.x;
    if (fb_refused(a, b, maxppt)) return;
    const int L = (int)(a.pos_off[b + 1] - a.pos_off[b]);
    const int nr = a.nrow[b];
    const int32_t *seq = a.seq + a.pos_off[b];
    bool bad = false;
    for (int j = threadIdx.x; j < L; j += FS_THREADS) bad |= seq[j] < 0 || seq[j] >= a.nstate;
    if (__syncthreads_or(bad ? 1 : 0)) return;
    O *occ = static_cast<O *>(A.occ) + (size_t)a.row_off[b] * (size_t)A.occ_ld;
    const size_t ostride = (size_t)a.row_step * (size_t)A.occ_ld;
    for (int r = blockIdx.y; r < nr; r += gridDim.y)
        for (int c = threadIdx.x; c < a.nstate; c += FS_THREADS) occ[(size_t)r * ostride + c] = (O)0;
}

static inline size_t fb_round256(size_t n) { return (n + 255) & ~(size_t)255; }

// doubles of workspace of one pair (host values): nothing for a pair the device refuses or that has no rows
static inline size_t fb_pair_doubles(int64_t np, int nr)
{
    if (np < 0 || np > FS_MAX_POSITIONS || nr <= 0) return 0;
    return (size_t)nr * FS_THREADS * fb_ppt((int)np + 1);
}

extern "C" size_t slk_forward_backward_workspace_bytes(int nread, const int32_t *nrow, const int64_t *pos_off)
{
    if (nread < 1 || !nrow || !pos_off) return 0;
    size_t n = fb_round256((size_t)(nread + 1) * sizeof(int64_t));
    for (int b = 0; b < nread; b++) n += sizeof(double) * fb_pair_doubles(pos_off[b + 1] - pos_off[b], nrow[b]);
    return n;
}

template <typename T, typename O>
static int fb_launch(const T *post, long ld, const int64_t *row_off, long row_step, const int32_t *nrow, int nstate, const int32_t *seq,
                     const int64_t *pos_off, int nread, int max_npos, int blank, int full, float min_prob, double *score_out, O *occ,
                     long occ_ld, int32_t *emit_row, double *emit_prob, void *workspace, size_t workspace_bytes, slk_stream_t stream)
{
    if (!post || !row_off || !nrow || !pos_off || !score_out || nread < 1 || nstate < 1 || ld < nstate || row_step < 1 || max_npos < 0 ||
        blank < 0 || blank >= nstate || !(min_prob >= 0.0f) || !(min_prob < 1.0f) || (!seq && max_npos > 0) || (occ && occ_ld < nstate))
        return SLK_ERR_INVALID_ARG;
    if (max_npos > FS_MAX_POSITIONS || nstate > FB_MAX_STATES) return SLK_ERR_UNSUPPORTED;
    if (!workspace || (reinterpret_cast<uintptr_t>(workspace) & 15)) return SLK_ERR_WORKSPACE;
    hipStream_t s = slk_stream(stream);
    // the lengths live on the device: they come to the host once, for the exact size and the pairs' offsets
    std::vector<int32_t> h_nrow(nread);
    std::vector<int64_t> h_pos(nread + 1), h_off(nread + 1);
    if (hipStreamSynchronize(s) != hipSuccess || hipMemcpy(h_nrow.data(), nrow, sizeof(int32_t) * nread, hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(h_pos.data(), pos_off, sizeof(int64_t) * (nread + 1), hipMemcpyDeviceToHost) != hipSuccess)
        return SLK_ERR_LAUNCH;
    if (workspace_bytes < slk_forward_backward_workspace_bytes(nread, h_nrow.data(), h_pos.data())) return SLK_ERR_WORKSPACE;
    h_off[0] = (int64_t)(fb_round256((size_t)(nread + 1) * sizeof(int64_t)) / sizeof(double));
    for (int b = 0; b < nread; b++) h_off[b + 1] = h_off[b] + (int64_t)fb_pair_doubles(h_pos[b + 1] - h_pos[b], h_nrow[b]);
    if (hipMemcpy(workspace, h_off.data(), sizeof(int64_t) * (nread + 1), hipMemcpyHostToDevice) != hipSuccess) return SLK_ERR_LAUNCH;

    fb_args A;
    fs_args &a = A.f;
    a.post = post; a.ld = ld; a.row_step = row_step; a.row_off = row_off; a.nrow = nrow; a.seq = seq; a.pos_off = pos_off;
    a.score_out = score_out; a.nstate = nstate; a.blank = blank; a.full = full ? 1 : 0;
    a.min_prob = min_prob; a.one_m = one_minus(min_prob, (double)min_prob);
    A.occ = occ; A.occ_ld = occ_ld; A.emit_row = emit_row; A.emit_prob = emit_prob;
    A.ws = static_cast<double *>(workspace); A.ws_off = static_cast<const int64_t *>(workspace);
    const int maxppt = max_npos < 2 * FS_THREADS ? 2 : (max_npos < 8 * FS_THREADS ? 8 : 32);
    if (occ) {
        hipLaunchKernelGGL((forward_backward_zero_kernel<O>), dim3(nread, FB_ZERO_SPLIT), dim3(FS_THREADS), 0, s, A, maxppt);
        const int rc = slk_launch_status();
        if (rc != SLK_OK) return rc;
    }
    const size_t lds = 2 * sizeof(unsigned long long) * (size_t)nstate;
    auto launch = [&](auto kernel) {
        if (lds > 64 * 1024) {
            const bool ok = SLK_PER_DEVICE(bool, hipFuncSetAttribute(reinterpret_cast<const void *>(kernel),
                                                                     hipFuncAttributeMaxDynamicSharedMemorySize,
                                                                     (int)(2 * sizeof(unsigned long long) * FB_MAX_STATES)) == hipSuccess);
            if (!ok) return (int)SLK_ERR_UNSUPPORTED;
        }
        hipLaunchKernelGGL(kernel, dim3(nread), dim3(FS_THREADS), lds, s, A);
        return slk_launch_status();
    };
    if (maxppt == 2) return launch(forward_backward_kernel<T, O, 2>);
    if (maxppt == 8) return launch(forward_backward_kernel<T, O, 8>);
    return launch(forward_backward_kernel<T, O, 32>);
}

extern "C" int slk_forward_backward_batch_f32(const float *post, long ld, const int64_t *row_off, long row_step, const int32_t *nrow,
                                              int nstate, const int32_t *seq, const int64_t *pos_off, int nread, int max_npos, int blank,
                                              int full, float min_prob, double *score, float *occ, long occ_ld, int32_t *emit_row,
                                              double *emit_prob, void *workspace, size_t workspace_bytes, slk_stream_t stream)
{
    return fb_launch<float, float>(post, ld, row_off, row_step, nrow, nstate, seq, pos_off, nread, max_npos, blank, full, min_prob, score,
                                   occ, occ_ld, emit_row, emit_prob, workspace, workspace_bytes, stream);
}

extern "C" int slk_forward_backward_batch_f64(const double *post, long ld, const int64_t *row_off, long row_step, const int32_t *nrow,
                                              int nstate, const int32_t *seq, const int64_t *pos_off, int nread, int max_npos, int blank,
                                              int full, double *score, double *occ, long occ_ld, int32_t *emit_row, double *emit_prob,
                                              void *workspace, size_t workspace_bytes, slk_stream_t stream)
{
    return fb_launch<double, double>(post, ld, row_off, row_step, nrow, nstate, seq, pos_off, nread, max_npos, blank, full, 0.0f, score,
                                     occ, occ_ld, emit_row, emit_prob, workspace, workspace_bytes, stream);
}
