// olddecode.hip -- the decoder of NON-transducer k-mer models on gfx950 (what basecall.decode_post(transducer=False) runs).
//
//   decode.prepare_post(drop_bad=True)     sloika/decode.py:21-36
//   olddecode.estimate_transitions         sloika/olddecode.py:93-117
//   olddecode.decode_profile               sloika/olddecode.py:13-73     (forward :36-65, backtrace :67-71)
//   olddecode.decode_simple                sloika/olddecode.py:85-90     (decode_profile without weights)
// olddecode.decode_transition (:76-82) cannot be called in the reference (np.copy of an itertools.repeat, then trans[:, 1]) and
// has no kernel here.
//
// One workgroup per read in every kernel, and every reduction in an order that depends on the read alone: what a read gets does not
// depend on what shares the launch.  Reads of a ragged batch carry their own row count in lens[b] (0 <= lens[b] <= T; the rows a
// read lost with its bad states are gone before the decoder sees it).
//
// Numerics (design/olddecode.md):
//   * prepare: float32, the row sum in numpy's own summation tree (blocks of <= 128 values, eight strided accumulators combined as
//     ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)), halves at n/2), one IEEE division, then decode.hip's prepare_post arithmetic: bit for
//     bit what numpy writes.
//   * transitions: the three sums per event in float64 (a product of two float32 values is exact there); the reference sums in float32.
//   * the recurrence: float64, as numpy runs it (a float32 row plus an np.float64 scalar promotes); every operation is one rounded
//     add or a maximum, so path and score are bit-exact functions of the float32 log-posteriors and the float64 weights.
// No MFMA and no inline asm: plain C++, DPP and lane builtins.
#include "common.h"

#define OD_ETA 1e-10f
#define OD_ROW_FILL 1e-10              /* olddecode.py:99-100: the last row of the estimate */
#define OD_LOG4 1.3862943611198906     /* np.log(4),  olddecode.py:9  */
#define OD_LOG16 2.772588722239781     /* np.log(16), olddecode.py:10 */
#define OD_BT_BYTES 32768              /* traceback bytes the backtrace stages in LDS at a time */

static inline bool od_dims(int nbase, int klen, int *nkmer)
{
    if (nbase != 4 || klen < 3 || klen > 6) return false;          // basecall.py:48; 64 .. 4096 states
    *nkmer = 1 << (2 * klen);
    return true;
}

__device__ __forceinline__ int od_len(const int *lens, int b, int T) { return lens ? min(max(lens[b], 0), T) : T; }

// Natural log of a float32 value, rounded once from the float64 log.  decode.hip's v_log_f32 * ln 2 was measured here first: its
// values lie 2.8e-8 (relative) to one side, which adds up over a read instead of averaging out -- ten times the distance numpy's
// float32 log keeps from a float64 evaluation of the same read (design/olddecode.md).  The logs do not sit on the score chain.
__device__ __forceinline__ float od_logf(float x) { return (float)log((double)x); }

// ------------------------------------------------------------------------------------------------------
// 1. decode.prepare_post(drop_bad=True) (decode.py:31-36): rows whose first arg-max is column 0 leave, column 0 leaves, the rest is
// renormalised and floored.  256 rows at a time: wave w finds the keep flags of its 64 rows (a row's first maximum is column 0 unless
// a later column is strictly greater), the ballots give every kept row its place, then each wave writes its own kept rows.
// ------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) prepare_drop_bad_kernel(const float *__restrict__ post, int T, int B, int N, float min_prob,
                                                               float one_m, const int *__restrict__ lens, float *__restrict__ out,
                                                               int32_t *__restrict__ kept, int32_t *__restrict__ kept_rows)
{
    __shared__ unsigned long long masks[4];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int S = N + 1, L = od_len(lens, b, T);
    const int nblk = N >= 128 ? N / 128 : 1, blen = N >= 128 ? 128 : N;      // numpy's blocks of at most 128 values
    int base = 0;
    for (int r0 = 0; r0 < L; r0 += 256) {
        bool mine = false;
        for (int i = 0; i < 64; i++) {
            const int t = r0 + wave * 64 + i;
            if (t >= L) break;                                               // (the same for the whole wave)
            const float *p = post + ((size_t)t * B + b) * S;
            const float p0 = p[0];
            bool gt = false;
            for (int s = 1 + lane; s < S; s += 64) gt |= p[s] > p0;
            const bool keep = __any(gt) != 0;                                // decode.py:32-33: np.argmax(row) > 0
            if (lane == i) mine = keep;
        }
        const unsigned long long m = __ballot(mine);
        if (lane == 0) masks[wave] = m;
        __syncthreads();
        int dest = base, total = 0;
        for (int w = 0; w < 4; w++) {
            const int n = __popcll(masks[w]);
            if (w < wave) dest += n;
            total += n;
        }
        for (unsigned long long rem = m; rem; rem &= rem - 1, dest++) {
            const int t = r0 + wave * 64 + (__ffsll(rem) - 1);
            const float *x = post + ((size_t)t * B + b) * S + 1;
            // np.sum(row) in float32 (decode.py:34), numpy's tree: lane 8 * blk + k is accumulator k of block blk
            float part[4] = {0.f, 0.f, 0.f, 0.f};
            for (int m0 = 0; m0 < nblk; m0 += 8) {
                const int blk = m0 + (lane >> 3);
                float r = 0.f;
                if (blk < nblk) {
                    const float *a = x + blk * blen + (lane & 7);
                    r = a[0];
                    for (int k = 8; k < blen; k += 8) r = __fadd_rn(r, a[k]);
                }
                r = __fadd_rn(r, __shfl_xor(r, 1));                          // (r0+r1), (r2+r3), ...
                r = __fadd_rn(r, __shfl_xor(r, 2));
                r = __fadd_rn(r, __shfl_xor(r, 4));                          // one block
                if (nblk >= 2) r = __fadd_rn(r, __shfl_xor(r, 8));           // halves at n/2, down to the blocks
                if (nblk >= 4) r = __fadd_rn(r, __shfl_xor(r, 16));
                if (nblk >= 8) r = __fadd_rn(r, __shfl_xor(r, 32));
                part[m0 >> 3] = r;
            }
            float tot = nblk > 8 ? __fadd_rn(__fadd_rn(part[0], part[1]), __fadd_rn(part[2], part[3])) : part[0];
            tot = __shfl(tot, 0);
            float *o = out + ((size_t)dest * B + b) * N;
            for (int s = lane; s < N; s += 64)                               // decode.py:35-36
                o[s] = __fadd_rn(min_prob, __fmul_rn(one_m, __fdiv_rn(x[s], tot)));
            if (kept_rows && lane == 0) kept_rows[(size_t)b * T + dest] = t;
        }
        base += total;
        __syncthreads();
    }
    if (tid == 0) kept[b] = base;
    if (kept_rows)
        for (int i = base + tid; i < T; i += 256) kept_rows[(size_t)b * T + i] = -1;
}

extern "C" int slk_prepare_post_drop_bad_f32(const float *post, int T, int B, int nbase, int klen, float min_prob,
                                             const int32_t *lens, float *out, int32_t *kept, int32_t *kept_rows,
                                             slk_stream_t stream)
{
    int nkmer;
    if (!post || !out || !kept || T < 1 || B < 1 || post == out) return SLK_ERR_INVALID_ARG;
    if (!od_dims(nbase, klen, &nkmer)) return SLK_ERR_INVALID_ARG;
    hipLaunchKernelGGL(prepare_drop_bad_kernel, dim3(B), dim3(256), 0, slk_stream(stream), post, T, B, nkmer, min_prob,
                       (float)(1.0 - (double)min_prob), lens, out, kept, kept_rows);
    return slk_launch_status();
}

// ------------------------------------------------------------------------------------------------------
// 2. olddecode.estimate_transitions (olddecode.py:93-117).  With A4[j] = sum_a prev[a N/4 + j] and G4[j] = sum_b cur[4j + b]:
//   stay = sum_s prev[s] cur[s]     step = (sum_j A4[j] G4[j]) / 4     skip = (sum_q A16[q] G16[q]) / 16
// A wave takes an event; lane j a group of four states; the four lanes of a quad add up G16 and split A16 between them.
// ------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double od_wave_sum(double x)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o);
    return x;
}

__global__ void __launch_bounds__(256) estimate_transitions_kernel(const float *__restrict__ post, int T, int B, int N, int have_trans,
                                                                   double p0, double p1, double p2, double eta,
                                                                   const int *__restrict__ lens, double *out, double *__restrict__ log_out)
{
    __shared__ double red[3][256];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int L = od_len(lens, b, T), n4 = N / 4, n16 = N / 16;
    double *res = out + (size_t)b * T * 3;
    for (int ev = 1 + wave; ev < L; ev += 4) {
        const float *a = post + ((size_t)(ev - 1) * B + b) * N, *c = post + ((size_t)ev * B + b) * N;
        double stay = 0.0, step = 0.0, skip = 0.0;
        for (int j = lane; j < n4; j += 64) {                                  // (n4 is a multiple of 16: whole quads)
            const float4 cv = *reinterpret_cast<const float4 *>(c + 4 * j), av = *reinterpret_cast<const float4 *>(a + 4 * j);
            stay += (double)av.x * cv.x;
            stay += (double)av.y * cv.y;
            stay += (double)av.z * cv.z;
            stay += (double)av.w * cv.w;
            const double g4 = ((double)cv.x + cv.y) + ((double)cv.z + cv.w);
            const double a4 = ((double)a[j] + a[n4 + j]) + ((double)a[2 * n4 + j] + a[3 * n4 + j]);
            step += a4 * g4;
            double g16 = g4 + __shfl_xor(g4, 1);
            g16 += __shfl_xor(g16, 2);
            const int k = (j & 3) * n16 + (j >> 2);                            // this lane's quarter of A16[j >> 2]
            const double a16 = ((double)a[k] + a[n4 + k]) + ((double)a[2 * n4 + k] + a[3 * n4 + k]);
            skip += a16 * g16;
        }
        stay = od_wave_sum(stay);
        step = od_wave_sum(step);
        skip = od_wave_sum(skip);
        if (lane == 0) {
            res[3 * (ev - 1)] = stay;
            res[3 * (ev - 1) + 1] = step * 0.25;
            res[3 * (ev - 1) + 2] = skip * 0.0625;
        }
    }
    if (tid < 3 && L > 0) res[3 * (L - 1) + tid] = OD_ROW_FILL;
    __syncthreads();
    double t0 = p0, t1 = p1, t2 = p2;
    if (!have_trans) {                                                         // olddecode.py:110-112: the read's own column sums
        double s0 = 0.0, s1 = 0.0, s2 = 0.0;
        for (int r = tid; r < L; r += 256) { s0 += res[3 * r]; s1 += res[3 * r + 1]; s2 += res[3 * r + 2]; }
        red[0][tid] = s0; red[1][tid] = s1; red[2][tid] = s2;
        __syncthreads();
        for (int o = 128; o > 0; o >>= 1) {
            if (tid < o) { red[0][tid] += red[0][tid + o]; red[1][tid] += red[1][tid + o]; red[2][tid] += red[2][tid + o]; }
            __syncthreads();
        }
        t0 = red[0][0]; t1 = red[1][0]; t2 = red[2][0];
        const double s = (t0 + t1) + t2;
        t0 /= s; t1 /= s; t2 /= s;
    }
    for (int r = tid; r < T; r += 256) {                                       // olddecode.py:114-115
        double x0 = 0.0, x1 = 0.0, x2 = 0.0;
        if (r < L) {
            x0 = res[3 * r] * t0; x1 = res[3 * r + 1] * t1; x2 = res[3 * r + 2] * t2;
            const double s = (x0 + x1) + x2;
            x0 /= s; x1 /= s; x2 /= s;
        }
        res[3 * r] = x0; res[3 * r + 1] = x1; res[3 * r + 2] = x2;
        if (log_out) {                                                         // basecall.py:50: np.log(eta + trans)
            double *lo = log_out + ((size_t)b * T + r) * 3;
            lo[0] = r < L ? log(eta + x0) : 0.0;
            lo[1] = r < L ? log(eta + x1) : 0.0;
            lo[2] = r < L ? log(eta + x2) : 0.0;
        }
    }
}

extern "C" int slk_estimate_transitions_f64(const float *post, int T, int B, int nbase, int klen, int have_trans, double t_stay,
                                            double t_step, double t_skip, double eta, const int32_t *lens, double *trans_out,
                                            double *log_trans_out, slk_stream_t stream)
{
    int nkmer;
    if (!post || !trans_out || T < 1 || B < 1 || (reinterpret_cast<uintptr_t>(post) & 15)) return SLK_ERR_INVALID_ARG;
    if (!od_dims(nbase, klen, &nkmer)) return SLK_ERR_INVALID_ARG;
    hipLaunchKernelGGL(estimate_transitions_kernel, dim3(B), dim3(256), 0, slk_stream(stream), post, T, B, nkmer, have_trans ? 1 : 0,
                       t_stay, t_step, t_skip, eta, lens, trans_out, log_trans_out);
    return slk_launch_status();
}

// ------------------------------------------------------------------------------------------------------
// 3. olddecode.decode_profile, forward (olddecode.py:36-65).  Thread j owns to-states 4j .. 4j+3, which share their four step
// predecessors a N/4 + j; the quad j >> 2 shares the sixteen skip predecessors (a 4 + b) N/16 + (j >> 2): lane c of the quad
// reduces the four with b = c, two DPP exchanges finish (first maximum in a 4 + b order, np.argmax over the reshaped view).
// Scores ping-pong between two float64 vectors in LDS, a thread's own four stay in registers; one barrier per step.
//
// The slip move wants the workgroup-wide maximum of the previous scores and its FIRST arg-max every step: a thread takes it where it
// WRITES its scores -- maximum of its four, maximum of the wave (DPP inside a row of 16 lanes, then the four rows), first lane that
// holds it (lanes own ascending states) -- and leaves (value, state) per wave in LDS, ping-pong like the scores; the next step combines
// the <= 16 wave entries in wave order.  The same entries give the final score and state.
//
// Per state the reference runs stay, slip, step, skip through np.where(score > new, old, new): the LAST candidate that equals the
// maximum wins.  Slip, step and skip are the same for the four states of a thread, so their winner is found once.
// Traceback: a byte per state and step (bits 0-1: 0 stay, 1 slip, 2 step, 3 skip; bits 2-5: a, or a 4 + b) and the slip source, 16 bits
// per step.
// ------------------------------------------------------------------------------------------------------
template <int CTL>
__device__ __forceinline__ int od_dpp_i(int x) { return __builtin_amdgcn_update_dpp(x, x, CTL, 0xf, 0xf, false); }
template <int CTL>
__device__ __forceinline__ double od_dpp_d(double x)
{
    return __hiloint2double(od_dpp_i<CTL>(__double2hiint(x)), od_dpp_i<CTL>(__double2loint(x)));
}
__device__ __forceinline__ double od_readlane_d(double x, int l)
{
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(x), l), __builtin_amdgcn_readlane(__double2loint(x), l));
}
__device__ __forceinline__ double od_wave_max(double m)
{
    m = fmax(m, od_dpp_d<0xB1>(m));                    // quad_perm [1,0,3,2]
    m = fmax(m, od_dpp_d<0x4E>(m));                    // quad_perm [2,3,0,1]
    m = fmax(m, od_dpp_d<0x141>(m));                   // row_half_mirror
    m = fmax(m, od_dpp_d<0x140>(m));                   // row_mirror: every lane holds the maximum of its row of 16
    return fmax(fmax(od_readlane_d(m, 0), od_readlane_d(m, 16)), fmax(od_readlane_d(m, 32), od_readlane_d(m, 48)));
}

template <int KLEN>
__global__ void __launch_bounds__(((1 << (2 * KLEN - 2)) < 64 ? 64 : (1 << (2 * KLEN - 2))))
    decode_profile_forward_kernel(const float *__restrict__ post, int T, int B, int mode, const double *__restrict__ trans,
                                  double log_slip, const int *__restrict__ lens, uint8_t *__restrict__ tb,
                                  uint16_t *__restrict__ slipsrc, int32_t *__restrict__ best_out, double *__restrict__ score_out)
{
    constexpr int N = 1 << (2 * KLEN), N4 = N / 4, N16 = N / 16, NTH = N4 < 64 ? 64 : N4, NW = NTH / 64;
    extern __shared__ __attribute__((aligned(16))) double od_sm[];
    double *vb0 = od_sm, *vb1 = od_sm + N;                   // scores of even / odd steps
    double *wmax = od_sm + 2 * N;                            // [2][NW] maximum of each wave's scores
    int *widx = reinterpret_cast<int *>(wmax + 2 * NW);      // [2][NW] its first state
    const int b = blockIdx.x, j = threadIdx.x, lane = j & 63, wave = j >> 6;
    const int L = od_len(lens, b, T);
    if (L == 0) {                                            // a read that lost every row
        if (j == 0) { score_out[b] = __longlong_as_double(0x7ff8000000000000LL); best_out[b] = -1; }
        return;
    }
    const bool active = j < N4;
    const int jj = active ? j : 0, q = jj >> 2, c = jj & 3;
    const float *pb = post + (size_t)b * N + 4 * jj;
    const size_t tstride = (size_t)B * N;
    uint8_t *tbb = tb + (size_t)b * T * N;
    uint16_t *slb = slipsrc + (size_t)b * T;
    auto load_row = [&](int t) { return *reinterpret_cast<const float4 *>(pb + (size_t)t * tstride); };
    auto xf = [&](float p) { return mode == SLK_POST_LOG ? p : od_logf(__fadd_rn(p, OD_ETA)); };          // olddecode.py:23-25
    auto publish = [&](const double (&v)[4], int par) {
        double m = v[0];
        int mi = 0;
#pragma unroll
        for (int cc = 1; cc < 4; cc++)
            if (v[cc] > m) { m = v[cc]; mi = cc; }
        if (!active) m = -INFINITY;
        const double wm = od_wave_max(m);
        const unsigned long long holders = __ballot(active && m == wm);
        const int src = holders ? __ffsll(holders) - 1 : 0;
        const int idx = __shfl(4 * jj + mi, src);
        if (lane == 0) { wmax[par * NW + wave] = wm; widx[par * NW + wave] = idx; }
    };
    auto combine = [&](int par, double &gm, int &gi) {       // first maximum over the waves, in wave (= state) order
        gm = wmax[par * NW];
        gi = widx[par * NW];
#pragma unroll
        for (int w = 1; w < NW; w++) {
            const double x = wmax[par * NW + w];
            const int xi = widx[par * NW + w];
            if (x > gm) { gm = x; gi = xi; }
        }
    };
    auto store4 = [&](double *v, const double (&x)[4]) {
        *reinterpret_cast<double2 *>(v + 4 * jj) = make_double2(x[0], x[1]);
        *reinterpret_cast<double2 *>(v + 4 * jj + 2) = make_double2(x[2], x[3]);
    };

    // step 0: pscore = lpost[0]  (olddecode.py:36)
    double own[4];
    {
        const float4 r = load_row(0);
        own[0] = xf(r.x); own[1] = xf(r.y); own[2] = xf(r.z); own[3] = xf(r.w);
    }
    if (active) store4(vb0, own);
    publish(own, 0);
    float4 nxt = load_row(L > 1 ? 1 : 0);
    __syncthreads();

    for (int t = 1; t < L; t++) {
        const float4 cur = nxt;
        nxt = load_row(t + 1 < L ? t + 1 : L - 1);           // a full step ahead of its use
        const double *vold = (t & 1) ? vb0 : vb1;
        double *vnew = (t & 1) ? vb1 : vb0;
        double gm;
        int gi;
        combine((t - 1) & 1, gm, gi);
        double t0 = 0.0, t1 = 0.0, t2 = 0.0;                 // olddecode.py:27-32: no weights, and then no log 4 / log 16 either
        if (trans) {
            const double *tp = trans + ((size_t)b * T + (t - 1)) * 3;
            t0 = tp[0];
            t1 = tp[1] - OD_LOG4;
            t2 = tp[2] - OD_LOG16;
        }
        // step: maximum over a, first wins (olddecode.py:52-53)
        double sm = vold[jj];
        int sa = 0;
#pragma unroll
        for (int a = 1; a < 4; a++) {
            const double x = vold[a * N4 + jj];
            if (x > sm) { sm = x; sa = a; }
        }
        // skip: maximum over a 4 + b, first wins (olddecode.py:59-60); this lane's share is b = c
        double km = vold[c * N16 + q];
        int ka = c;
#pragma unroll
        for (int a = 1; a < 4; a++) {
            const double x = vold[a * N4 + c * N16 + q];
            if (x > km) { km = x; ka = a * 4 + c; }
        }
        {
            const double ov = od_dpp_d<0xB1>(km);
            const int ok = od_dpp_i<0xB1>(ka);
            const bool take = (ov > km) | ((ov == km) & (ok < ka));
            km = take ? ov : km;
            ka = take ? ok : ka;
        }
        {
            const double ov = od_dpp_d<0x4E>(km);
            const int ok = od_dpp_i<0x4E>(ka);
            const bool take = (ov > km) | ((ov == km) & (ok < ka));
            km = take ? ov : km;
            ka = take ? ok : ka;
        }
        // slip, step, skip in the reference's order: a later candidate wins a tie (olddecode.py:47-48, 54-55, 61-62)
        double mv = gm + log_slip;                           // olddecode.py:45
        uint32_t mc = 1u;
        const double stepv = sm + t1, skipv = km + t2;
        if (!(mv > stepv)) mc = 2u | ((uint32_t)sa << 2);
        mv = fmax(mv, stepv);
        if (!(mv > skipv)) mc = 3u | ((uint32_t)ka << 2);
        mv = fmax(mv, skipv);
        const double lp[4] = {xf(cur.x), xf(cur.y), xf(cur.z), xf(cur.w)};
        uint32_t codes = 0;
#pragma unroll
        for (int cc = 0; cc < 4; cc++) {
            const double stay = own[cc] + t0;                // olddecode.py:42
            const bool keep = stay > mv;
            codes |= (keep ? 0u : mc) << (8 * cc);
            own[cc] = fmax(stay, mv) + lp[cc];               // olddecode.py:65
        }
        if (active) {
            store4(vnew, own);
            *reinterpret_cast<uint32_t *>(tbb + (size_t)t * N + 4 * jj) = codes;
        }
        if (j == 0) slb[t] = (uint16_t)gi;                   // olddecode.py:46
        publish(own, t & 1);
        __syncthreads();
    }
    if (j == 0) {                                            // olddecode.py:68, 73
        double gm;
        int gi;
        combine((L - 1) & 1, gm, gi);
        score_out[b] = gm;
        best_out[b] = gi;
    }
}

// ------------------------------------------------------------------------------------------------------
// 4. backtrace (olddecode.py:67-71): one state per row, so the path is as long as the read; one wave per read stages blocks of
// traceback rows in LDS, its first lane walks them.
// ------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(64) decode_profile_backtrace_kernel(const uint8_t *__restrict__ tb, const uint16_t *__restrict__ slipsrc,
                                                                      const int32_t *__restrict__ best, int T, int N, int tblk,
                                                                      const int *__restrict__ lens, int32_t *__restrict__ path_out,
                                                                      int32_t *__restrict__ len_out)
{
    __shared__ __attribute__((aligned(16))) uint8_t blk[OD_BT_BYTES];
    const int b = blockIdx.x, lane = threadIdx.x;
    const int L = od_len(lens, b, T), n4 = N / 4, n16 = N / 16;
    int32_t *path = path_out + (size_t)b * T;
    const uint8_t *tbb = tb + (size_t)b * T * N;
    const uint16_t *slb = slipsrc + (size_t)b * T;
    for (int i = L + lane; i < T; i += 64) path[i] = -1;
    if (lane == 0) len_out[b] = L;
    if (L == 0) return;
    int cur = best[b];
    if (lane == 0) path[L - 1] = cur;
    for (int t1 = L; t1 > 1; t1 -= tblk) {                   // rows [t0, t1)
        const int t0 = max(1, t1 - tblk);
        const int nvec = (t1 - t0) * (N / 16);
        const uint4 *src = reinterpret_cast<const uint4 *>(tbb + (size_t)t0 * N);
        __syncthreads();
        for (int k = lane; k < nvec; k += 64) reinterpret_cast<uint4 *>(blk)[k] = src[k];
        __syncthreads();
        if (lane == 0) {
            for (int t = t1 - 1; t >= t0; t--) {
                const int code = blk[(t - t0) * N + cur];
                const int kind = code & 3, arg = code >> 2;
                if (kind == 1) cur = slb[t];
                else if (kind == 2) cur = arg * n4 + (cur >> 2);
                else if (kind == 3) cur = arg * n16 + (cur >> 4);
                path[t - 1] = cur;
            }
        }
        cur = __shfl(cur, 0);
    }
}

static inline size_t od_round256(size_t x) { return (x + 255) & ~(size_t)255; }

extern "C" size_t slk_decode_profile_workspace_bytes(int T, int B, int nbase, int klen)
{
    int nkmer;
    if (T < 1 || B < 1 || !od_dims(nbase, klen, &nkmer)) return 0;
    return od_round256((size_t)B * T * nkmer) + od_round256((size_t)B * T * sizeof(uint16_t)) + od_round256((size_t)B * sizeof(int32_t));
}

template <int KLEN>
static int launch_profile_forward(const float *post, int T, int B, int mode, const double *trans, double log_slip, const int *lens,
                                  uint8_t *tb, uint16_t *slipsrc, int32_t *best, double *score_out, hipStream_t s)
{
    constexpr int N = 1 << (2 * KLEN), N4 = N / 4, NTH = N4 < 64 ? 64 : N4, NW = NTH / 64;
    const size_t lds = sizeof(double) * (2 * (size_t)N + 2 * NW) + sizeof(int) * 2 * NW;
    if (lds > 64 * 1024) {
        const bool ok = SLK_PER_DEVICE(bool, hipFuncSetAttribute(reinterpret_cast<const void *>(decode_profile_forward_kernel<KLEN>),
                                                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) == hipSuccess);
        if (!ok) return SLK_ERR_UNSUPPORTED;
    }
    hipLaunchKernelGGL((decode_profile_forward_kernel<KLEN>), dim3(B), dim3(NTH), lds, s, post, T, B, mode, trans, log_slip, lens, tb,
                       slipsrc, best, score_out);
    return slk_launch_status();
}

extern "C" int slk_decode_profile_f64(const float *post, int T, int B, int nbase, int klen, int input_mode, const double *trans,
                                      double log_slip, const int32_t *lens, void *workspace, size_t workspace_bytes,
                                      double *score_out, int32_t *path_out, int32_t *len_out, slk_stream_t stream)
{
    int nkmer;
    if (!post || !score_out || !path_out || !len_out || T < 1 || B < 1 || (input_mode != SLK_POST_PLAIN && input_mode != SLK_POST_LOG) ||
        (reinterpret_cast<uintptr_t>(post) & 15))
        return SLK_ERR_INVALID_ARG;
    if (!od_dims(nbase, klen, &nkmer)) return SLK_ERR_INVALID_ARG;
    if (!workspace || (reinterpret_cast<uintptr_t>(workspace) & 15) || workspace_bytes < slk_decode_profile_workspace_bytes(T, B, nbase, klen))
        return SLK_ERR_WORKSPACE;
    uint8_t *tb = static_cast<uint8_t *>(workspace);
    uint16_t *slipsrc = reinterpret_cast<uint16_t *>(tb + od_round256((size_t)B * T * nkmer));
    int32_t *best = reinterpret_cast<int32_t *>(reinterpret_cast<uint8_t *>(slipsrc) + od_round256((size_t)B * T * sizeof(uint16_t)));
    hipStream_t s = slk_stream(stream);
    int rc;
    switch (klen) {
    case 3: rc = launch_profile_forward<3>(post, T, B, input_mode, trans, log_slip, lens, tb, slipsrc, best, score_out, s); break;
    case 4: rc = launch_profile_forward<4>(post, T, B, input_mode, trans, log_slip, lens, tb, slipsrc, best, score_out, s); break;
    case 5: rc = launch_profile_forward<5>(post, T, B, input_mode, trans, log_slip, lens, tb, slipsrc, best, score_out, s); break;
    default: rc = launch_profile_forward<6>(post, T, B, input_mode, trans, log_slip, lens, tb, slipsrc, best, score_out, s); break;
    }
    if (rc != SLK_OK) return rc;
    int tblk = OD_BT_BYTES / nkmer;
    if (tblk > T) tblk = T;
    hipLaunchKernelGGL(decode_profile_backtrace_kernel, dim3(B), dim3(64), 0, s, tb, slipsrc, best, T, nkmer, tblk, lens, path_out,
                       len_out);
    return slk_launch_status();
}
