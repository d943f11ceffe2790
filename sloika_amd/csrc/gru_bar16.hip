// gru_bar16.hip -- a whole Gru layer (sloika/layers.py:1010-1021) in one persistent kernel of FOUR waves per workgroup,
// one per SIMD, in lock step.  Arithmetic: every float32 product as fp16 split terms (f16split.h) with float32 accumulation,
// rows scaled by powers of two.
//
// The plan this one replaced (tools/experiments/gru_fused16.hip, no longer in the library) ran eight waves coupled by progress
// counters in LDS; a step of its chain cost two counter round trips (poll, ballot, retry), shared its SIMDs with the projection
// waves, and lived in 256 registers.  Measured there: of ~2200 cycles per step only ~860 were the chain's MFMAs.  Here:
//   * one wave per SIMD (256 threads, 512 registers each): nobody competes with the chain for issue slots;
//   * the two exchanges of a step (r*h, then h) are two s_barrier -- LDS data written before the barrier is simply there
//     after it, no counters, no retries;
//   * the time-parallel projection vI = x.iW^T + b (four steps at a time) is cut into pieces that the waves execute at
//     fixed places of the step: a chain wave issues its share (CT tiles, one K block per step) behind its write of r*h,
//     under that write's latency (four K blocks of input: right after a barrier, while its LDS reads of the state are in
//     flight); the service waves (the SIMDs without a chain wave) take the rest,
//     split x into fp16 halves ONCE per group for everybody (operand images in LDS), and run the x DMA one request at a
//     time so that they always reach the next barrier before the chain does;
//   * every chain lane owns (neuron, chunk) pairs and stores its new state straight to h_out (sixteen lanes write 64
//     consecutive bytes, a wave a whole 128-byte line per chunk and step): no staging ring, no copy-out pass.
// Layout of the recurrent 16x16x32 tiles: the STATE is the A operand and the weights are B (design/gru_transposed.md).  A row
// 4c + j carries chunk c -- j = 0: its hi half, j = 2: its lo half; rows j = 1, 3 are not used and fetch the neighbouring chunk so
// that a ds_read_b128 touches every bank once -- and a B column is a neuron of the tile, so lane (chunk c = lane >> 4, neuron
// n = lane & 15) finds hi.W in register 0 and lo.W in register 2 of its accumulator: a gate's pre-activation is one v_add_f32
// (bar16_common.h: pick_sum_kept).  The K order of the packed operand images: bar16_rec_image.h.
// Shared with gru_bar16d.hip and gru_bar16q.hip (design/gru_prologue.md): the statements that make the weight images
// (bar16_proj_image.h, bar16_rec_image.h), the shape constants (bar16_common.h: Bar16Dims), the interval function (bar16_tile_first;
// the tables stay with their kernels) and the launch (launch_bar16_either).
#include <limits.h>
#include <stdlib.h>

#include "bar16_common.h"

// Recurrent products take TWO MFMAs each: the state's hi and lo halves ride in different rows of the A operand (bar16_common.h: mfma2t).
//
// Diagnostics (per-section shader-clock stamps, ablation launches, workgroup clocks) exist only in builds with -DSLK_DIAG
// (tools/build_diag_lib.sh; readers: tools/bar16_check.py, tools/bar16_wg_times.py).  ABL bits (results are then garbage):
// 1 = no s_barrier, 2 = chain waves issue no MFMAs, 4 = cheap activations, 8 = service waves only keep the barriers,
// 16 = no stores to h_out, 32 = every workgroup records where it ran and for how long, 64 = chain waves issue no z MFMAs and no z
// epilogue, the blend takes constants (the bound of what moving the update gate off the chain can gain: design/gru_zgate.md),
// 128 = chain waves without their share of the projection (no projection MFMAs, no outputs, no reads of the x operands: the bound of
// what moving it to the service wave can gain), 256 / 512 = the service wave computes six / three of its tiles a second time, spread
// over the intervals as a table for eighteen / fifteen tiles would spread them (whether it still reaches every barrier first:
// design/gru_projection.md), 1024 = the z products stay, the z picks and sigmoid(z), 1 - z, z*h are bit 64's constants (the bound of what
// placing the z epilogue can gain), 2048 = the head of interval A without the vI and x-operand requests and without the stores: the
// gate terms are constants (the bound of what moving them behind the own-block products can gain: design/gru_step_order.md).
// What bit 16 takes away, piece by piece (design/gru_store.md; meaningful on a full batch with B % 4 == 0 and lens = NULL only):
// 4096 = the predicate of the h_out stores and its branch around an empty body, 8192 = both stores without the predicate,
// 16384 = the first store of the two only, 32768 = the stores' row never moves (no pointer bump: everything lands on one row).
#ifdef SLK_DIAG
__device__ unsigned long long slk_dbg_bar16[4][16];
extern "C" SLK_API int slk_debug_read_bar16(unsigned long long *host_out)
{
    return hipMemcpyFromSymbol(host_out, HIP_SYMBOL(slk_dbg_bar16), sizeof(unsigned long long) * 64) == hipSuccess ? SLK_OK
                                                                                                                : SLK_ERR_LAUNCH;
}
__device__ unsigned long long slk_dbg_bar16_wg[1024][4];
extern "C" SLK_API int slk_debug_read_bar16_wg(unsigned long long *host_out)
{
    return hipMemcpyFromSymbol(host_out, HIP_SYMBOL(slk_dbg_bar16_wg), sizeof(unsigned long long) * 4096) == hipSuccess ? SLK_OK
                                                                                                                    : SLK_ERR_LAUNCH;
}
#define BSTAMP(i)                                                                     \
    if constexpr (DIAG) {                                                             \
        unsigned long long tnow;                                                      \
        __builtin_amdgcn_sched_barrier(0);                                            \
        asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(tnow)::"memory");   \
        __builtin_amdgcn_sched_barrier(0);                                            \
        sacc[i] += tnow - tprev;                                                      \
        tprev = tnow;                                                                 \
    }
#else
#define BSTAMP(i)
#endif

// The service wave's tiles per interval, as proportions for bar16_tile_first (bar16_common.h); row = TBL of gru_bar16_body.h.
// row 0: lighter where the leader also splits x (intervals 1..4) and fetches operands (0).
// row 1, a single service wave behind chain waves that project behind their write of r*h (gru_bar16_body.h: LATE): by the stamps
// of row 0 (design/gru_projection.md) the wave reached the barrier behind interval 1 -- a tile and the scale of the coming
// group's rows, in the shorter half of the step -- last of the four, and the one behind interval 4 -- two tiles, a K block of the
// split, the loads of x -- 50 cycles ahead of the chain.  Interval 1 keeps no tile, interval 4 one; 0 and 2, in the longer half, two.
constexpr int BAR16_TILE_W[2][8] = {{1, 1, 1, 1, 2, 2, 2, 2}, {2, 0, 2, 1, 1, 2, 2, 2}};

// ABL bits 256 / 512: tiles an interval of the service wave computes a second time, on top of whatever row of the table it has -- measured on
// row 0 (design/gru_projection.md 1), where they made {2,2,2,2,2,2,3,3} and {1,2,2,2,2,2,2,2} tiles per interval of {1,1,1,1,2,2,2,2}
__host__ __device__ constexpr int tile_extra(int abl, int k)
{
    constexpr int six[8] = {1, 1, 1, 1, 0, 0, 1, 1}, three[8] = {0, 1, 1, 1, 0, 0, 0, 0};
    return (abl & 256) ? six[k] : (abl & 512) ? three[k] : 0;
}

template <int I, int N, bool SAVE, bool DIAG = false, int ABL = 0>
__global__ void __launch_bounds__(256, 1) gru_bar16_kernel(const float *__restrict__ x, long ldx, const float *__restrict__ iW,
                                                           const float *__restrict__ bias, const float *__restrict__ sW,
                                                           const float *__restrict__ sW2, float *__restrict__ h_out, long ldh,
                                                           int T, int B, int reverse, const int *__restrict__ lens,
                                                           float *__restrict__ zr_out)
{
    constexpr bool PACKED = false, FULL = false;
    [[maybe_unused]] const void *const pack = nullptr;
#include "gru_bar16_body.h"
}

// The same layer with its weight images loaded from `pack`: the loop body of gru_bar16_stack_kernel.
// FULLV: the full-batch stores of h (gru_bar16_body.h: FULL).  ABLV: diagnostic builds only.
template <int I, int N, bool FULLV, int ABLV>
__device__ __forceinline__ void gru_bar16_layer_packed(const float *__restrict__ x, long ldx, const void *__restrict__ pack,
                                                       float *__restrict__ h_out, long ldh, int T, int B, int reverse,
                                                       const int *__restrict__ lens)
{
    constexpr bool PACKED = true, SAVE = false, DIAG = false, FULL = FULLV;
    constexpr int ABL = ABLV;
    [[maybe_unused]] const float *const iW = nullptr, *const bias = nullptr, *const sW = nullptr, *const sW2 = nullptr;
    [[maybe_unused]] float *const zr_out = nullptr;
#include "gru_bar16_body.h"
}

// The weight images of one layer, written once per set of weights: blocks 0 .. NCW-1 the recurrent images of chain wave w (and the
// bias), the others one projection tile each.  One wave per block, every lane active.
template <int I, int N>
__global__ void __launch_bounds__(64) gru_bar16_pack_kernel(const float *__restrict__ iW, const float *__restrict__ bias,
                                                            const float *__restrict__ sW, const float *__restrict__ sW2,
                                                            void *__restrict__ pack)
{
    using PK = Bar16Pack<I, N>;
    half8 *const pk8 = static_cast<half8 *>(pack);
    float *const pf = reinterpret_cast<float *>(pk8 + PK::FLT0);
    const int lane = threadIdx.x;
    if ((int)blockIdx.x < PK::NCW) {
        const int w = blockIdx.x;
        float inv_z[2], inv_r[2], inv_c[2];
#pragma unroll
        for (int p = 0; p < 2; p++) {
            half8 wz_hi[PK::KBS], wz_lo[PK::KBS], wr_hi[PK::KBS], wr_lo[PK::KBS], wc_hi[PK::KBS], wc_lo[PK::KBS];
            bar16_rec_tile<N, PK::KBS>(sW, sW2, w, p, lane, wz_hi, wz_lo, wr_hi, wr_lo, wc_hi, wc_lo, inv_z[p], inv_r[p], inv_c[p]);
#pragma unroll
            for (int i = 0; i < PK::KBS; i++) {
                pk8[PK::rec(w, p, 0, i, 0) + lane] = wz_hi[i]; pk8[PK::rec(w, p, 0, i, 1) + lane] = wz_lo[i];
                pk8[PK::rec(w, p, 1, i, 0) + lane] = wr_hi[i]; pk8[PK::rec(w, p, 1, i, 1) + lane] = wr_lo[i];
                pk8[PK::rec(w, p, 2, i, 0) + lane] = wc_hi[i]; pk8[PK::rec(w, p, 2, i, 1) + lane] = wc_lo[i];
            }
        }
        const f32x4 s0 = {inv_z[0], inv_z[1], inv_r[0], inv_r[1]}, s1 = {inv_c[0], inv_c[1], 0.0f, 0.0f};
        *reinterpret_cast<f32x4 *>(pk8 + PK::rec_inv(w, 0) + lane) = s0;
        *reinterpret_cast<f32x4 *>(pk8 + PK::rec_inv(w, 1) + lane) = s1;
        for (int i = 64 * w + lane; i < 3 * N; i += 64 * PK::NCW) pf[3 * N + i] = bias ? bias[i] : 0.0f;
    } else {
        const int tile = blockIdx.x - PK::NCW, pcol = lane & 15, kg = lane >> 4;
        half8 hi[PK::KBLK], lo[PK::KBLK];
        const float inv = bar16_proj_tile<I, PK::KBLK>(iW, tile, pcol, kg, hi, lo);
#pragma unroll
        for (int kb = 0; kb < PK::KBLK; kb++) { pk8[PK::proj(tile, kb, 0) + lane] = hi[kb]; pk8[PK::proj(tile, kb, 1) + lane] = lo[kb]; }
        if (kg == 0) pf[16 * tile + pcol] = inv;
    }
}

// Up to eight layers of one <I, N> in one launch (include/sloika_amd.h: slk_gru_bar16_stack_f32).  Workgroup b of a layer reads the
// rows of chunks 4b .. 4b+3 of its input and writes the rows of the same chunks, so layer k+1 of a workgroup needs layer k of THAT
// workgroup and nothing else: the layers are a loop around the layer above, and the kernel boundary between them -- drain, dispatch,
// the wait for the slowest workgroup of the grid -- becomes one workgroup barrier.  At the boundary every wave has left the layer's
// last interval (chain and service waves execute three barriers in front of the step loop and two per step, whatever T and lens
// are: the conditions of their loops are the same expressions of T); the release / acquire pair at workgroup scope makes the chain
// waves' stores of h_out visible to the leader's loads of x of the next layer (one CU, one vector cache: the release waits for the
// stores, nothing has to be written back or invalidated); the next layer then initialises LDS and its registers as a launch does.
struct Bar16StackArgs {
    slk_gru_stack_layer l[SLK_GRU_STACK_MAX];
};
template <int I, int N, bool FULLV = false, int ABLV = 0>
__global__ void __launch_bounds__(256, 1) gru_bar16_stack_kernel(const Bar16StackArgs a, int nlayer, int T, int B,
                                                                 const int *__restrict__ lens)
{
    for (int k = 0; k < nlayer; k++) {
        const slk_gru_stack_layer &d = a.l[k];
        gru_bar16_layer_packed<I, N, FULLV, ABLV>(d.x, d.ldx, d.pack, d.h_out, d.ldh, T, B, d.reverse & 1,
                                                  (FULLV || (d.reverse & SLK_GRU_STACK_NO_LENS)) ? nullptr : lens);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __syncthreads();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    }
}

// One workgroup per CU: the dynamic LDS to ask for so that two cannot share a CU (asked once per kernel and device).
template <auto KERNEL>
static size_t exclusive_cu_lds_bar()
{
    return SLK_PER_DEVICE(size_t, ([] {
        hipFuncAttributes attr;
        if (hipFuncGetAttributes(&attr, reinterpret_cast<const void *>(KERNEL)) != hipSuccess) return (size_t)0;
        const size_t half_cu = 80 * 1024 + 512;                     // 160 KB of LDS per CU
        const size_t dyn = attr.sharedSizeBytes >= half_cu ? 0 : half_cu - attr.sharedSizeBytes;
        if (dyn && hipFuncSetAttribute(reinterpret_cast<const void *>(KERNEL), hipFuncAttributeMaxDynamicSharedMemorySize,
                                       (int)dyn) != hipSuccess)
            return (size_t)0;
        return dyn;
    }()));
}

template <typename K>
static int bar16_blocks_per_cu(K kernel)
{
    int nb = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, reinterpret_cast<const void *>(kernel), 256, 0) != hipSuccess) return 0;
    return nb;
}

// share_cu: the caller runs more four-chunk workgroups at a time than there are CUs and the instantiation fits two per CU (<= 256
// registers, <= 80 KB of LDS: the 64-wide ones): no dynamic LDS, so that two of them -- the directions of a birnn -- share a CU
template <int I, int N>
static int launch_bar16(const float *x, long ldx, const float *iW, const float *bias, const float *sW, const float *sW2,
                        float *y, long ldy, int T, int B, int reverse, const int *lens, float *zr_out, hipStream_t s, bool share_cu)
{
#ifdef SLK_DIAG
    if constexpr (I == 96 && N == 96) {
        // diagnostic launches (undocumented bits, tools/bar16_check.py; SLOIKA_AMD_BAR16_DIAG forces one for every launch of a
        // process so that tools/bar16_wg_times.py --pipeline can read the clock the kernel gets inside the whole step)
        static const int forced = getenv("SLOIKA_AMD_BAR16_DIAG") ? atoi(getenv("SLOIKA_AMD_BAR16_DIAG")) : 0;
        const int dv = forced ? forced : reverse >> 1;
#define DIAG_LAUNCH(CODE, STAMPS, ABLV)                                                                                   \
        if (dv == CODE) {                                                                                                 \
            constexpr auto K = gru_bar16_kernel<I, N, false, STAMPS, ABLV>;                                               \
            return launch_bar16_chunks<4, K, K>(x, ldx, iW, bias, sW, sW2, y, ldy, T, B, reverse, lens, zr_out, s,       \
                                                exclusive_cu_lds_bar<K>());                                               \
        }
        DIAG_LAUNCH(1, true, 0) DIAG_LAUNCH(2, false, 1) DIAG_LAUNCH(3, false, 2) DIAG_LAUNCH(4, false, 4) DIAG_LAUNCH(5, false, 8)
        DIAG_LAUNCH(6, false, 16) DIAG_LAUNCH(7, false, 9) DIAG_LAUNCH(8, false, 3) DIAG_LAUNCH(9, false, 11) DIAG_LAUNCH(10, false, 31)
        DIAG_LAUNCH(11, false, 32) DIAG_LAUNCH(12, false, 34) DIAG_LAUNCH(13, false, 40) DIAG_LAUNCH(14, false, 42) DIAG_LAUNCH(15, false, 36)
        DIAG_LAUNCH(16, false, 64) DIAG_LAUNCH(17, true, 64) DIAG_LAUNCH(18, false, 128) DIAG_LAUNCH(19, true, 128)
        DIAG_LAUNCH(20, false, 256) DIAG_LAUNCH(21, true, 256) DIAG_LAUNCH(22, false, 512) DIAG_LAUNCH(23, true, 512)
        DIAG_LAUNCH(24, false, 384) DIAG_LAUNCH(25, true, 384) DIAG_LAUNCH(26, false, 640) DIAG_LAUNCH(27, true, 640)
        DIAG_LAUNCH(28, false, 1024) DIAG_LAUNCH(29, true, 1024) DIAG_LAUNCH(30, false, 2048) DIAG_LAUNCH(31, true, 2048)
        DIAG_LAUNCH(32, false, 3072)
        DIAG_LAUNCH(33, false, 4096) DIAG_LAUNCH(34, false, 8192) DIAG_LAUNCH(35, false, 16384) DIAG_LAUNCH(36, false, 32768)
        DIAG_LAUNCH(37, true, 4096) DIAG_LAUNCH(38, true, 8192) DIAG_LAUNCH(39, true, 16384) DIAG_LAUNCH(40, true, 32768)
        DIAG_LAUNCH(41, true, 16)
#undef DIAG_LAUNCH
    }
#endif
    const bool shared = share_cu && N <= 64;
    if (shared) {
        // the caller's plan counts on two of these workgroups per CU: ask the runtime whether they fit (a compiler that takes more
        // than 256 registers or 80 KB of LDS for the instantiation would otherwise halve the plan's speed silently)
        const int fit = zr_out ? SLK_PER_DEVICE(int, bar16_blocks_per_cu(gru_bar16_kernel<I, N, true>))
                               : SLK_PER_DEVICE(int, bar16_blocks_per_cu(gru_bar16_kernel<I, N, false>));
        if (fit < 2) return SLK_ERR_UNSUPPORTED;         // -> slk_gru_bar16_f32 takes the eight-chunk plan
    }
    const size_t dyn = shared ? 0
                       : zr_out ? exclusive_cu_lds_bar<gru_bar16_kernel<I, N, true>>()
                                : exclusive_cu_lds_bar<gru_bar16_kernel<I, N, false>>();
    return launch_bar16_chunks<4, gru_bar16_kernel<I, N, true>, gru_bar16_kernel<I, N, false>>(x, ldx, iW, bias, sW, sW2, y, ldy, T, B,
                                                                                              reverse, lens, zr_out, s, dyn);
}

// More workgroups of four chunks than CUs would run one after the other: such batches take the eight-chunk plan of
// gru_bar16d.hip, and the sixteen-chunk plan of gru_bar16q.hip when the eight-chunk workgroups do not fit either (bits 8-9 of
// `reverse` force a plan per call).  Returns chunks per workgroup divided by four.  This is plan 0 of the C ABI;
// sloika_amd.layers.gru_launch restates it (its rule 3) and always passes an explicit plan.
static int bar16_auto_plan(int B)
{
    const int ncu = SLK_PER_DEVICE(int, ([] {
        int dev = 0, n = 0;
        if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) n = 256;
        return n > 0 ? n : 256;
    }()));
    if ((B + 3) / 4 <= ncu) return 1;
    return (B + 7) / 8 <= ncu ? 2 : 4;
}

// The contract is in include/sloika_amd.h; SLK_ERR_UNSUPPORTED when no instantiation covers the request.
extern "C" int slk_gru_bar16_f32(const float *x, long ldx, const float *iW, const float *sW, const float *sW2,
                                 const float *bias, float *y, long ldy, int T, int B, int insize, int n, int reverse, int act,
                                 int gate_act, const int32_t *lens, float *zr_out, slk_stream_t stream)
{
    if (!x || !iW || !sW || !sW2 || !y || T < 1 || B < 1 || insize < 1 || n < 1 || ldx < insize || ldy < n)
        return SLK_ERR_INVALID_ARG;
    if (act != SLK_ACT_TANH || gate_act != SLK_ACT_SIGMOID) return SLK_ERR_UNSUPPORTED;
    if ((ldx & 3) || (reinterpret_cast<uintptr_t>(x) & 15)) return SLK_ERR_UNSUPPORTED;   // 16-byte DMA pieces
    hipStream_t s = slk_stream(stream);
    const int plan = (reverse >> 8) & 3;                 // include/sloika_amd.h: 0 = by batch size, 1 / 2 / 3 = four / eight / sixteen chunks
    const bool share_cu = (reverse >> 10) & 1;           // ... bit 10: four-chunk workgroups of a 64-wide layer may share a CU
    reverse &= 0xff;
    const int per4 = plan == 1 ? 1 : plan == 2 ? 2 : plan == 3 ? 4 : ((reverse >> 1) == 0 ? bar16_auto_plan(B) : 1);
    if (per4 == 4) {
        const int rc = slk_gru_bar16q_launch(x, ldx, iW, sW, sW2, bias, y, ldy, T, B, insize, n, reverse, lens, zr_out, s);
        if (rc != SLK_ERR_UNSUPPORTED) return rc;
    }
    if (per4 >= 2) {
        const int rc = slk_gru_bar16d_launch(x, ldx, iW, sW, sW2, bias, y, ldy, T, B, insize, n, reverse, lens, zr_out, s);
        if (rc != SLK_ERR_UNSUPPORTED) return rc;
    }
#define BAR16(II, NN)                                                                                                              \
    if (insize == II && n == NN) {                                                                                                 \
        int rc = launch_bar16<II, NN>(x, ldx, iW, bias, sW, sW2, y, ldy, T, B, reverse, lens, zr_out, s, share_cu);                 \
        if (rc == SLK_ERR_UNSUPPORTED && share_cu) {     /* two workgroups per CU do not fit: eight chunks, else one per CU */     \
            rc = slk_gru_bar16d_launch(x, ldx, iW, sW, sW2, bias, y, ldy, T, B, insize, n, reverse, lens, zr_out, s);              \
            if (rc == SLK_ERR_UNSUPPORTED) rc = launch_bar16<II, NN>(x, ldx, iW, bias, sW, sW2, y, ldy, T, B, reverse, lens, zr_out, s, false); \
        }                                                                                                                          \
        return rc;                                                                                                                 \
    }
    BAR16_SHAPES(BAR16)
#undef BAR16
    return SLK_ERR_UNSUPPORTED;
}

// ---- weights packed once per model, layers stacked in one launch (include/sloika_amd.h; shapes: BAR16_PACKED_SHAPES) ------------------
extern "C" size_t slk_gru_bar16_pack_bytes(int insize, int n)
{
#define BAR16(II, NN) if (insize == II && n == NN) return Bar16Pack<II, NN>::BYTES;
    BAR16_PACKED_SHAPES(BAR16)
#undef BAR16
    return 0;
}

extern "C" int slk_gru_bar16_pack_f32(const float *iW, const float *bias, const float *sW, const float *sW2, int insize, int n,
                                      void *pack, slk_stream_t stream)
{
    if (!iW || !sW || !sW2 || !pack || insize < 1 || n < 1) return SLK_ERR_INVALID_ARG;
    if (reinterpret_cast<uintptr_t>(pack) & 15) return SLK_ERR_INVALID_ARG;
    hipStream_t s = slk_stream(stream);
#define BAR16(II, NN)                                                                                                      \
    if (insize == II && n == NN) {                                                                                         \
        using PK = Bar16Pack<II, NN>;                                                                                      \
        hipLaunchKernelGGL((gru_bar16_pack_kernel<II, NN>), dim3(PK::NCW + PK::NT16), dim3(64), 0, s, iW, bias, sW, sW2, pack); \
        return slk_launch_status();                                                                                        \
    }
    BAR16_PACKED_SHAPES(BAR16)
#undef BAR16
    return SLK_ERR_UNSUPPORTED;
}

// Which kernel a stack launch takes (include/sloika_amd.h): 1 = the full-batch instantiation (gru_bar16_body.h: FULL), whose chain
// waves store h without a predicate, 0 = the general one.
extern "C" int slk_gru_bar16_stack_path(int B, int ragged) { return !ragged && B >= 4 && !(B & 3) ? 1 : 0; }

#ifdef SLK_DIAG
// (tools/bar16_check.py) the 96 -> 96 stack launches of the process take <FULL, ABL> of the pairs below
static int dbg_stack_full = -1, dbg_stack_abl = 0;
extern "C" SLK_API void slk_debug_bar16_stack_variant(int full, int abl) { dbg_stack_full = full; dbg_stack_abl = abl; }
#endif

// full: the full-batch instantiation (ABLV: diagnostic builds only)
template <int I, int N, int ABLV = 0>
static int launch_bar16_stack(bool full, const Bar16StackArgs &a, int nlayer, int T, int B, const int *lens, hipStream_t s)
{
    const size_t dyn = full ? exclusive_cu_lds_bar<gru_bar16_stack_kernel<I, N, true, ABLV>>()
                            : exclusive_cu_lds_bar<gru_bar16_stack_kernel<I, N, false, ABLV>>();
    return launch_bar16_either<gru_bar16_stack_kernel<I, N, true, ABLV>, gru_bar16_stack_kernel<I, N, false, ABLV>>(
        full, (B + 3) / 4, dyn, s, a, nlayer, T, B, lens);
}

extern "C" int slk_gru_bar16_stack_f32(int nlayer, const slk_gru_stack_layer *layers, int insize, int n, int T, int B,
                                       const int32_t *lens, slk_stream_t stream)
{
    if (!layers || nlayer < 1 || nlayer > SLK_GRU_STACK_MAX || T < 1 || B < 1 || insize < 1 || n < 1) return SLK_ERR_INVALID_ARG;
    if (nlayer > 1 && insize != n) return SLK_ERR_INVALID_ARG;                // a layer's output is the next layer's input
    Bar16StackArgs a = {};
    bool ragged = false;                                                      // does any layer look at lens
    for (int k = 0; k < nlayer; k++) {
        const slk_gru_stack_layer &d = layers[k];
        if (!d.x || !d.h_out || !d.pack || d.ldx < insize || d.ldh < n || d.x == d.h_out) return SLK_ERR_INVALID_ARG;
        if ((d.ldx & 3) || (reinterpret_cast<uintptr_t>(d.x) & 15) || (reinterpret_cast<uintptr_t>(d.pack) & 15))
            return SLK_ERR_UNSUPPORTED;                                       // 16-byte pieces, as slk_gru_bar16_f32
        a.l[k] = d;
        ragged = ragged || (lens && !(d.reverse & SLK_GRU_STACK_NO_LENS));
    }
    hipStream_t s = slk_stream(stream);
    const bool full = slk_gru_bar16_stack_path(B, ragged) == 1;
#ifdef SLK_DIAG
    if (insize == 96 && n == 96 && dbg_stack_full >= 0) {
        // (the caller's business: FULL on a full batch without lens only)
#define DIAG_STACK(FULLV, ABLV) \
        if (dbg_stack_full == FULLV && dbg_stack_abl == ABLV) return launch_bar16_stack<96, 96, ABLV>(FULLV != 0, a, nlayer, T, B, lens, s);
        DIAG_STACK(0, 0) DIAG_STACK(0, 16) DIAG_STACK(0, 4096) DIAG_STACK(0, 8192) DIAG_STACK(0, 16384) DIAG_STACK(0, 32768)
        DIAG_STACK(1, 0) DIAG_STACK(1, 16) DIAG_STACK(1, 16384)
#undef DIAG_STACK
        return SLK_ERR_UNSUPPORTED;
    }
#endif
#define BAR16(II, NN)                                                                                                      \
    if (insize == II && n == NN) return launch_bar16_stack<II, NN>(full, a, nlayer, T, B, lens, s);
    BAR16_PACKED_SHAPES(BAR16)
#undef BAR16
    return SLK_ERR_UNSUPPORTED;
}
