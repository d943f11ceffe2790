// bar16_common.h -- helpers shared by the barrier-stepped Gru kernels (gru_bar16.hip: four chunks per workgroup,
// gru_bar16d.hip: eight, gru_bar16q.hip: sixteen): barriers that wait for LDS the cheap way, the five-instruction tanh, 3-term split
// MFMA sequences and the projection's MFMAs with weights named in accumulation registers; then what the three plans derive alike from
// (insize, n) (Bar16Dims), the interval function of their service waves, the weight images (their statements are bar16_proj_image.h
// and bar16_rec_image.h, included by the kernels' prologues and by the pack kernel's functions here) and the layout of a pack; at the
// end the host side the three files share: the table of shapes, the entry points they call across files and THE launch of one of two
// instantiations of a kernel, which every launcher of the family goes through.
#pragma once
#include <type_traits>

#include "f16split.h"

template <bool REAL = true>
__device__ __forceinline__ void lds_bar()
{
    if constexpr (REAL) asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    else asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
}
// barrier for a wave whose two youngest LDS operations are reads of its OWN data: LDS executes a wave's operations in
// order, so everything older -- the writes the other waves are waiting for -- has been performed once at most two remain
template <bool REAL = true>
__device__ __forceinline__ void lds_bar_2reads()
{
    if constexpr (REAL) asm volatile("s_waitcnt lgkmcnt(2)\n\ts_barrier" ::: "memory");
    else asm volatile("s_waitcnt lgkmcnt(2)" ::: "memory");
}
__device__ __forceinline__ void lds_fence() { asm volatile("" ::: "memory"); }
// tanh through one exp, 1 - 2/(exp(2x)+1), written so that it is five instructions (the same values as slk_tanh: 2x and
// 2r are exact)
__device__ __forceinline__ float tanh5(float x)
{
    const float e = __builtin_amdgcn_exp2f(x * 2.8853900817779268f);
    return fmaf(-2.0f, __builtin_amdgcn_rcpf(e + 1.0f), 1.0f);
}
__device__ __forceinline__ float sigmoid4(float x)
{
    return __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(x * -1.4426950408889634f));
}

template <int V>
using ic = std::integral_constant<int, V>;
template <int B_, int E_, class F>
__device__ __forceinline__ void static_for(F &&f)
{
    if constexpr (B_ < E_) {
        f(ic<B_>{});
        static_for<B_ + 1, E_>(f);
    }
}

// acc0 += W0.h, acc1 += W1.h as 3-term splits with the two accumulation chains interleaved: consecutive MFMAs never depend on
// each other (per accumulator the order of the terms is that of mfma3)
__device__ __forceinline__ void mfma3x2(const half8 &w0_hi, const half8 &w0_lo, const half8 &w1_hi, const half8 &w1_lo,
                                        const half8 &h_hi, const half8 &h_lo, f32x4 &acc0, f32x4 &acc1)
{
    acc0 = __builtin_amdgcn_mfma_f32_16x16x32_f16(w0_hi, h_lo, acc0, 0, 0, 0);
    acc1 = __builtin_amdgcn_mfma_f32_16x16x32_f16(w1_hi, h_lo, acc1, 0, 0, 0);
    acc0 = __builtin_amdgcn_mfma_f32_16x16x32_f16(w0_lo, h_hi, acc0, 0, 0, 0);
    acc1 = __builtin_amdgcn_mfma_f32_16x16x32_f16(w1_lo, h_hi, acc1, 0, 0, 0);
    acc0 = __builtin_amdgcn_mfma_f32_16x16x32_f16(w0_hi, h_hi, acc0, 0, 0, 0);
    acc1 = __builtin_amdgcn_mfma_f32_16x16x32_f16(w1_hi, h_hi, acc1, 0, 0, 0);
}
// Projection weights in ACCUMULATION registers (a wave alone on its SIMD has 256 of them next to its 256 ordinary ones), named
// directly as the MFMA's A operand.  hipcc treats those registers as spill space and copies every operand back (four
// v_accvgpr_read per operand and use); operands only ever used through an "a" constraint stay where they are.
__device__ __forceinline__ half8 to_acc_regs(half8 v)
{
    half8 a;
    asm volatile("" : "=a"(a) : "0"(v));
    return a;
}
// a whole tile: acc = sum over K blocks of the 3-term split, first MFMA with a zero C operand (no VALU write of the accumulator
// in front of an instruction the compiler does not know to be an MFMA), then let the matrix pipe drain before ordinary
// instructions read the result (the compiler's hazard bookkeeping does not see asm)
template <int KBLK_>
__device__ __forceinline__ f32x4 tile_mfma_acc(const half8 *w_hi, const half8 *w_lo, const half8 *x_hi, const half8 *x_lo)
{
    f32x4 acc;
    asm volatile("v_mfma_f32_16x16x32_f16 %0, %1, %2, 0" : "=&v"(acc) : "a"(w_hi[0]), "v"(x_lo[0]));
    asm volatile("v_mfma_f32_16x16x32_f16 %0, %1, %2, %0" : "+v"(acc) : "a"(w_lo[0]), "v"(x_hi[0]));
    asm volatile("v_mfma_f32_16x16x32_f16 %0, %1, %2, %0" : "+v"(acc) : "a"(w_hi[0]), "v"(x_hi[0]));
#pragma unroll
    for (int kb = 1; kb < KBLK_; kb++) {
        asm volatile("v_mfma_f32_16x16x32_f16 %0, %1, %2, %0" : "+v"(acc) : "a"(w_hi[kb]), "v"(x_lo[kb]));
        asm volatile("v_mfma_f32_16x16x32_f16 %0, %1, %2, %0" : "+v"(acc) : "a"(w_lo[kb]), "v"(x_hi[kb]));
        asm volatile("v_mfma_f32_16x16x32_f16 %0, %1, %2, %0" : "+v"(acc) : "a"(w_hi[kb]), "v"(x_hi[kb]));
    }
    return acc;
}
// (Eight wait states: what hipcc itself puts between a v_mfma_f32_16x16x32_f16 and a vector instruction that reads its result; the
//  hardware does not interlock that read, and seven is where every register arrives -- tools/probes/mfma_read_hazard_probe.hip.)
// ONLY behind v_mfma_f32_16x16x32_f16 (a four-pass MFMA: the figure is that instruction's); a 32x32 tile (eight or sixteen passes) needs
// more -- f32x4 in the signature is the guard: a sixteen-register accumulator does not convert.
__device__ __forceinline__ void mfma_drain(f32x4 &a) { asm volatile("s_nop 7" : "+v"(a)); }
__device__ __forceinline__ void mfma_drain2(f32x4 &a, f32x4 &b) { asm volatile("s_nop 7" : "+v"(a), "+v"(b)); }
// one K block of one tile, accumulator kept across steps (chain waves); FIRST: start from zero
template <bool FIRST>
__device__ __forceinline__ void block_mfma_acc(f32x4 &acc, const half8 &w_hi, const half8 &w_lo, const half8 &x_hi, const half8 &x_lo)
{
    if constexpr (FIRST) asm volatile("v_mfma_f32_16x16x32_f16 %0, %1, %2, 0" : "=&v"(acc) : "a"(w_hi), "v"(x_lo));
    else asm volatile("v_mfma_f32_16x16x32_f16 %0, %1, %2, %0" : "+v"(acc) : "a"(w_hi), "v"(x_lo));
    asm volatile("v_mfma_f32_16x16x32_f16 %0, %1, %2, %0" : "+v"(acc) : "a"(w_lo), "v"(x_hi));
    asm volatile("v_mfma_f32_16x16x32_f16 %0, %1, %2, %0" : "+v"(acc) : "a"(w_hi), "v"(x_hi));
}

// one tile's product with one K block, three terms (per accumulator the order of mfma3), weights in accumulation registers
template <bool FIRST>
__device__ __forceinline__ void tile_block_mfma(f32x4 &a, const half8 &w_hi, const half8 &w_lo, const half8 &bh, const half8 &bl)
{
    if constexpr (FIRST) asm volatile("v_mfma_f32_16x16x32_f16 %0, %1, %2, 0" : "=&v"(a) : "a"(w_hi), "v"(bl));
    else asm volatile("v_mfma_f32_16x16x32_f16 %0, %1, %2, %0" : "+v"(a) : "a"(w_hi), "v"(bl));
    asm volatile("v_mfma_f32_16x16x32_f16 %0, %1, %2, %0" : "+v"(a) : "a"(w_lo), "v"(bh));
    asm volatile("v_mfma_f32_16x16x32_f16 %0, %1, %2, %0" : "+v"(a) : "a"(w_hi), "v"(bh));
}
// z products of one K block for the wave's two tiles, weights in accumulation registers, the two accumulation chains interleaved
// (per accumulator the order of the terms is that of mfma3)
template <bool FIRST>
__device__ __forceinline__ void z_block_mfma(f32x4 &a0, f32x4 &a1, const half8 &w0_hi, const half8 &w0_lo, const half8 &w1_hi,
                                             const half8 &w1_lo, const half8 &bh, const half8 &bl)
{
    if constexpr (FIRST) {
        asm volatile("v_mfma_f32_16x16x32_f16 %0, %1, %2, 0" : "=&v"(a0) : "a"(w0_hi), "v"(bl));
        asm volatile("v_mfma_f32_16x16x32_f16 %0, %1, %2, 0" : "=&v"(a1) : "a"(w1_hi), "v"(bl));
    } else {
        asm volatile("v_mfma_f32_16x16x32_f16 %0, %1, %2, %0" : "+v"(a0) : "a"(w0_hi), "v"(bl));
        asm volatile("v_mfma_f32_16x16x32_f16 %0, %1, %2, %0" : "+v"(a1) : "a"(w1_hi), "v"(bl));
    }
    asm volatile("v_mfma_f32_16x16x32_f16 %0, %1, %2, %0" : "+v"(a0) : "a"(w0_lo), "v"(bh));
    asm volatile("v_mfma_f32_16x16x32_f16 %0, %1, %2, %0" : "+v"(a1) : "a"(w1_lo), "v"(bh));
    asm volatile("v_mfma_f32_16x16x32_f16 %0, %1, %2, %0" : "+v"(a0) : "a"(w0_hi), "v"(bh));
    asm volatile("v_mfma_f32_16x16x32_f16 %0, %1, %2, %0" : "+v"(a1) : "a"(w1_hi), "v"(bh));
}
// ---- two MFMAs per product instead of three: the state's hi and lo halves in DIFFERENT column groups --------------------------
// With four chunks per workgroup the 16 columns of the recurrent MFMAs hold four copies of every chunk (lane (g, q, c) reads
// column 4q + c, the copies differ in q).  Let the copies q = 0, 1 carry the hi half of the state and q = 2, 3 the lo half (one
// operand fetch per K block instead of two: the lane picks its image by q): then W_lo.B and W_hi.B give, in a hi column,
// lo.hi + hi.hi and, in a lo column, lo.lo + hi.lo -- all four terms of (W_hi + W_lo)(h_hi + h_lo) from TWO instructions -- and the
// product for row 4g+j of chunk c is the sum of register j over the columns (c, q) and (c, q ^ 2).  pick_mix does that sum and the
// row selection at once: four v_add_f32 whose first source comes from the lane eight columns away (row_ror:8) and whose bank mask
// lets only the lane quartet q = j write register j's sum -- one instruction more than sel4's three selects.
__device__ __forceinline__ void mfma2x2(const half8 &w0_hi, const half8 &w0_lo, const half8 &w1_hi, const half8 &w1_lo, const half8 &bm,
                                        f32x4 &acc0, f32x4 &acc1)
{
    acc0 = __builtin_amdgcn_mfma_f32_16x16x32_f16(w0_lo, bm, acc0, 0, 0, 0);
    acc1 = __builtin_amdgcn_mfma_f32_16x16x32_f16(w1_lo, bm, acc1, 0, 0, 0);
    acc0 = __builtin_amdgcn_mfma_f32_16x16x32_f16(w0_hi, bm, acc0, 0, 0, 0);
    acc1 = __builtin_amdgcn_mfma_f32_16x16x32_f16(w1_hi, bm, acc1, 0, 0, 0);
}
// the same with the weights in accumulation registers (asm: see z_block_mfma)
template <bool FIRST>
__device__ __forceinline__ void z_block_mfma2(f32x4 &a0, f32x4 &a1, const half8 &w0_hi, const half8 &w0_lo, const half8 &w1_hi,
                                              const half8 &w1_lo, const half8 &bm)
{
    if constexpr (FIRST) {
        asm volatile("v_mfma_f32_16x16x32_f16 %0, %1, %2, 0" : "=&v"(a0) : "a"(w0_lo), "v"(bm));
        asm volatile("v_mfma_f32_16x16x32_f16 %0, %1, %2, 0" : "=&v"(a1) : "a"(w1_lo), "v"(bm));
    } else {
        asm volatile("v_mfma_f32_16x16x32_f16 %0, %1, %2, %0" : "+v"(a0) : "a"(w0_lo), "v"(bm));
        asm volatile("v_mfma_f32_16x16x32_f16 %0, %1, %2, %0" : "+v"(a1) : "a"(w1_lo), "v"(bm));
    }
    asm volatile("v_mfma_f32_16x16x32_f16 %0, %1, %2, %0" : "+v"(a0) : "a"(w0_hi), "v"(bm));
    asm volatile("v_mfma_f32_16x16x32_f16 %0, %1, %2, %0" : "+v"(a1) : "a"(w1_hi), "v"(bm));
}
// one tile's product with one K block of the mixed operand
// An operand of an asm MFMA must not have been written by a vector instruction in the instruction slot or two before it: the hardware
// does not interlock that (the MFMA reads what the register held before), and hipcc counts no wait states for what is inside asm.
// Operands normally arrive from LDS behind an s_waitcnt; the exception is a CONSTANT -- the zero state of step 0 -- which hipcc
// materialises with v_mov right in front of its first use (found when a rescheduled step 0 of gru_bar16q_kernel<64,64,true> computed
// its first r gate from whatever the registers held: tests/test_gpu_gru_bar16.py, saved gates).  settle() makes the value opaque (no
// rematerialisation later) and puts the wait states behind its definition, once.
__device__ __forceinline__ void settle(half8 &v) { asm volatile("s_nop 1" : "+v"(v)); }
__device__ __forceinline__ void mfma2(const half8 &w_hi, const half8 &w_lo, const half8 &bm, f32x4 &acc)
{
    acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(w_lo, bm, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(w_hi, bm, acc, 0, 0, 0);
}
// WS: wait states in front of the first read.  The compiler does not look into asm: a DPP source written by a VALU instruction just
// before needs two, an accumulator written by an MFMA eight counted from that MFMA (mfma_drain) -- callers that have pinned other
// instructions in between pass what is left of the eight.
template <int WS = 2>
__device__ __forceinline__ float pick_mix(const f32x4 &a)
{
    static_assert(WS >= 2 && WS <= 8, "wait states");
    float r;
    asm volatile("s_nop %c5\n\t"
                 "v_add_f32_dpp %0, %1, %1 row_ror:8 row_mask:0xf bank_mask:0x1\n\t"
                 "v_add_f32_dpp %0, %2, %2 row_ror:8 row_mask:0xf bank_mask:0x2\n\t"
                 "v_add_f32_dpp %0, %3, %3 row_ror:8 row_mask:0xf bank_mask:0x4\n\t"
                 "v_add_f32_dpp %0, %4, %4 row_ror:8 row_mask:0xf bank_mask:0x8"
                 : "=&v"(r)
                 : "v"(a[0]), "v"(a[1]), "v"(a[2]), "v"(a[3]), "n"(WS - 1));
    return r;
}
// ... into a register the caller keeps from step to step (see split2_kept).  Not volatile: the scheduler may move it among the MFMAs
// of another gate; `after` is an operand the statement only waits for -- the value whose producer must lie in front of it (the
// accumulator of the tile whose MFMAs supply the wait states, or the result of the pick that does).
template <int WS = 2>
__device__ __forceinline__ void pick_mix_kept(const f32x4 &a, float &r, float after)
{
    static_assert(WS >= 2 && WS <= 8, "wait states");
    asm("s_nop %c5\n\t"
        "v_add_f32_dpp %0, %1, %1 row_ror:8 row_mask:0xf bank_mask:0x1\n\t"
        "v_add_f32_dpp %0, %2, %2 row_ror:8 row_mask:0xf bank_mask:0x2\n\t"
        "v_add_f32_dpp %0, %3, %3 row_ror:8 row_mask:0xf bank_mask:0x4\n\t"
        "v_add_f32_dpp %0, %4, %4 row_ror:8 row_mask:0xf bank_mask:0x8"
        : "+v"(r)
        : "v"(a[0]), "v"(a[1]), "v"(a[2]), "v"(a[3]), "n"(WS - 1), "v"(after));
}
// ---- the same two MFMAs with the operands exchanged: the STATE is A, the weights are B (gru_bar16.hip) ---------------------------------
// The result is the transpose: lane (g' = lane >> 4, n = lane & 15) holds rows 4g' .. 4g'+3 of column n, a column is a neuron of the
// weight tile and a row is whatever the lane that supplies that A row fetched.  With rows 4c + 0 = chunk c's hi image and 4c + 2 = its
// lo image, lane (c, n) finds hi.W in register 0 and lo.W in register 2: the product for (chunk c, neuron n) is their sum, and all 64
// lanes hold 64 different (chunk, neuron) pairs -- no row selection, no DPP.  The products are those of mfma2 (fp16 x fp16 is exact and
// commutative), accumulated over the same k positions in the same order (W_lo first), and hi + lo adds the same two values.
__device__ __forceinline__ void mfma2t(const half8 &am, const half8 &w_hi, const half8 &w_lo, f32x4 &acc)
{
    acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(am, w_lo, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(am, w_hi, acc, 0, 0, 0);
}
// r = a[0] + a[2] behind WS wait states, in the form of pick_mix_kept (plain asm with `after`, a register kept from step to step).  No
// DPP source, so one wait state is the least; the eight behind the MFMA that wrote `a` are the caller's to count as before.
template <int WS = 1>
__device__ __forceinline__ void pick_sum_kept(const f32x4 &a, float &r, float after)
{
    static_assert(WS >= 1 && WS <= 8, "wait states");
    asm("s_nop %c3\n\t"
        "v_add_f32 %0, %1, %2"
        : "+v"(r)
        : "v"(a[0]), "v"(a[2]), "n"(WS - 1), "v"(after));
}
// The same for gru_bar16d.hip's layout (eight chunks per workgroup: the two copies of a chunk sit FOUR columns apart, copy q&1 = 0 carries
// the hi half and owns rows 4g + {0, 1}, copy 1 the lo half and rows 4g + {2, 3}): value j of the lane = register 2(q&1) + j summed over
// both copies.  Two instructions: the even quartets take their partner four lanes up, the odd ones four lanes down.
__device__ __forceinline__ float pick_mix_d(const f32x4 &a, int j)
{
    float r;
    if (j == 0)
        asm volatile("s_nop 1\n\t"
                     "v_add_f32_dpp %0, %1, %1 row_shl:4 row_mask:0xf bank_mask:0x5\n\t"
                     "v_add_f32_dpp %0, %2, %2 row_shr:4 row_mask:0xf bank_mask:0xa"
                     : "=&v"(r)
                     : "v"(a[0]), "v"(a[2]));
    else
        asm volatile("s_nop 1\n\t"
                     "v_add_f32_dpp %0, %1, %1 row_shl:4 row_mask:0xf bank_mask:0x5\n\t"
                     "v_add_f32_dpp %0, %2, %2 row_shr:4 row_mask:0xf bank_mask:0xa"
                     : "=&v"(r)
                     : "v"(a[1]), "v"(a[3]));
    return r;
}
// barrier for a wave whose youngest LDS operation is a read of its own data (lds_bar_2reads with one operand image)
template <bool REAL = true>
__device__ __forceinline__ void lds_bar_1read()
{
    if constexpr (REAL) asm volatile("s_waitcnt lgkmcnt(1)\n\ts_barrier" ::: "memory");
    else asm volatile("s_waitcnt lgkmcnt(1)" ::: "memory");
}

// One projection tile for both sets, weights in accumulation registers: the two accumulation chains alternate (consecutive
// MFMAs never depend on each other) and hook(ic<i>) runs after MFMA i = 0 .. 6 KBLK - 1 -- the matrix pipe keeps the wave's issue
// port for 4 cycles of every 16, the leader's split of x is cut into pieces that fill the rest.
template <int KBLK_, class F>
__device__ __forceinline__ void tile2_mfma_acc(f32x4 &a0, f32x4 &a1, const half8 *w_hi, const half8 *w_lo, const half8 *x0_hi,
                                               const half8 *x0_lo, const half8 *x1_hi, const half8 *x1_lo, F &&hook)
{
    static_for<0, KBLK_>([&](auto KBC) {
        constexpr int kb = decltype(KBC)::value;
        if constexpr (kb == 0) {
            asm volatile("v_mfma_f32_16x16x32_f16 %0, %1, %2, 0" : "=&v"(a0) : "a"(w_hi[0]), "v"(x0_lo[0]));
            hook(ic<0>{});
            // (x0_lo[0] is listed so that the fresh destination does not take over the registers the MFMA just issued still reads:
            //  tests/test_isa_hygiene.py)
            asm volatile("v_mfma_f32_16x16x32_f16 %0, %1, %2, 0" : "=&v"(a1) : "a"(w_hi[0]), "v"(x1_lo[0]), "v"(x0_lo[0]));
            hook(ic<1>{});
        } else {
            asm volatile("v_mfma_f32_16x16x32_f16 %0, %1, %2, %0" : "+v"(a0) : "a"(w_hi[kb]), "v"(x0_lo[kb]));
            hook(ic<6 * kb>{});
            asm volatile("v_mfma_f32_16x16x32_f16 %0, %1, %2, %0" : "+v"(a1) : "a"(w_hi[kb]), "v"(x1_lo[kb]));
            hook(ic<6 * kb + 1>{});
        }
        asm volatile("v_mfma_f32_16x16x32_f16 %0, %1, %2, %0" : "+v"(a0) : "a"(w_lo[kb]), "v"(x0_hi[kb]));
        hook(ic<6 * kb + 2>{});
        asm volatile("v_mfma_f32_16x16x32_f16 %0, %1, %2, %0" : "+v"(a1) : "a"(w_lo[kb]), "v"(x1_hi[kb]));
        hook(ic<6 * kb + 3>{});
        asm volatile("v_mfma_f32_16x16x32_f16 %0, %1, %2, %0" : "+v"(a0) : "a"(w_hi[kb]), "v"(x0_hi[kb]));
        hook(ic<6 * kb + 4>{});
        asm volatile("v_mfma_f32_16x16x32_f16 %0, %1, %2, %0" : "+v"(a1) : "a"(w_hi[kb]), "v"(x1_hi[kb]));
        hook(ic<6 * kb + 5>{});
    });
}

// ---- what the three plans derive from (insize, n) alike ---------------------------------------------------------------------------------
// Per plan, and therefore in the kernels: GS, R, CT, ST, NA, the LDS layouts (OPSTEP / OPIMG, VSTEP, IMG) and the check that CT tiles per
// chain wave and ST per service wave make up NT16.
template <int I, int N>
struct Bar16Dims {
    static constexpr int NCW = N / 32;                   // chain waves = 32-wide K blocks of the recurrent products
    static constexpr int KBS = N / 32;
    static constexpr int NSW = 4 - NCW;                  // service waves
    static constexpr int NT = N / 16;                    // tiles per gate
    static constexpr int NT16 = 3 * NT;                  // tiles of vI rows (z | r | c)
    static constexpr int KBLK = (I + 31) / 32;
    static constexpr int NACAP = 240 / (8 * KBLK);       // 256 accumulation registers, 2 * KBLK * 4 per tile
    static_assert(I % 16 == 0 && N % 32 == 0 && N <= 96, "unsupported size for the barrier-stepped GRU kernel");
    static_assert(KBLK <= 4, "interval plan");
};

// First tile of interval k of a service wave with st tiles per group (and set) when the n intervals of a group take tiles in the
// proportions w[0 .. n-1] (k = n: st).  The tables stand next to the kernels that own them.
__host__ __device__ constexpr int bar16_tile_first(int st, int k, const int *w, int n)
{
    int tot = 0, acc = 0;
    for (int i = 0; i < n; i++) tot += w[i];
    for (int i = 0; i < k && i < n; i++) acc += w[i];
    return k >= n ? st : (acc * st + tot / 2) / tot < st ? (acc * st + tot / 2) / tot : st;
}

// ---- the weight images -------------------------------------------------------------------------------------------------------------------
// Every workgroup of the per-layer kernels makes its images in its prologue; gru_bar16_pack_kernel (gru_bar16.hip) makes the four-chunk
// kernel's once per set of weights with the two functions below.  The arithmetic is ONE text, bar16_proj_image.h and bar16_rec_image.h,
// included here and in the prologues (what it expects in scope: there): a pack holds the bits a prologue makes.  All 64 lanes of the
// wave call these.
// One iW tile -> A operands; returns the row's inverse scale.
template <int I, int KBLK>
__device__ __forceinline__ float bar16_proj_tile(const float *iW, int tile, int pcol, int kg, half8 *hi, half8 *lo)
{
#define BAR16_PROJ_INV(row, inv)
#include "bar16_proj_image.h"
#undef BAR16_PROJ_INV
    return inv;
}
// Recurrent weights of chain wave w, tile p of its two -> B operands; inv_z / inv_r / inv_c: the rows' inverse scales.
template <int N, int KBS>
__device__ __forceinline__ void bar16_rec_tile(const float *sW, const float *sW2, int w, int p, int lane, half8 *wz_hi, half8 *wz_lo,
                                               half8 *wr_hi, half8 *wr_lo, half8 *wc_hi, half8 *wc_lo, float &inv_z, float &inv_r,
                                               float &inv_c)
{
    const int g = lane >> 4;
#define BAR16_REC_INV(iz, ir, ic_) inv_z = iz; inv_r = ir; inv_c = ic_;
#define BAR16_REC_W(a) a
#include "bar16_rec_image.h"
#undef BAR16_REC_W
#undef BAR16_REC_INV
}
// Where the pack keeps them, in 16-byte pieces: every image is 64 consecutive pieces, one per lane, so a wave's prologue is a run of
// 1-KiB loads.  Per chain wave the images of its two tiles -- item(p, gate z / r / c, K block i in ITS rotated order, hi / lo) -- and
// two pieces of inverse scales {iz0, iz1, ir0, ir1}, {ic0, ic1, -, -}; then the projection tiles [tile][K block][hi / lo] as the lane
// of ANY wave holds them (which wave takes which tile is the kernel's business); then invw[3N] and bias[3N] as floats.
template <int I, int N>
struct Bar16Pack {
    using D = Bar16Dims<I, N>;
    static constexpr int NCW = D::NCW, KBS = D::KBS, NT16 = D::NT16, KBLK = D::KBLK;
    static constexpr int REC_ITEMS = 12 * KBS + 2;
    static constexpr size_t PROJ0 = (size_t)NCW * REC_ITEMS * 64;
    static constexpr size_t FLT0 = PROJ0 + (size_t)NT16 * KBLK * 2 * 64;
    static constexpr size_t BYTES = FLT0 * 16 + (size_t)6 * N * sizeof(float);
    __host__ __device__ static constexpr size_t rec(int w, int p, int gate, int i, int hl)
    {
        return ((size_t)w * REC_ITEMS + ((p * 3 + gate) * KBS + i) * 2 + hl) * 64;
    }
    __host__ __device__ static constexpr size_t rec_inv(int w, int k) { return ((size_t)w * REC_ITEMS + 12 * KBS + k) * 64; }
    __host__ __device__ static constexpr size_t proj(int tile, int kb, int hl) { return PROJ0 + ((size_t)(tile * KBLK + kb) * 2 + hl) * 64; }
};

// ---- host side ------------------------------------------------------------------------------------------------------------------------
// THE (insize, n) the three kernels are instantiated for; every dispatcher expands this table (sloika_amd.layers.GRU_LAYER_SHAPES and
// the comment of slk_gru_bar16_f32 in include/sloika_amd.h repeat it).  The order is the order of instantiation, and with it the layout of
// the code object: add at the end.
#define BAR16_SHAPES(X) X(96, 96) X(64, 64) X(32, 96) X(128, 96) X(64, 96) X(48, 32) X(16, 64)
// ... and those with a packed four-chunk kernel (slk_gru_bar16_pack_bytes / _pack_f32 / _stack_f32)
#define BAR16_PACKED_SHAPES(X) X(96, 96) X(64, 64)

// The eight- and sixteen-chunk plans behind slk_gru_bar16_f32 (gru_bar16d.hip, gru_bar16q.hip; same contract): SLK_ERR_UNSUPPORTED when
// no instantiation covers the request or y cannot take the kernel's state stores -- the caller then takes the next smaller plan.
extern "C" int slk_gru_bar16d_launch(const float *x, long ldx, const float *iW, const float *sW, const float *sW2, const float *bias,
                                     float *y, long ldy, int T, int B, int insize, int n, int reverse, const int32_t *lens,
                                     float *zr_out, hipStream_t s);
extern "C" int slk_gru_bar16q_launch(const float *x, long ldx, const float *iW, const float *sW, const float *sW2, const float *bias,
                                     float *y, long ldy, int T, int B, int insize, int n, int reverse, const int32_t *lens,
                                     float *zr_out, hipStream_t s);

// THE launch of one of two instantiations of a kernel (the one that writes the gates or the plain one; the full-batch stack kernel or the
// general one): nwg workgroups of four waves, dyn bytes of dynamic LDS.  The kernels are template arguments, not run-time pointers:
// whatever a launcher keeps per device (SLK_PER_DEVICE) it then keeps per kernel.
template <auto K_FIRST, auto K_SECOND, class... Args>
static int launch_bar16_either(bool first, int nwg, size_t dyn, hipStream_t s, Args... args)
{
    if (first) hipLaunchKernelGGL(K_FIRST, dim3(nwg), dim3(256), dyn, s, args...);
    else hipLaunchKernelGGL(K_SECOND, dim3(nwg), dim3(256), dyn, s, args...);
    return slk_launch_status();
}
// A layer: one workgroup per CHUNKS chunks of the batch; K_SAVE / K_PLAIN: the kernel's instantiations that do / do not write the gates.
template <int CHUNKS, auto K_SAVE, auto K_PLAIN>
static int launch_bar16_chunks(const float *x, long ldx, const float *iW, const float *bias, const float *sW, const float *sW2,
                               float *y, long ldy, int T, int B, int reverse, const int *lens, float *zr_out, hipStream_t s,
                               size_t dyn = 0)
{
    return launch_bar16_either<K_SAVE, K_PLAIN>(zr_out != nullptr, (B + CHUNKS - 1) / CHUNKS, dyn, s, x, ldx, iW, bias, sW, sW2, y, ldy, T,
                                                B, reverse & 1, lens, zr_out);
}
