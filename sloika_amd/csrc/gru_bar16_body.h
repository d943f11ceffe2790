// gru_bar16_body.h -- the body of one layer of the four-chunk Gru kernel, all four waves of the workgroup.  Included by
// gru_bar16.hip inside gru_bar16_kernel (a launch per layer; PACKED = false: the prologue makes the weight images from iW, sW, sW2
// with the statements of bar16_proj_image.h and bar16_rec_image.h) and inside gru_bar16_layer_packed (the loop body of
// gru_bar16_stack_kernel; PACKED = true: the images, their inverse scales and the bias come from `pack`, which gru_bar16_pack_kernel
// wrote with the same statements).  Text, not a function: as a function inlined into both, the per-layer kernels came out of the
// compiler with another register assignment and 1.6 % slower (design/gru_prologue.md: the same holds for the image statements).
// In scope where it is included: I, N, SAVE, DIAG, ABL, PACKED, FULL (constants) and x, ldx, iW, bias, sW, sW2, pack, h_out, ldh, T,
// B, reverse, lens, zr_out.
// FULL (design/gru_store.md): the launcher saw that no layer looks at lens and that B % 4 == 0, so every chunk slot of every workgroup
// is a chunk of T steps: no lane computes, tests or branches on a predicate for its stores of h.  Only the packed stack kernels take it.
    static_assert(!PACKED || !SAVE, "the training pass changes its weights every step: no pack");
    static_assert(!FULL || (PACKED && !SAVE), "the full-batch stores are the packed stack kernel's");
    using PK = Bar16Pack<I, N>;
    [[maybe_unused]] const half8 *const pk8 = static_cast<const half8 *>(pack);
    using DM = Bar16Dims<I, N>;                          // bar16_common.h: what (I, N) alone decide
    constexpr int NCW = DM::NCW, KBS = DM::KBS, NSW = DM::NSW, NT = DM::NT, NT16 = DM::NT16, KBLK = DM::KBLK, NACAP = DM::NACAP;
    constexpr int GS = 4;                                // steps per projection group (16 MFMA columns = 4 steps x 4 chunks)
    constexpr int R = 2 * GS;                            // vI ring: group G+1 is written while group G is consumed
    // projection tiles of a chain wave (weights in accumulation registers); three where four K blocks of the input would not leave
    // the service wave room for the tiles it keeps in ordinary registers next to the x rows it loads (128 -> 96 spilled)
    constexpr int CT = NCW == 3 ? (KBLK == 4 ? 3 : 2) : 0;
    constexpr int ST = (NT16 - NCW * CT) / NSW;                         // ... of a service wave
    // Where a chain wave issues its share's MFMAs (design/gru_projection.md).  LATE: behind the write of r*h, in front of barrier B, with
    // the x operands requested at the start of the same interval -- six MFMAs end under the write's own latency there, while in the LDS
    // round trip at the start of interval A (the other place) they stand in front of the r products of the other blocks together with
    // the own r and z blocks.  Four K blocks of input (128 -> 96: nine MFMAs in every step, the outputs right behind the last) keep the
    // round trip.
    constexpr bool LATE = CT > 0 && KBLK <= 3;
    constexpr int TBL = (NSW == 1 && KBLK <= 3) ? 1 : 0;                // the service wave's tiles per interval: row of BAR16_TILE_W
    constexpr int NA = ST < NACAP ? ST : NACAP;                               // of which this many keep their weights in accumulation registers
    static_assert(NCW * CT + NSW * ST == NT16 && ST <= 21, "tile assignment");
    // dwords of one operand image: [step][k block][slot(k group, chunk)][8 halves]; the steps lie 32 banks apart so that the 16-lane
    // groups of a ds_read_b128 (lanes of two k groups and two steps each) find their pieces on different banks
    constexpr int OPSTEP = KBLK * 64 + 32;
    constexpr int OPIMG = GS * OPSTEP;
    // floats of one step's vI: [tile][g][chunk ^ (g & 2)][r], row = 16 tile + 4g + r; + 16: the steps of a projection tile (one per
    // lane quartet of its 16-byte writes) on different banks.
    // slot(g, chunk): where the 16 bytes of (g, chunk) lie among the sixteen of a vI tile or of a K block of a state image.  A chain
    // lane owns neuron lane & 15 of chunk lane >> 4, so the half waves of its 4-byte accesses are two chunks times every g: with the
    // plain order 4g + chunk, g and g + 2 would meet on one bank (the banks of 4-byte accesses repeat every 32 dwords); g = 2, 3
    // therefore keep their chunks in the order 2, 3, 0, 1.  The 16-byte accesses see the same pieces per lane group as before.
    constexpr int VSTEP = NT16 * 64 + 16;
    auto slot = [](int g_, int c_) { return 4 * g_ + (c_ ^ (g_ & 2)); };

    __shared__ __attribute__((aligned(16))) unsigned xop_hi[2 * OPIMG], xop_lo[2 * OPIMG];
    __shared__ __attribute__((aligned(16))) float xinv_lds[2 * 16];
    __shared__ __attribute__((aligned(16))) float vbuf[R * VSTEP];
    // One image: [k block][slot(g, chunk)][4 dwords = 8 halves].  The lo image lies 32 banks behind the hi image: a 16-lane group of a
    // ds_read_b128 of the mixed operand (two k groups, every chunk, hi and lo) reads 16 pieces on 64 different banks
    // (2N + 4 put the two on the same banks: SQ_LDS_BANK_CONFLICT was 37 % of the kernel's LDS cycles)
    constexpr int IMG = 2 * N + (2 * N % 64 == 0 ? 32 : 2 * N % 64 == 32 ? 0 : 4);
    __shared__ __attribute__((aligned(16))) unsigned h_img[2 * IMG], rh_img[2 * IMG];             // hi image, then lo image
    unsigned *const h_hi = h_img, *const h_lo = h_img + IMG, *const rh_hi = rh_img, *const rh_lo = rh_img + IMG;
    __shared__ __attribute__((aligned(16))) float bias_lds[3 * N], invw_lds[3 * N];

    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int b0 = blockIdx.x * 4;
#ifdef SLK_DIAG
    unsigned long long wg_t0 = 0, wg_r0 = 0;
    if constexpr (ABL & 32) asm volatile("s_memtime %0\n\ts_memrealtime %1\n\ts_waitcnt lgkmcnt(0)" : "=s"(wg_t0), "=s"(wg_r0)::"memory");
#endif

    for (int i = tid; i < 2 * N; i += 256) { h_hi[i] = 0u; h_lo[i] = 0u; }             // h(-1) = 0
    if constexpr (PACKED) {
        const float *pf = reinterpret_cast<const float *>(pk8 + PK::FLT0);
        for (int i = tid; i < 3 * N; i += 256) { invw_lds[i] = pf[i]; bias_lds[i] = pf[3 * N + i]; }
    } else {
        for (int i = tid; i < 3 * N; i += 256) bias_lds[i] = bias ? bias[i] : 0.0f;
    }

    // ---------------- projection pieces shared by both kinds of wave ----------------
    const int pcol = lane & 15, kg = lane >> 4;          // operand row / column and k group of this lane
    const int pstep = pcol >> 2, pc = pcol & 3;          // as a B column: (step in group, chunk)
    // + 64 kb: my 16 bytes of an operand image, in dwords (the pieces of a K block in the order of slot() as well: every 16-byte access
    // sees the same pieces per lane group in either order, and the lane's offset into a vI tile stays the one into a K block)
    const int poff = pstep * OPSTEP + 4 * slot(kg, pc);
    auto ldH = [](const unsigned *img, int off) { return *reinterpret_cast<const half8 *>(img + off); };
    // iW tile -> A operands (lane: row pcol of the tile, k = 32 kb + 8 kg + 0..7), row scale remembered in invw_lds
    auto load_tile = [&](int tile, half8 *hi, half8 *lo) {
        if constexpr (PACKED) {
            // (the tile is the same for the whole wave: said so, the images' addresses are a scalar base and the lane's 16 bytes)
            const half8 *const src = pk8 + PK::proj(__builtin_amdgcn_readfirstlane(tile), 0, 0);
#pragma unroll
            for (int kb = 0; kb < KBLK; kb++) { hi[kb] = src[PK::proj(0, kb, 0) - PK::PROJ0 + lane]; lo[kb] = src[PK::proj(0, kb, 1) - PK::PROJ0 + lane]; }
        } else {
#define BAR16_PROJ_INV(row, inv) if (kg == 0) invw_lds[row] = inv;
#include "bar16_proj_image.h"
#undef BAR16_PROJ_INV
        }
    };
    // accumulator of a tile for group G1 -> vI ring: lane holds rows 4 kg + r of column (pstep, pc)
    auto proj_out = [&](int tile, const f32x4 &acc, int G1) {
        const float xin = xinv_lds[(G1 & 1) * 16 + pcol];
        const f32x4 iw = *reinterpret_cast<const f32x4 *>(&invw_lds[16 * tile + 4 * kg]);
        const f32x4 bs = *reinterpret_cast<const f32x4 *>(&bias_lds[16 * tile + 4 * kg]);
        f32x4 o;
#pragma unroll
        for (int r = 0; r < 4; r++) o[r] = fmaf(acc[r] * xin, iw[r], bs[r]);
        const int st = GS * G1 + pstep;
        *reinterpret_cast<f32x4 *>(&vbuf[(st % R) * VSTEP + 64 * tile + 4 * slot(kg, pc)]) = o;
    };
    const int NG = (T + GS - 1) / GS;

    if (wave < NCW) {
        // =================================================================================================
        // chain waves
        // =================================================================================================
        const int w = wave;
        const int g = lane >> 4;                         // as an operand: k group
        const int cn = lane >> 4, nn = lane & 15;        // as an owner: chunk, neuron of each of my two tiles
        // recurrent weights: B operands (column lane & 15 = neuron, k group g), K blocks in the rotated order w, w+1, ... (element
        // (g, j) of block kb is neuron 32 kb + 16 (j&1) + 4 g + (j>>1), the order the owners' packed writes create), rows scaled to [1, 2)
        half8 wz_hi[2][KBS], wz_lo[2][KBS], wr_hi[2][KBS], wr_lo[2][KBS], wc_hi[2][KBS], wc_lo[2][KBS];
        float inv_z[2], inv_r[2], inv_c[2];
        if constexpr (PACKED) {
            const half8 *const src = pk8 + PK::rec(__builtin_amdgcn_readfirstlane(w), 0, 0, 0, 0);      // (scalar base, as in load_tile)
#pragma unroll
            for (int p = 0; p < 2; p++) {
#pragma unroll
                for (int i = 0; i < KBS; i++) {
                    wz_hi[p][i] = src[PK::rec(0, p, 0, i, 0) + lane]; wz_lo[p][i] = src[PK::rec(0, p, 0, i, 1) + lane];
                    wr_hi[p][i] = src[PK::rec(0, p, 1, i, 0) + lane]; wr_lo[p][i] = src[PK::rec(0, p, 1, i, 1) + lane];
                    wc_hi[p][i] = src[PK::rec(0, p, 2, i, 0) + lane]; wc_lo[p][i] = src[PK::rec(0, p, 2, i, 1) + lane];
                }
            }
            const f32x4 s0 = *reinterpret_cast<const f32x4 *>(src + PK::rec_inv(0, 0) + lane);
            const f32x4 s1 = *reinterpret_cast<const f32x4 *>(src + PK::rec_inv(0, 1) + lane);
            inv_z[0] = s0[0]; inv_z[1] = s0[1]; inv_r[0] = s0[2]; inv_r[1] = s0[3]; inv_c[0] = s1[0]; inv_c[1] = s1[1];
        } else {
#pragma unroll
            for (int p = 0; p < 2; p++) {
                // (kgroup_max: every lane of a row has the row's scale, and its neuron IS its row)
#define BAR16_REC_INV(iz, ir, ic_) inv_z[p] = iz; inv_r[p] = ir; inv_c[p] = ic_;
#define BAR16_REC_W(a) a[p]
#include "bar16_rec_image.h"
#undef BAR16_REC_W
#undef BAR16_REC_INV
                // (one tile's rows at a time: interleaved, the two conversions are where the kernel needs the most registers, and the
                //  64-wide instantiations must stay within the 256 that let two workgroups share a CU)
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        constexpr int CTA = CT > 0 ? CT : 1;
        half8 pw_hi[CTA][KBLK], pw_lo[CTA][KBLK];
        f32x4 pacc[CTA];
        if constexpr (CT > 0) {
#pragma unroll
            for (int t = 0; t < CT; t++) {
                load_tile(w * CT + t, pw_hi[t], pw_lo[t]);
#pragma unroll
                for (int kb = 0; kb < KBLK; kb++) { pw_hi[t][kb] = to_acc_regs(pw_hi[t][kb]); pw_lo[t][kb] = to_acc_regs(pw_lo[t][kb]); }
            }
        }
        // my 16 bytes of K block (w + i) % KBS as row lane & 15 = 4 ac + aj of the A operand, in dwords: chunk ac's hi image for
        // aj = 0, its lo image for aj = 2; the rows nobody reads (aj = 1, 3) fetch chunk ac ^ 1 so that the lanes of a row quartet
        // read four different pieces
        const int ac = (lane & 15) >> 2, aj = lane & 3;
        int moff[KBS];
#pragma unroll
        for (int i = 0; i < KBS; i++) moff[i] = (aj >> 1) * IMG + 64 * ((w + i) % KBS) + 4 * slot(g, ac ^ (aj & 1));
        const int wd = 64 * w + 4 * slot(nn >> 2, cn) + (nn & 3);                               // my packed pair, in dwords
        const int n0 = 32 * w + nn;                                                             // my neuron of tile 2w (+16: 2w+1)
        const int voff = 4 * slot(nn >> 2, cn) + (nn & 3);                                      // my element of a vI tile
        // my chunk's rows of h_out (ragged batch: chunk bc is Tc <= T steps long; a reversed scan starts at ITS last step)
        const int bc = b0 + cn;
        const bool live = FULL || bc < B;
        const int Tc = FULL ? T : (lens && live) ? min(max(lens[bc], 1), T) : T;
        const long hstep = (reverse ? -1L : 1L) * (long)B * ldh;
        float *hp = h_out + ((size_t)(reverse ? Tc - 1 : 0) * B + (live ? bc : 0)) * ldh + n0;
        const long zstep = (reverse ? -1L : 1L) * (long)B * 2 * N;
        float *zp = SAVE ? zr_out + ((size_t)(reverse ? Tc - 1 : 0) * B + (live ? bc : 0)) * (2 * N) + n0 : nullptr;

        __syncthreads();                                 // LDS initialised, every wave's invw_lds rows written
        lds_bar();                                       // x operand images of groups 0 and 1 (service leader)
        half8 pxh = {0, 0, 0, 0, 0, 0, 0, 0}, pxl = pxh;    // x operands of the coming step's share of the projection
        settle(pxh);
        settle(pxl);
        if constexpr (CT > 0) {                          // vI of group 0
            half8 xh0[KBLK], xl0[KBLK];
#pragma unroll
            for (int kb = 0; kb < KBLK; kb++) { xh0[kb] = ldH(xop_hi, poff + 64 * kb); xl0[kb] = ldH(xop_lo, poff + 64 * kb); }
#pragma unroll
            for (int t = 0; t < CT; t++) {
                pacc[t] = tile_mfma_acc<KBLK>(pw_hi[t], pw_lo[t], xh0, xl0);
                mfma_drain(pacc[t]);
                proj_out(w * CT + t, pacc[t], 0);
            }
            if constexpr (!LATE) {
                pxh = ldH(xop_hi, OPIMG + poff);         // step 0 projects K block 0 of group 1
                pxl = ldH(xop_lo, OPIMG + poff);
            }
        }
        lds_bar();                                       // vI of group 0 complete

        [[maybe_unused]] unsigned long long sacc[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, tprev = 0;
        if constexpr (DIAG) { asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(tprev)::"memory"); }
        float hold[2] = {0.0f, 0.0f};
        [[maybe_unused]] float zkeep[2] = {0.0f, 0.0f};  // SAVE: the update gate of the step before, stored with its h
        auto store_h = [&]() {                           // `hold` to its row (ABL 16384: the first of the two stores only)
            hp[0] = hold[0];
            if constexpr (!(ABL & 16384)) hp[16] = hold[1];
        };
        // carried from step to step: my own K block of h(s-1) as A operand, read back right after I wrote it
        half8 oh = {0, 0, 0, 0, 0, 0, 0, 0};
        settle(oh);
        // registers the asm statements of a step write, kept from step to step (bar16_common.h: pick_sum_kept)
        float pk0 = 0.0f, pk1 = 0.0f;
        unsigned sp_hi = 0u, sp_lo = 0u;
        // One step = two intervals, each opened by a barrier; MFMAs are issued in an order that keeps the matrix pipe busy
        // through every LDS round trip and every stretch of gate arithmetic (an MFMA occupies the pipe for 16 cycles and
        // the issuing wave for 4):
        //   A  [others' h(s-1) visible]  request the other K blocks; r and z products with my own block (already in registers: they
        //      wait for nothing) while those fly, and in the products' shadow the store of h(s-1), the pointer bumps, the requests
        //      of vI(s) and of the x operands of this step's share of the projection (HEAD below; HEAD 0: all of that in front of
        //      the first product); r products with the others, tile 0 first; sigmoid(r), r*h, split, write, own block read back;
        //      ALL z products somewhere in this interval (NB_S, NB_E below); this step's share of the projection behind the write
        //      (LATE; otherwise in the round trip at the start)
        //   B  [others' r*h visible]     request the other K blocks (not LATE: then the x operands of the next step's share of the
        //      projection); candidate products with my own block; candidate products with the others (tile 0 first) with the
        //      picks of z, sigmoid(z), 1 - z and z*h among them, one MFMA to two vector instructions (ZEPI below; ZEPI 0: as one
        //      block in front of them, while the others' r*h flies); tanh, blend, split, write, own block read back, store
        // The gate arithmetic reads the accumulators from inline asm (pick_sum_kept), where hipcc inserts no wait states, and the
        // hardware does not interlock a vector read of an MFMA result: seven wait states must lie between a
        // v_mfma_f32_16x16x32_f16 and the read (tools/probes/mfma_read_hazard_probe.hip).  Every tile's last MFMA is therefore
        // pinned (sched_barrier) in front of at least eight wait states of other instructions: tile 1's MFMAs for tile 0 --
        // which also hides their latency behind tile 0's arithmetic -- and tile 0's pick for tile 1.
        auto mfma2 = [](const half8 &w_hi, const half8 &w_lo, const half8 &am, f32x4 &acc) {
            if constexpr (ABL & 2) {
                half8 a = w_hi, b = am;
                asm volatile("" : "+v"(a), "+v"(b), "+v"(acc));
            } else {
                ::mfma2t(am, w_hi, w_lo, acc);
            }
        };
        // wait states in front of tile 0's pick when 2 (KBS - 1) MFMAs of tile 1 (at least two: its own block) follow tile 0's last
        constexpr int WS0 = KBS > 1 ? (8 - 2 * (KBS - 1) > 1 ? 8 - 2 * (KBS - 1) : 1) : 6;
        constexpr int WS1 = (8 - WS0 - 1) > 1 ? (8 - WS0 - 1) : 1;         // ... of tile 1's, behind tile 0's pick (WS0 + one read)
        // Where a step issues the z products (design/gru_zgate.md; every placement gives each accumulator the same MFMAs in the same
        // order, own block first).  All of them lie in interval A, so that sigmoid(z) can be formed in interval B while the other
        // blocks of r*h are on their way from LDS, not between the candidate's MFMAs and its pick:
        //   blocks 0 .. NB_S-1     in the LDS round trip at the start of A (the own block is in registers);
        //   blocks NB_S .. NB_E-1  under the r epilogue, one MFMA to three vector instructions;
        //   blocks NB_E .. KBS-1   behind the write of r*h, where the wave only waits for its writes and for barrier B.
        // Three K blocks: own block at the start, the others under the epilogue -- twelve MFMAs behind the write keep the matrix pipe
        // busy past barrier B.  Two K blocks (the 64-wide layers): all eight behind the write; the measured best of five placements each.
        constexpr int NB_S = KBS == 2 ? 0 : 1, NB_E = KBS == 2 ? 0 : KBS;
        // What stands between barrier A and the first MFMA, and how the z epilogue shares interval B with the candidate's products
        // (design/gru_step_order.md).  The own-block products wait for nothing but `oh`, which the wave read back before the barrier:
        //   HEAD 0  state requests, store of h(s-1), pointer bumps, vI(s) and x-operand requests, THEN the own-block r and z products;
        //   HEAD 1  state requests, own-block r and z products, then stores, bumps and requests in the products' shadow;
        //   HEAD 2  state requests, vI(s) and x-operand requests, own-block products, then stores and bumps;
        //   ZEPI 0  sigmoid(z), 1 - z, z*h as one block between the candidate's own-block products and those of the other blocks;
        //   ZEPI 1  among the other blocks' products, one MFMA to two vector instructions.
        // Measured per instantiation (the note's section 2; the variants not kept: tools/experiments/gru_step_order_variants.patch.txt):
        // the layers whose chain waves project behind the write (LATE) take ZEPI 1, and HEAD 1 inside the stack kernel, HEAD 2 as a
        // launch of their own.  The 64-wide layers have four other-block candidate MFMAs, too few to hide an epilogue under, and four K
        // blocks of input keep the projection in the round trip the head would give to the own-block products: both stay at 0.
        constexpr int HEAD = LATE ? (PACKED ? 1 : 2) : 0;
        constexpr int ZEPI = LATE ? 1 : 0;
        constexpr bool NOHEAD = (ABL & 2048) != 0;       // diagnostic: no stores, no vI or x-operand requests (constants instead)
        auto step = [&](auto PHC, const int s, const int G) {
            constexpr int ph = decltype(PHC)::value;
            constexpr bool PROJ = CT > 0 && ph < KBLK && !(ABL & 128);
            // ------------------------------ interval A ------------------------------
            if constexpr (DIAG) lds_bar(); else lds_bar_1read<!(ABL & 1)>();
            BSTAMP(0)
            half8 bh[KBS];
            bh[0] = oh;
#pragma unroll
            for (int i = 1; i < KBS; i++) bh[i] = ldH(h_img, moff[i]);       // what the step waits for is requested first
            __builtin_amdgcn_sched_barrier(0);
            float vz[2], vr[2], vc[2];
            [[maybe_unused]] auto put_h = [&]() {        // h(s-1): still in `hold`
                if (FULL ? (ph > 0 || s > 0) : s > 0) {  // (FULL: a fact in phases 1 to 3, a test of the group counter in phase 0)
                    if constexpr (FULL) {
                        if constexpr (!(ABL & 16) && !NOHEAD) store_h();
                    } else if constexpr (ABL & 4096) {   // diagnostic: the predicate and its branch around nothing
                        if (live && s - 1 < Tc) asm volatile("" ::"v"(hold[0]), "v"(hold[1]), "v"(hp));
                    } else if ((ABL & 8192) || (live && s - 1 < Tc && !(ABL & 16) && !NOHEAD)) {
                        store_h();
                        if constexpr (SAVE) { zp[0] = zkeep[0]; zp[16] = zkeep[1]; }
                    }
                    if constexpr (!(ABL & 32768)) hp += hstep;           // (diagnostic: a row that never moves)
                    if constexpr (SAVE) zp += zstep;
                }
            };
            // vI(s): complete since the previous barrier at the latest (the service waves use every interval); never asked for in
            // front of barrier A -- vI(4G) is only complete there
            [[maybe_unused]] auto ask_v = [&]() {
                if constexpr (NOHEAD) {
                    vz[0] = vz[1] = vr[0] = vr[1] = vc[0] = vc[1] = 0.125f;
                } else {
                    const float *vcur = vbuf + (s % R) * VSTEP + voff;
#pragma unroll
                    for (int p = 0; p < 2; p++) {
                        vr[p] = vcur[64 * (NT + 2 * w + p)];
                        vz[p] = vcur[64 * (2 * w + p)];
                        vc[p] = vcur[64 * (2 * NT + 2 * w + p)];
                    }
                    if constexpr (LATE && PROJ) {        // x operands of my share, K block ph of group G+1 (split a group ago): behind h and vI
                        const int ob = ((G + 1) & 1) * OPIMG + poff + 64 * ph;
                        pxh = ldH(xop_hi, ob);
                        pxl = ldH(xop_lo, ob);
                    }
                }
            };
            if constexpr (HEAD == 0) {
                put_h();
                __builtin_amdgcn_sched_barrier(0);
                ask_v();
                __builtin_amdgcn_sched_barrier(0);
            } else if constexpr (HEAD == 2) {
                ask_v();
                __builtin_amdgcn_sched_barrier(0);
            }
            BSTAMP(8)
            f32x4 accR[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
            mfma2(wr_hi[0][0], wr_lo[0][0], bh[0], accR[0]);
            mfma2(wr_hi[1][0], wr_lo[1][0], bh[0], accR[1]);
            if constexpr (PROJ && !LATE) {              // my tile of the projection, K block ph: inside the LDS round trip
                if constexpr (!(ABL & 2)) {
#pragma unroll
                    for (int t = 0; t < CT; t++) block_mfma_acc<ph == 0>(pacc[t], pw_hi[t][ph], pw_lo[t][ph], pxh, pxl);
                }
            }
            if constexpr (CT > 0 && ph == 3 && !(ABL & 128)) {   // vI of group G+1 (its last MFMAs were issued a step ago unless KBLK = 4)
#pragma unroll
                for (int t = 0; t < CT; t++) {
                    if constexpr (KBLK == 4) mfma_drain(pacc[t]);
                    proj_out(w * CT + t, pacc[t], G + 1);
                }
            }
            f32x4 accZ[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
            if constexpr (!(ABL & 64)) {
#pragma unroll
                for (int i = 0; i < NB_S; i++) {
                    mfma2(wz_hi[0][i], wz_lo[0][i], bh[i], accZ[0]);
                    mfma2(wz_hi[1][i], wz_lo[1][i], bh[i], accZ[1]);
                }
            }
            if constexpr (HEAD != 0) {
                // the own-block products in front of everything below (the statements hand the accumulators on: see the r products)
                asm volatile("" : "+v"(accR[0]), "+v"(accR[1]));
                if constexpr (NB_S > 0 && !(ABL & 64)) asm volatile("" : "+v"(accZ[0]), "+v"(accZ[1]));
                __builtin_amdgcn_sched_barrier(0);
                put_h();
                if constexpr (HEAD == 1) {
                    __builtin_amdgcn_sched_barrier(0);
                    ask_v();
                }
            }
            __builtin_amdgcn_sched_barrier(0);
            BSTAMP(1)
#pragma unroll
            for (int i = 1; i < KBS; i++) mfma2(wr_hi[0][i], wr_lo[0][i], bh[i], accR[0]);
            // tile 0 complete BEFORE tile 1's remaining MFMAs are issued (WS0 counts on them).  Instruction selection places an MFMA
            // anywhere its operands allow, sched_barrier or not; these statements (volatile: they keep their order) hand the
            // accumulators on, so the MFMAs in front of one and behind the next cannot change sides.
            asm volatile("" : "+v"(accR[0]));
            asm volatile("" : "+v"(accR[1]));
#pragma unroll
            for (int i = 1; i < KBS; i++) mfma2(wr_hi[1][i], wr_lo[1][i], bh[i], accR[1]);
            asm volatile("" : "+v"(accR[1]));
            if constexpr (NB_E > NB_S && !(ABL & 64)) asm volatile("" : "+v"(accZ[0]), "+v"(accZ[1]));   // the z products: behind the r products
            __builtin_amdgcn_sched_barrier(0);
            BSTAMP(2)
            if constexpr (!(ABL & 64)) {
#pragma unroll
                for (int i = NB_S; i < NB_E; i++) {
                    mfma2(wz_hi[0][i], wz_lo[0][i], bh[i], accZ[0]);
                    mfma2(wz_hi[1][i], wz_lo[1][i], bh[i], accZ[1]);
                }
            }
            float rr[2];
            pick_sum_kept<WS0>(accR[0], pk0, accR[1][0]);                     // behind tile 1's MFMAs
            pick_sum_kept<WS1>(accR[1], pk1, pk0);                            // behind tile 0's pick
            rr[0] = (ABL & 4) ? fmaf(pk0, inv_r[0], vr[0]) * 0.01f : sigmoid4(fmaf(pk0, inv_r[0], vr[0]));
            rr[1] = (ABL & 4) ? fmaf(pk1, inv_r[1], vr[1]) * 0.01f : sigmoid4(fmaf(pk1, inv_r[1], vr[1]));
            split2_kept(rr[0] * hold[0], rr[1] * hold[1], sp_hi, sp_lo);
            lds_fence();
            rh_hi[wd] = sp_hi;
            rh_lo[wd] = sp_lo;
            // the accumulators stay allocated until here: a value that moved into their registers right behind the picks would
            // make the compiler pad for the MFMAs it knows wrote them (it counts an asm statement as one wait state)
            asm volatile("" ::"v"(accR[0]), "v"(accR[1]));
            half8 ch[KBS];
            ch[0] = ldH(rh_img, moff[0]);                // my own block, straight back (LDS executes a wave's operations in order)
            lds_fence();
            // one MFMA, then up to three VALU instructions, for as long as both last
#pragma unroll
            for (int i = 0; i < 4 * (NB_E - NB_S); i++) {
                __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                __builtin_amdgcn_sched_group_barrier(0x002, 3, 0);
            }
            __builtin_amdgcn_sched_barrier(0);
            // the z products behind the write: the operand statement keeps them there (volatile statements keep their order, the MFMAs
            // need its result), the accumulator statement in front of the barrier
            if constexpr (!(ABL & 64) && KBS > NB_E) {
                asm volatile("" : "+v"(bh[NB_E]));
#pragma unroll
                for (int i = NB_E; i < KBS; i++) {
                    mfma2(wz_hi[0][i], wz_lo[0][i], bh[i], accZ[0]);
                    mfma2(wz_hi[1][i], wz_lo[1][i], bh[i], accZ[1]);
                }
                asm volatile("" : "+v"(accZ[0]), "+v"(accZ[1]));
            }
            // my share of the projection, K block ph: asm statements, so they stay behind the fence above and in front of the barrier
            if constexpr (PROJ && LATE && !(ABL & 2)) {
#pragma unroll
                for (int t = 0; t < CT; t++) block_mfma_acc<ph == 0>(pacc[t], pw_hi[t][ph], pw_lo[t][ph], pxh, pxl);
            }
            const bool store = live && s < Tc && !(ABL & 16);
            // ------------------------------ interval B ------------------------------
            if constexpr (DIAG) { BSTAMP(3) lds_bar(); } else lds_bar_1read<!(ABL & 1)>();
            BSTAMP(4)
#pragma unroll
            for (int i = 1; i < KBS; i++) ch[i] = ldH(rh_img, moff[i]);
            __builtin_amdgcn_sched_barrier(0);
            if constexpr (SAVE) {                        // (behind the barrier, like h: while the requested operands are on their way)
                if (store) { zp[N] = rr[0]; zp[N + 16] = rr[1]; }
                __builtin_amdgcn_sched_barrier(0);
            }
            constexpr int nph = (ph + 1) & 3;            // the next step projects K block nph of the group after ITS group
            constexpr bool NPROJ = CT > 0 && nph < KBLK && !(ABL & 128) && !LATE;
            if constexpr (NPROJ) {
                const int ob = ((G + (ph == 3 ? 2 : 1)) & 1) * OPIMG + poff + 64 * nph;
                pxh = ldH(xop_hi, ob);
                pxl = ldH(xop_lo, ob);
            }
            __builtin_amdgcn_sched_barrier(0);
            f32x4 accC[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
            mfma2(wc_hi[0][0], wc_lo[0][0], ch[0], accC[0]);
            mfma2(wc_hi[1][0], wc_lo[1][0], ch[0], accC[1]);
            // everything below -- sigmoid(z) and the other blocks' candidate products -- behind these four MFMAs
            asm volatile("" : "+v"(accC[0]), "+v"(accC[1]));
            __builtin_amdgcn_sched_barrier(0);
            if constexpr (ZEPI != 0) { BSTAMP(5) }                            // (a stamp is a fence: not between the epilogue and its MFMAs)
            float zz[2], omz[2], zh[2];
            if constexpr (ABL & (64 | 1024)) {                              // no update gate (1024: its products stay): the blend takes constants
                zz[0] = zz[1] = omz[0] = omz[1] = 0.5f;
                zh[0] = zh[1] = 0.25f;
            } else if constexpr (ZEPI != 0) {
                // the same picks and the same two chains, side by side, but no fence behind them: they are spread among the other
                // blocks' products below
                pick_sum_kept<1>(accZ[0], pk0, accC[1][0]);
                pick_sum_kept<1>(accZ[1], pk1, accC[1][0]);
                zz[0] = (ABL & 4) ? fmaf(pk0, inv_z[0], vz[0]) * 0.01f : sigmoid4(fmaf(pk0, inv_z[0], vz[0]));
                zz[1] = (ABL & 4) ? fmaf(pk1, inv_z[1], vz[1]) * 0.01f : sigmoid4(fmaf(pk1, inv_z[1], vz[1]));
#pragma unroll
                for (int p = 0; p < 2; p++) { omz[p] = 1.0f - zz[p]; zh[p] = zz[p] * hold[p]; }
            } else {
                // sigmoid(z) while the other blocks of r*h are on their way from LDS.  `after` keeps the picks behind the candidate's four
                // own-block MFMAs, and those behind barrier B.  The z MFMAs behind the write are pinned in front of the barrier; the
                // last ones under the r epilogue may trail past it (nothing pins a builtin MFMA), and then still have two LDS reads
                // and the four MFMAs between them and the pick -- and hipcc, which placed them and sees the accumulator among the
                // operands of the pick's asm, pads what it finds missing (tests/test_isa_hygiene.py scans the outcome).
                pick_sum_kept<1>(accZ[0], pk0, accC[1][0]);
                pick_sum_kept<1>(accZ[1], pk1, accC[1][0]);
                zz[0] = (ABL & 4) ? fmaf(pk0, inv_z[0], vz[0]) * 0.01f : sigmoid4(fmaf(pk0, inv_z[0], vz[0]));
                zz[1] = (ABL & 4) ? fmaf(pk1, inv_z[1], vz[1]) * 0.01f : sigmoid4(fmaf(pk1, inv_z[1], vz[1]));
#pragma unroll
                for (int p = 0; p < 2; p++) { omz[p] = 1.0f - zz[p]; zh[p] = zz[p] * hold[p]; }
                asm volatile("" : "+v"(zh[0]), "+v"(omz[0]), "+v"(zh[1]), "+v"(omz[1]), "+v"(pk0), "+v"(pk1));
                __builtin_amdgcn_sched_barrier(0);
            }
            if constexpr (ZEPI == 0) { BSTAMP(5) }
#pragma unroll
            for (int i = 1; i < KBS; i++) mfma2(wc_hi[0][i], wc_lo[0][i], ch[i], accC[0]);
            asm volatile("" : "+v"(accC[0]));                                // as above: tile 0's sum before tile 1's
            asm volatile("" : "+v"(accC[1]));
#pragma unroll
            for (int i = 1; i < KBS; i++) mfma2(wc_hi[1][i], wc_lo[1][i], ch[i], accC[1]);
            asm volatile("" : "+v"(accC[1]));
            if constexpr (ZEPI != 0 && !(ABL & (64 | 1024))) {
                // one MFMA, then two of the z epilogue's vector instructions, for as long as both last: the wave issues for 4 of the 16
                // cycles an MFMA keeps the pipe
#pragma unroll
                for (int i = 0; i < 4 * (KBS - 1); i++) {
                    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                    __builtin_amdgcn_sched_group_barrier(0x002, 2, 0);
                }
            }
            __builtin_amdgcn_sched_barrier(0);
            if constexpr (ZEPI != 0 && !(ABL & (64 | 1024))) {
                // (behind the products: in front of them it would be a fence for the epilogue)
                asm volatile("" : "+v"(zh[0]), "+v"(omz[0]), "+v"(zh[1]), "+v"(omz[1]), "+v"(pk0), "+v"(pk1));
                __builtin_amdgcn_sched_barrier(0);
            }
            BSTAMP(6)
            float hn[2];
            {
                pick_sum_kept<WS0>(accC[0], pk0, accC[1][0]);
                pick_sum_kept<WS1>(accC[1], pk1, pk0);
                const float h0 = (ABL & 4) ? fmaf(pk0, inv_c[0], vc[0]) * 0.01f : tanh5(fmaf(pk0, inv_c[0], vc[0]));
                const float h1 = (ABL & 4) ? fmaf(pk1, inv_c[1], vc[1]) * 0.01f : tanh5(fmaf(pk1, inv_c[1], vc[1]));
                hn[0] = fmaf(omz[0], h0, zh[0]);                              // layers.py:1020
                hn[1] = fmaf(omz[1], h1, zh[1]);
            }
            split2_kept(hn[0], hn[1], sp_hi, sp_lo);
            lds_fence();
            h_hi[wd] = sp_hi;
            h_lo[wd] = sp_lo;
            asm volatile("" ::"v"(accC[0]), "v"(accC[1]), "v"(accZ[0]), "v"(accZ[1]));
            oh = ldH(h_img, moff[0]);
            lds_fence();
            // (h(s) is stored by the NEXT step, behind its first barrier, while that step waits for the state it has requested from LDS;
            //  here the stores were two more instructions between the last write of the state and the barrier everybody waits at)
            if constexpr (SAVE) {
                zkeep[0] = zz[0];
                zkeep[1] = zz[1];
            }
#pragma unroll
            for (int p = 0; p < 2; p++) hold[p] = hn[p];
            BSTAMP(7)
        };
        for (int G = 0; G < NG; G++) {
            const int s = GS * G;
            step(ic<0>{}, s, G);
            if (s + 1 < T) step(ic<1>{}, s + 1, G);
            if (s + 2 < T) step(ic<2>{}, s + 2, G);
            if (s + 3 < T) step(ic<3>{}, s + 3, G);
        }
        if (!(ABL & 16) && (FULL || (live && T - 1 < Tc))) {         // h (and z) of the last step
            store_h();
            if constexpr (SAVE) { zp[0] = zkeep[0]; zp[16] = zkeep[1]; }
        }
#ifdef SLK_DIAG
        if constexpr (DIAG) {
            if (blockIdx.x == 0 && lane == 0)
                for (int i = 0; i < 16; i++) slk_dbg_bar16[wave][i] = sacc[i];
        }
        if constexpr (ABL & 32) {
            unsigned long long t1, r1;
            unsigned hwid, xcc;
            asm volatile("s_memtime %0\n\ts_memrealtime %1\n\ts_getreg_b32 %2, hwreg(HW_REG_HW_ID)\n\ts_getreg_b32 %3, hwreg(HW_REG_XCC_ID)\n\ts_waitcnt lgkmcnt(0)"
                         : "=s"(t1), "=s"(r1), "=s"(hwid), "=s"(xcc)::"memory");
            if (wave == 0 && lane == 0 && blockIdx.x < 1024) {
                slk_dbg_bar16_wg[blockIdx.x][0] = t1 - wg_t0;
                slk_dbg_bar16_wg[blockIdx.x][1] = r1 - wg_r0;
                slk_dbg_bar16_wg[blockIdx.x][2] = ((unsigned long long)xcc << 32) | hwid;
                slk_dbg_bar16_wg[blockIdx.x][3] = wg_r0;
            }
        }
#endif
    } else {
        // =================================================================================================
        // service waves: the rest of the projection; the leader (first of them) also runs the x DMA and splits x
        // =================================================================================================
        const int sw = wave - NCW;
        const bool leader = sw == 0;
        const int tile0 = NCW * CT + sw * ST;
        constexpr int NV = ST - NA > 0 ? ST - NA : 1;
        half8 pa_hi[NA][KBLK], pa_lo[NA][KBLK];          // tiles 0..NA-1: accumulation registers
        half8 pw_hi[NV][KBLK], pw_lo[NV][KBLK];          // the rest: ordinary registers
        // (PACKED: the images arrive in ordinary registers and move on from there; four tiles' loads in flight at a time, not all of them)
        constexpr int LB = PACKED ? 4 : 1;
#pragma unroll
        for (int t0 = 0; t0 < NA; t0 += LB) {
#pragma unroll
            for (int t = t0; t < t0 + LB && t < NA; t++) load_tile(tile0 + t, pa_hi[t], pa_lo[t]);
#pragma unroll
            for (int t = t0; t < t0 + LB && t < NA; t++) {
#pragma unroll
                for (int kb = 0; kb < KBLK; kb++) { pa_hi[t][kb] = to_acc_regs(pa_hi[t][kb]); pa_lo[t][kb] = to_acc_regs(pa_lo[t][kb]); }
            }
            if constexpr (PACKED) __builtin_amdgcn_sched_barrier(0);
        }
#pragma unroll
        for (int t = NA; t < ST; t++) load_tile(tile0 + t, pw_hi[t - NA], pw_lo[t - NA]);

        // x of a group: the leader's lane (row pcol = (step, chunk), k group kg) loads ITS eight floats of every K block straight
        // into registers (the four lanes of a row and K block cover one 128-byte line) a group ahead of the split -- no staging
        // in LDS, no LDS-DMA (a 1-KiB request kept the issuing wave ~150 cycles, twelve of sixteen intervals carried one).
        // Ordinary loads: the compiler waits for them where the split first uses them, a group later.
        const int xbc = FULL ? b0 + pc : min(b0 + pc, B - 1);
        const int xTc = FULL ? T : lens ? min(max(lens[xbc], 1), T) : T;
        f32x4 xr[KBLK][2];
        auto load_x = [&](int G2) {
            // steps past the chunk's end re-read its last valid row (their results are never stored)
            const int ss = min(G2 * GS + pstep, xTc - 1);
            const int tt = reverse ? xTc - 1 - ss : ss;
            const float *row = x + ((size_t)tt * B + xbc) * ldx;
#pragma unroll
            for (int kb = 0; kb < KBLK; kb++) {
                const int k0 = 32 * kb + 8 * kg;
                const bool kok = (I % 32 == 0) || k0 < I;
                const float *src = row + (kok ? k0 : 0);
                xr[kb][0] = *reinterpret_cast<const f32x4 *>(src);
                xr[kb][1] = *reinterpret_cast<const f32x4 *>(src + 4);
            }
        };
        float xs = 1.0f;
        float raw[KBLK][8];                              // the group's rows as read for the scale, kept for the split
        auto split_scale = [&](int G2) {                 // pass 1: the row's power-of-two scale
            float amax = 0.0f;
#pragma unroll
            for (int kb = 0; kb < KBLK; kb++) {
                const int k0 = 32 * kb + 8 * kg;
                const bool kok = (I % 32 == 0) || k0 < I;
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    raw[kb][j] = kok ? xr[kb][0][j] : 0.0f;
                    raw[kb][4 + j] = kok ? xr[kb][1][j] : 0.0f;
                    amax = fmaxf(amax, fmaxf(fabsf(raw[kb][j]), fabsf(raw[kb][4 + j])));
                }
            }
            float xinv;
            xs = pow2_scale(kgroup_max(amax), xinv);
            if (kg == 0) xinv_lds[(G2 & 1) * 16 + pcol] = xinv;
        };
        auto split_block = [&](int G2, int kb) {         // pass 2: K block kb -> operand images
            unsigned ahi[4], alo[4];
#pragma unroll
            for (int j = 0; j < 4; j++) split2(raw[kb][2 * j] * xs, raw[kb][2 * j + 1] * xs, ahi[j], alo[j]);
            const int ob = (G2 & 1) * OPIMG + poff + 64 * kb;
            *reinterpret_cast<uint4 *>(xop_hi + ob) = make_uint4(ahi[0], ahi[1], ahi[2], ahi[3]);
            *reinterpret_cast<uint4 *>(xop_lo + ob) = make_uint4(alo[0], alo[1], alo[2], alo[3]);
        };

        __syncthreads();
        if (leader) {
            for (int G2 = 0; G2 < 2; G2++) {
                load_x(G2);
                split_scale(G2);
#pragma unroll
                for (int kb = 0; kb < KBLK; kb++) split_block(G2, kb);
            }
            load_x(2);                                   // group 2: split during group 0
        }
        lds_bar();
        half8 xh[KBLK], xl[KBLK];
        auto load_operands = [&](int G1) {
#pragma unroll
            for (int kb = 0; kb < KBLK; kb++) {
                const int ob = (G1 & 1) * OPIMG + poff + 64 * kb;
                xh[kb] = ldH(xop_hi, ob);
                xl[kb] = ldH(xop_lo, ob);
            }
        };
        // accumulator of one tile (no drain): accumulation-register weights through asm, the rest through the builtin
        auto tile_acc = [&](auto TC) {
            constexpr int t = decltype(TC)::value;
            if constexpr (t < NA) {
                return tile_mfma_acc<KBLK>(pa_hi[t], pa_lo[t], xh, xl);
            } else {
                f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int kb = 0; kb < KBLK; kb++) acc = mfma3(pw_hi[t - NA][kb], pw_lo[t - NA][kb], xh[kb], xl[kb], acc);
                return acc;
            }
        };
        // two tiles: their output constants are requested first, then all MFMAs (the matrix pipe stays busy through the LDS
        // round trip), one drain, then the outputs
        auto project_tiles = [&](auto T0, auto T1, int G1) {
            constexpr int t0 = decltype(T0)::value, t1 = decltype(T1)::value;
            const float xin = xinv_lds[(G1 & 1) * 16 + pcol];
            f32x4 iw0, bs0, iw1, bs1;
            iw0 = *reinterpret_cast<const f32x4 *>(&invw_lds[16 * (tile0 + t0) + 4 * kg]);
            bs0 = *reinterpret_cast<const f32x4 *>(&bias_lds[16 * (tile0 + t0) + 4 * kg]);
            if constexpr (t1 < ST) {
                iw1 = *reinterpret_cast<const f32x4 *>(&invw_lds[16 * (tile0 + t1) + 4 * kg]);
                bs1 = *reinterpret_cast<const f32x4 *>(&bias_lds[16 * (tile0 + t1) + 4 * kg]);
            }
            f32x4 a0 = tile_acc(T0), a1 = {0.f, 0.f, 0.f, 0.f};
            if constexpr (t1 < ST) a1 = tile_acc(ic<t1 < ST ? t1 : 0>{});
            mfma_drain2(a0, a1);
            const int st = GS * G1 + pstep;
            float *dst = &vbuf[(st % R) * VSTEP + 4 * slot(kg, pc)];
            f32x4 o;
#pragma unroll
            for (int r = 0; r < 4; r++) o[r] = fmaf(a0[r] * xin, iw0[r], bs0[r]);
            *reinterpret_cast<f32x4 *>(dst + 64 * (tile0 + t0)) = o;
            if constexpr (t1 < ST) {
#pragma unroll
                for (int r = 0; r < 4; r++) o[r] = fmaf(a1[r] * xin, iw1[r], bs1[r]);
                *reinterpret_cast<f32x4 *>(dst + 64 * (tile0 + t1)) = o;
            }
        };
        // which tiles an interval computes: the leader's intervals 1-3 carry the x split, so they get fewer
        auto project_interval = [&](auto KC, int G1) {
            constexpr int k = decltype(KC)::value;
            constexpr int lo = bar16_tile_first(ST, k, BAR16_TILE_W[TBL], 8), hi = bar16_tile_first(ST, k + 1, BAR16_TILE_W[TBL], 8);
            static_assert(hi - lo <= 3, "at most three tiles per interval");
            if constexpr (hi - lo == 1) project_tiles(ic<lo>{}, ic<ST>{}, G1);
            if constexpr (hi - lo == 2) project_tiles(ic<lo>{}, ic<lo + 1>{}, G1);
            if constexpr (hi - lo == 3) { project_tiles(ic<lo>{}, ic<lo + 1>{}, G1); project_tiles(ic<lo + 2>{}, ic<ST>{}, G1); }
        };
        load_operands(0);
        static_for<0, 8>([&](auto KC) { project_interval(KC, 0); });
        lds_bar();                                       // vI of group 0 complete

        // interval k = 0..7 of group G (two per step, each opened by the barrier the chain waves open theirs with)
        [[maybe_unused]] unsigned long long sacc[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, tprev = 0;
        if constexpr (DIAG) { asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(tprev)::"memory"); }
        auto interval = [&](auto KC, const int G) {
            constexpr int k = decltype(KC)::value;
            lds_bar<!(ABL & 1)>();
            BSTAMP(8 + k)
            if constexpr (ABL & 8) return;
            if constexpr (k == 0) load_operands(G + 1);
            project_interval(KC, G + 1);
            if constexpr (tile_extra(ABL, k) > 0) {      // ablation: one tile of this interval once more (same value, same place)
                constexpr int lo = bar16_tile_first(ST, k, BAR16_TILE_W[TBL], 8);
                project_tiles(ic<(lo < NA ? lo : NA - 1)>{}, ic<ST>{}, G + 1);
            }
            if (leader) {
                if constexpr (k == 1) split_scale(G + 2);
                if constexpr (k >= 2 && k < 2 + KBLK) split_block(G + 2, k - 2);
                if constexpr (k == 1 + KBLK) load_x(G + 3);
            }
            BSTAMP(k)
        };
        for (int G = 0; G < NG; G++) {
            const int s = GS * G;
            interval(ic<0>{}, G); interval(ic<1>{}, G);
            if (s + 1 < T) { interval(ic<2>{}, G); interval(ic<3>{}, G); }
            if (s + 2 < T) { interval(ic<4>{}, G); interval(ic<5>{}, G); }
            if (s + 3 < T) { interval(ic<6>{}, G); interval(ic<7>{}, G); }
        }
#ifdef SLK_DIAG
        if constexpr (DIAG) {
            if (blockIdx.x == 0 && lane == 0)
                for (int i = 0; i < 16; i++) slk_dbg_bar16[wave][i] = sacc[i];
        }
#endif
    }
