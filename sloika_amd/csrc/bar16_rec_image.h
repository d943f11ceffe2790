// bar16_rec_image.h -- THE statements that make the recurrent operands of chain wave w for tile p of its two: per gate (z, r from sW,
// the candidate from sW2) the lane's row, scaled by a power of two to [1, 2) and split into fp16 hi / lo halves.  Column lane & 15 is the
// neuron, g = lane >> 4 the k group; K blocks in the rotated order w, w+1, ... (element (g, j) of block kb is neuron
// 32 kb + 16 (j&1) + 4 g + (j>>1), the order the owners' packed writes create).  Text, not a function (design/gru_prologue.md):
// included in the `for p` loops of the prologues of gru_bar16_body.h, gru_bar16d.hip and gru_bar16q.hip, and in bar16_rec_tile
// (bar16_common.h) for gru_bar16_pack_kernel.  All 64 lanes of the wave execute it (kgroup_max swaps across lanes).
// In scope where it is included: N, KBS (constants); sW, sW2, w, p, g, lane; the six arrays wz_hi, wz_lo, wr_hi, wr_lo, wc_hi, wc_lo and
// the macro BAR16_REC_W(a), tile p's half8[KBS] of array a (a[p] in the kernels, which keep both tiles; a in bar16_rec_tile); and the
// macro BAR16_REC_INV(iz, ir, ic_), the site's statement for the rows' inverse scales (every lane of a row has the row's, and its
// neuron IS its row), which stands between the scales and the conversion.
// Declares row, vz, vr, vc, mz, mr, mc, iz, ir, ic_, sz, sr, sc in the scope that includes it.
const int row = 32 * w + 16 * p + (lane & 15);
float vz[KBS][8], vr[KBS][8], vc[KBS][8];
float mz = 0.0f, mr = 0.0f, mc = 0.0f;
#pragma unroll
for (int i = 0; i < KBS; i++) {
    const int kb = (w + i) % KBS;
#pragma unroll
    for (int j = 0; j < 8; j++) {
        const int k = 32 * kb + 16 * (j & 1) + 4 * g + (j >> 1);
        vz[i][j] = sW[(size_t)row * N + k];
        vr[i][j] = sW[(size_t)(N + row) * N + k];
        vc[i][j] = sW2[(size_t)row * N + k];
        mz = fmaxf(mz, fabsf(vz[i][j])); mr = fmaxf(mr, fabsf(vr[i][j])); mc = fmaxf(mc, fabsf(vc[i][j]));
    }
}
float iz, ir, ic_;
const float sz = pow2_scale(kgroup_max(mz), iz), sr = pow2_scale(kgroup_max(mr), ir), sc = pow2_scale(kgroup_max(mc), ic_);
BAR16_REC_INV(iz, ir, ic_)
#pragma unroll
for (int i = 0; i < KBS; i++) {
#pragma unroll
    for (int j = 0; j < 8; j++) {
        const float az = vz[i][j] * sz, ar = vr[i][j] * sr, ac = vc[i][j] * sc;
        const _Float16 hz = (_Float16)az, hr = (_Float16)ar, hc = (_Float16)ac;
        BAR16_REC_W(wz_hi)[i][j] = hz; BAR16_REC_W(wz_lo)[i][j] = (_Float16)(az - (float)hz);
        BAR16_REC_W(wr_hi)[i][j] = hr; BAR16_REC_W(wr_lo)[i][j] = (_Float16)(ar - (float)hr);
        BAR16_REC_W(wc_hi)[i][j] = hc; BAR16_REC_W(wc_lo)[i][j] = (_Float16)(ac - (float)hc);
    }
}
