// bar16_proj_image.h -- THE statements that turn one 16-row tile of iW into the projection's A operands: the lane's row is scaled by a
// power of two to [1, 2) and split into fp16 hi / lo halves (lane: row pcol of the tile, k = 32 kb + 8 kg + 0..7).  Text, not a function
// (design/gru_prologue.md): included where the images are made -- the load_tile lambdas of gru_bar16_body.h, gru_bar16d.hip and
// gru_bar16q.hip, and bar16_proj_tile (bar16_common.h) for gru_bar16_pack_kernel -- so that a pack holds the bits a prologue makes.
// All 64 lanes of the wave execute it (kgroup_max swaps across lanes).
// In scope where it is included: I, KBLK (constants); iW, tile, pcol, kg; half8 hi[KBLK], lo[KBLK] to fill; and the macro
// BAR16_PROJ_INV(row, inv), the site's statement for the row's inverse scale, which stands between the scale and the conversion.
// Declares row, u, m, inv, ws in the scope that includes it.
const int row = 16 * tile + pcol;
float u[KBLK][8];
float m = 0.0f;
#pragma unroll
for (int kb = 0; kb < KBLK; kb++) {
    const int k0 = 32 * kb + 8 * kg;
    const bool kok = (I % 32 == 0) || k0 < I;
    const float *src = iW + (size_t)row * I + (kok ? k0 : 0);
    const float4 u0 = *reinterpret_cast<const float4 *>(src), u1 = *reinterpret_cast<const float4 *>(src + 4);
    const float t[8] = {u0.x, u0.y, u0.z, u0.w, u1.x, u1.y, u1.z, u1.w};
#pragma unroll
    for (int j = 0; j < 8; j++) {
        u[kb][j] = kok ? t[j] : 0.0f;
        m = fmaxf(m, fabsf(u[kb][j]));
    }
}
float inv;
const float ws = pow2_scale(kgroup_max(m), inv);
BAR16_PROJ_INV(row, inv)
#pragma unroll
for (int kb = 0; kb < KBLK; kb++) {
#pragma unroll
    for (int j = 0; j < 8; j++) {
        const float v = u[kb][j] * ws;
        const _Float16 h = (_Float16)v;
        hi[kb][j] = h;
        lo[kb][j] = (_Float16)(v - (float)h);
    }
}
