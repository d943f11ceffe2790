// rescore_common.h -- what rescore_edits.hip (dense lattices) and rescore_band.hip (banded lattices) share: the limits, the order of
// the four wave sums, the shift clamp of the (mantissa, exponent) sums, the staging of a posterior row into LDS and the head of the
// workspace.  Moved here unchanged from rescore_edits.hip (design/rescore_edits.md 3 to 5).
#pragma once
#include "forward_row.h"

#define RE_MAX_STATES 8192
#define RE_CAND 256                                           // candidates per workgroup
#define RE_NAN __longlong_as_double(0x7ff8000000000000LL)

__device__ __forceinline__ double re_sum4(const double *w) { return ((w[0] + w[1]) + w[2]) + w[3]; }

__device__ __forceinline__ int re_clamp_shift(int64_t s) { return (int)(s < -4096 ? -4096 : (s > 4096 ? 4096 : s)); }

// One posterior row on its way into LDS: the row's bytes in 16-byte granules of its own alignment, granule tid + 256 k in r[k].  A
// granule that lies wholly inside the row is one 16-byte load; the row's first and last granule are read value by value, so that
// nothing outside the row is touched.  In LDS value c of the row sits at index c + mis (mis: the row's first value inside its granule).
template <typename T, int NCH>
struct re_stage {
    static constexpr int PER = 16 / sizeof(T);
    uint4 r[NCH];
    __device__ __forceinline__ static int mis(const T *row) { return (int)((reinterpret_cast<uintptr_t>(row) & 15) / sizeof(T)); }
    __device__ __forceinline__ void load(const T *row, int nstate)
    {
        const int ms = mis(row);
        const T *g0 = row - ms;                               // (16-byte aligned; only values inside the row are read)
        const int ngran = (ms + nstate + PER - 1) / PER;
#pragma unroll
        for (int k = 0; k < NCH; k++) {
            const int q = threadIdx.x + FS_THREADS * k;
            if (q >= ngran) continue;
            const int lo = q * PER - ms;                      // the row's value at the granule's first slot
            if (lo >= 0 && lo + PER <= nstate) r[k] = *reinterpret_cast<const uint4 *>(g0 + (size_t)q * PER);
            else {
                auto at = [&](int i) { return (lo + i >= 0 && lo + i < nstate) ? row[lo + i] : (T)0; };
                if constexpr (PER == 4)
                    r[k] = make_uint4(__float_as_uint(at(0)), __float_as_uint(at(1)), __float_as_uint(at(2)), __float_as_uint(at(3)));
                else {
                    const double x = at(0), y = at(1);
                    r[k] = make_uint4((unsigned)__double2loint(x), (unsigned)__double2hiint(x), (unsigned)__double2loint(y),
                                      (unsigned)__double2hiint(y));
                }
            }
        }
    }
    __device__ __forceinline__ void store(uint4 *buf, const T *row, int nstate) const
    {
        const int ngran = (mis(row) + nstate + PER - 1) / PER;
#pragma unroll
        for (int k = 0; k < NCH; k++) {
            const int q = threadIdx.x + FS_THREADS * k;
            if (q < ngran) buf[q] = r[k];
        }
    }
};

static inline size_t re_round256(size_t n) { return (n + 255) & ~(size_t)255; }
static inline size_t re_head_bytes(int nread) { return re_round256(2 * (size_t)(nread + 1) * sizeof(int64_t)); }
