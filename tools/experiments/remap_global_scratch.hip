// The simplest way to remap a reference of any length (design/remap_long.md, 4, "the simplest alternative"): the LDS-resident
// kernel's own body, map_to_sequence_body, pointed at a scratch in GLOBAL memory of the layout it keeps in LDS (7 words per position
// and the slack), behind the read's traceback.  An experiment, not part of the library (sloika_amd/build.py compiles csrc/ only): the
// tiled kernel had to beat it to ship.  It takes the arguments of slk_map_to_sequence_long_batch_f32 (`tile` is ignored) and a
// workspace of nev * npos + 7 * npos + 33 int32 per read, which tools/remap_time.py --experiment leaves room for:
//
//   hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -fno-fast-math -ffp-contract=off -shared -I sloika_amd/csrc -I include \
//         tools/experiments/remap_global_scratch.hip -o tools/_build/libremap_global_scratch.so
//   python tools/remap_time.py --events 2000 --positions 11692 --long --experiment tools/_build/libremap_global_scratch.so
#include "../../sloika_amd/csrc/transducer.hip"

__global__ void __launch_bounds__(256) exp_global_scratch_batch_kernel(const float *__restrict__ ltrans, int nst,
                                                                       const int64_t *__restrict__ ev_off,
                                                                       const int32_t *__restrict__ seq,
                                                                       const int64_t *__restrict__ pos_off, float slip,
                                                                       const double *__restrict__ prior_initial,
                                                                       const double *__restrict__ prior_final, int32_t *vmat,
                                                                       const int64_t *__restrict__ ws_off,
                                                                       float *__restrict__ score_out, int32_t *__restrict__ path_out)
{
    const int b = blockIdx.x;
    const int64_t e0 = ev_off[b], p0 = pos_off[b];
    const int nev = (int)(ev_off[b + 1] - e0), npos = (int)(pos_off[b + 1] - p0);
    if (nev < 1 || npos < 3) {
        if (threadIdx.x == 0) score_out[b] = -INFINITY;
        return;
    }
    int32_t *vm = vmat + ws_off[b];
    // the first 8-byte boundary behind the traceback: the pairs are read as 8 bytes
    float *scratch = reinterpret_cast<float *>((reinterpret_cast<uintptr_t>(vm + (size_t)nev * npos) + 7) & ~(uintptr_t)7);
    map_to_sequence_body(scratch, ltrans + e0 * nst, nev, nst, seq + p0, npos, slip, prior_initial ? prior_initial + p0 : nullptr,
                         prior_final ? prior_final + p0 : nullptr, vm, score_out + b, path_out + e0);
}

extern "C" __attribute__((visibility("default"))) int exp_map_to_sequence_long_batch_f32(
    const float *ltrans, int nst, const int64_t *ev_off, const int32_t *seq, const int64_t *pos_off, int nread, int max_npos, float slip,
    const double *prior_initial, const double *prior_final, void *workspace, const int64_t *ws_off, int tile, float *score_out,
    int32_t *path_out, slk_stream_t stream)
{
    if (!ltrans || !ev_off || !seq || !pos_off || !workspace || !ws_off || !score_out || !path_out || nst < 1 || nread < 1 || max_npos < 3)
        return SLK_ERR_INVALID_ARG;
    hipLaunchKernelGGL(exp_global_scratch_batch_kernel, dim3(nread), dim3(256), 0, slk_stream(stream), ltrans, nst, ev_off, seq, pos_off,
                       slip, prior_initial, prior_final, static_cast<int32_t *>(workspace), ws_off, score_out, path_out);
    return slk_launch_status();
}
