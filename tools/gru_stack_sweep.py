"""What a Gru layer launch costs OUTSIDE its step loop (design/gru_stack.md): five 96->96 layers of alternating direction, B = 1024,
chained through two buffers as the flagship chains them, timed at T' = 100, 200, 400, 800 and fitted time = intercept + slope T'.  The
slope is the chain, the intercept is what the five launches pay besides: dispatch, drain, the prologue that makes the weight images,
the fill of the first groups of x.

Every library given is run three ways where it has the entries (a library without slk_gru_bar16_stack_f32 only the first):
    layer   five slk_gru_bar16_f32 launches
    packed  five slk_gru_bar16_stack_f32 launches of one layer each (the weight images come from a pack)
    stack   one slk_gru_bar16_stack_f32 launch of five layers
in interleaved rounds (the method of tools/gru_ab.py: three untimed rounds, nine timed, two passes over the five layers per timing).
Printed per variant: the median and the spread (largest - smallest) of the rounds per T', and the fit through the medians together with
the spread of the intercepts of the nine per-round fits.
    python tools/gru_stack_sweep.py [tools/_build/libref_<rev>.so ...] [sloika_amd/_build/libsloika_amd.so]"""
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

NLAYER, I, N, B = 5, 96, 96, 1024
TS = (100, 200, 400, 800)


class StackLayer(C.Structure):
    _fields_ = [("x", C.c_void_p), ("ldx", C.c_long), ("h_out", C.c_void_p), ("ldh", C.c_long), ("pack", C.c_void_p),
                ("reverse", C.c_int), ("reserved", C.c_int)]


def main():
    import torch
    from sloika_amd import _lib
    _lib.require_gpu()
    paths = [a for a in sys.argv[1:] if a.endswith(".so")] or [_lib.LIB_PATH]
    vp = C.c_void_p
    st = torch.cuda.current_stream().cuda_stream
    g = torch.Generator(device="cuda")
    g.manual_seed(3)
    ws = []
    for _ in range(NLAYER):
        ws.append((torch.randn(3 * N, I, device="cuda", generator=g) / np.sqrt(I + N), torch.randn(3 * N, device="cuda", generator=g),
                   2 * torch.randn(2 * N, N, device="cuda", generator=g) / np.sqrt(2 * N),
                   2 * torch.randn(N, N, device="cuda", generator=g) / np.sqrt(2 * N)))
    xin = torch.randn(max(TS), B, I, device="cuda", generator=g)
    bufs = [torch.empty(max(TS), B, N, device="cuda") for _ in range(2)]
    variants = []                                       # (name, run(T))
    keep = []
    for p in paths:
        L = C.CDLL(p)
        tag = os.path.basename(p)
        L.slk_gru_bar16_f32.argtypes = [vp, C.c_long, vp, vp, vp, vp, vp, C.c_long] + [C.c_int] * 7 + [vp, vp, vp]
        L.slk_gru_bar16_f32.restype = C.c_int

        def chain(k):                                   # (input, output) of layer k
            return (xin if k == 0 else bufs[(k - 1) & 1]), bufs[k & 1]

        def run_layer(T, L=L):
            for k, (iW, bb, sW, sW2) in enumerate(ws):
                x, y = chain(k)
                rc = L.slk_gru_bar16_f32(x.data_ptr(), I, iW.data_ptr(), sW.data_ptr(), sW2.data_ptr(), bb.data_ptr(), y.data_ptr(), N, T, B,
                                         I, N, ((k + 1) & 1) | (1 << 8), 1, 2, None, None, st)
                assert rc == 0, rc
        variants.append((tag + " layer", run_layer))
        if not hasattr(L, "slk_gru_bar16_stack_f32"):
            continue
        L.slk_gru_bar16_pack_bytes.argtypes = [C.c_int, C.c_int]
        L.slk_gru_bar16_pack_bytes.restype = C.c_size_t
        L.slk_gru_bar16_pack_f32.argtypes = [vp, vp, vp, vp, C.c_int, C.c_int, vp, vp]
        L.slk_gru_bar16_pack_f32.restype = C.c_int
        L.slk_gru_bar16_stack_f32.argtypes = [C.c_int, C.POINTER(StackLayer)] + [C.c_int] * 4 + [vp, vp]
        L.slk_gru_bar16_stack_f32.restype = C.c_int
        packs = []
        for iW, bb, sW, sW2 in ws:
            pk = torch.empty(L.slk_gru_bar16_pack_bytes(I, N), dtype=torch.uint8, device="cuda")
            assert L.slk_gru_bar16_pack_f32(iW.data_ptr(), bb.data_ptr(), sW.data_ptr(), sW2.data_ptr(), I, N, pk.data_ptr(), st) == 0
            packs.append(pk)
        keep.append(packs)
        descs = (StackLayer * NLAYER)()
        for k in range(NLAYER):
            x, y = chain(k)
            descs[k] = StackLayer(x.data_ptr(), I, y.data_ptr(), N, packs[k].data_ptr(), (k + 1) & 1, 0)

        def run_packed(T, L=L, descs=descs):
            for k in range(NLAYER):
                rc = L.slk_gru_bar16_stack_f32(1, C.cast(C.byref(descs[k]), C.POINTER(StackLayer)), I, N, T, B, None, st)
                assert rc == 0, rc

        def run_stack(T, L=L, descs=descs):
            rc = L.slk_gru_bar16_stack_f32(NLAYER, descs, I, N, T, B, None, st)
            assert rc == 0, rc
        variants += [(tag + " packed", run_packed), (tag + " stack", run_stack)]

    outs = []
    for _, run in variants:                             # every variant computes the same bits
        run(TS[1])
        torch.cuda.synchronize()
        outs.append(bufs[(NLAYER - 1) & 1][:TS[1]].clone())
    for (name, _), o in zip(variants, outs):
        print("%-40s T'=%d equals the first variant bit for bit: %s" % (name, TS[1], bool(torch.equal(o, outs[0]))), flush=True)
    res = {(v, T): [] for v in range(len(variants)) for T in TS}
    for rnd in range(-3, 9):
        for T in TS:
            for v, (_, run) in enumerate(variants):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                run(T)
                run(T)
                e1.record()
                torch.cuda.synchronize()
                if rnd >= 0:
                    res[v, T].append(e0.elapsed_time(e1) / 2)
    ts = np.array(TS, dtype=np.float64)
    for v, (name, _) in enumerate(variants):
        med = np.array([np.median(res[v, T]) for T in TS])
        print("%s: ms per five layers" % name)
        for T, m in zip(TS, med):
            print("    T'=%3d median %.4f spread %.4f rounds %s" % (T, m, max(res[v, T]) - min(res[v, T]), " ".join("%.4f" % r for r in res[v, T])))
        slope, icpt = np.polyfit(ts, med, 1)
        per_round = [np.polyfit(ts, np.array([res[v, T][r] for T in TS]), 1)[1] for r in range(9)]
        print("    fit: %.3f us per step and layer, intercept %.2f us per layer (per-round intercepts: spread %.2f us, %s)"
              % (slope / NLAYER * 1e3, icpt / NLAYER * 1e3, (max(per_round) - min(per_round)) / NLAYER * 1e3,
                 " ".join("%.2f" % (p / NLAYER * 1e3) for p in per_round)), flush=True)


if __name__ == "__main__":
    main()
