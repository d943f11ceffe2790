"""csrc/gru_bar16.hip: in-process timing, the ablation launches and the per-section stamps of the diagnostic build
    tools/build_diag_lib.sh && SLOIKA_AMD_LIB=$PWD/tools/_build/libsloika_amd_diag.so python tools/bar16_check.py [IxN ...]
--store: only the gate of the h_out stores (design/gru_store.md), layer launch and one-layer stack launch."""
import sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ctypes
import numpy as np, torch
from sloika_amd import _lib
L = _lib.lib()
st = torch.cuda.current_stream().cuda_stream

def run(entry, x, iW, sW, sW2, b, T, B, I, n, rev, lens=None, zr=None):
    y = torch.full((T, B, n), float('nan'), device='cuda')
    rc = getattr(L, entry)(x.data_ptr(), I, iW.data_ptr(), sW.data_ptr(), sW2.data_ptr(), b.data_ptr(), y.data_ptr(), n, T, B, I, n, rev, 1, 2,
                           None if lens is None else lens.data_ptr(), None if zr is None else zr.data_ptr(), st)
    torch.cuda.synchronize()
    return rc, y

def store_gate(I, n, T=800, B=1024, rounds=5, reps=10):
    """What the h_out stores of a chain step consist of (design/gru_store.md): the layer launch and the one-layer stack launch (96x96),
    production next to bit 16 and its pieces, then the stack kernel's FULL instantiation.  Rounds alternate over the rows;
    printed: the median in cycles per step at 2.4 GHz, the difference to the production row of the same kind, the spread of the rounds."""
    from sloika_amd._lib import GruStackLayer
    g = torch.Generator(device='cuda'); g.manual_seed(1)
    iW = torch.randn(3 * n, I, device='cuda', generator=g) / np.sqrt(I + n)
    bb = torch.randn(3 * n, device='cuda', generator=g)
    sW = torch.randn(2 * n, n, device='cuda', generator=g) / np.sqrt(2 * n) * 2
    sW2 = torch.randn(n, n, device='cuda', generator=g) / np.sqrt(2 * n) * 2
    x = torch.randn(T, B, I, device='cuda', generator=g)
    y = torch.empty(T, B, n, device='cuda')
    pk = torch.empty(L.slk_gru_bar16_pack_bytes(I, n), dtype=torch.uint8, device='cuda')
    assert L.slk_gru_bar16_pack_f32(iW.data_ptr(), bb.data_ptr(), sW.data_ptr(), sW2.data_ptr(), I, n, pk.data_ptr(), st) == 0
    desc = (GruStackLayer * 1)(GruStackLayer(x.data_ptr(), I, y.data_ptr(), n, pk.data_ptr(), 0, 0))
    L.slk_debug_bar16_stack_variant.argtypes = [ctypes.c_int, ctypes.c_int]
    L.slk_debug_bar16_stack_variant.restype = None

    def layer(code):
        return lambda: L.slk_gru_bar16_f32(x.data_ptr(), I, iW.data_ptr(), sW.data_ptr(), sW2.data_ptr(), bb.data_ptr(), y.data_ptr(), n, T, B, I, n,
                                           2 * code | (1 << 8), 1, 2, None, None, st)

    def stack(full, abl):
        def f():
            L.slk_debug_bar16_stack_variant(full, abl)
            rc = L.slk_gru_bar16_stack_f32(1, desc, I, n, T, B, None, st)
            L.slk_debug_bar16_stack_variant(-1, 0)
            return rc
        return f
    rows = [("layer", "production", layer(0)), ("layer", "no h_out stores (16)", layer(6)), ("layer", "predicate only (4096)", layer(33)),
            ("layer", "stores without predicate (8192)", layer(34)), ("layer", "one store of two (16384)", layer(35)),
            ("layer", "row never moves (32768)", layer(36)),
            ("stack", "production (general kernel)", stack(0, 0)), ("stack", "no h_out stores (16)", stack(0, 16)),
            ("stack", "predicate only (4096)", stack(0, 4096)), ("stack", "stores without predicate (8192)", stack(0, 8192)),
            ("stack", "one store of two (16384)", stack(0, 16384)), ("stack", "row never moves (32768)", stack(0, 32768)),
            ("stack", "FULL (the full-batch kernel)", stack(1, 0)), ("stack", "FULL, no h_out stores (16)", stack(1, 16)),
            ("stack", "FULL, one store of two (16384)", stack(1, 16384))]
    res = [[] for _ in rows]
    for rnd in range(-2, rounds):
        for k, (_, _, f) in enumerate(rows):
            assert f() == 0, rows[k][:2]
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps): f()
            e1.record(); torch.cuda.synchronize()
            if rnd >= 0: res[k].append(e0.elapsed_time(e1) / reps * 1e6 / T * 2.4)
    print("store gate, I=%d n=%d T'=%d B=%d: cycles per step at 2.4 GHz, median of %d rounds of %d launches (results of ablated launches are garbage)" % (I, n, T, B, rounds, reps))
    base = {}
    for (kind, nm, _), r in zip(rows, res):
        med = float(np.median(r))
        base.setdefault(kind, med)
        print("   %-5s %-44s %7.1f  %+7.1f   spread %5.1f   rounds %s" % (kind, nm, med, med - base[kind], max(r) - min(r), " ".join("%.1f" % v for v in r)), flush=True)
    print("stamps of the layer launch, chain wave 0, cycles per step (section names: see below)")
    L.slk_debug_read_bar16.argtypes = [ctypes.c_void_p]
    for code, what in ((1, "production"), (41, "no h_out stores (16)"), (37, "predicate only (4096)"), (38, "stores without predicate (8192)"),
                       (39, "one store of two (16384)"), (40, "row never moves (32768)")):
        layer(code)(); torch.cuda.synchronize()
        stp = (ctypes.c_ulonglong * 64)()
        L.slk_debug_read_bar16(stp)
        v = [stp[i] / T for i in range(16)]
        print("   %-36s total %6.0f | %s" % (what, sum(v[:9]), " ".join("%5.0f" % v[i] for i in (0, 8, 1, 2, 3, 4, 5, 6, 7))), flush=True)


if "--store" in sys.argv:
    for I, n in [tuple(int(v) for v in a.split('x')) for a in sys.argv[1:] if 'x' in a] or [(96, 96)]:
        store_gate(I, n)
    sys.exit(0)
shapes = [(96, 96)] if len(sys.argv) < 2 else [tuple(int(v) for v in a.split('x')) for a in sys.argv[1:]]
for I, n in shapes:
    g = torch.Generator(device='cuda'); g.manual_seed(1)
    iW = torch.randn(3 * n, I, device='cuda', generator=g) / np.sqrt(I + n)
    bb = torch.randn(3 * n, device='cuda', generator=g)
    sW = torch.randn(2 * n, n, device='cuda', generator=g) / np.sqrt(2 * n) * 2
    sW2 = torch.randn(n, n, device='cuda', generator=g) / np.sqrt(2 * n) * 2
    T, B = 800, 1024
    x = torch.randn(T, B, I, device='cuda', generator=g)
    y = torch.empty(T, B, n, device='cuda')
    def timeit(entry, reps=10):
        f = lambda: getattr(L, entry)(x.data_ptr(), I, iW.data_ptr(), sW.data_ptr(), sW2.data_ptr(), bb.data_ptr(), y.data_ptr(), n, T, B, I, n, 0, 1, 2, None, None, st)
        f(); torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps): f()
        e1.record(); torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps
    for rnd in range(3):
        b = timeit('slk_gru_bar16_f32')
        print("I=%d n=%d T=800 B=1024: bar16 %.3f ms  (%.0f cycles/step at 2.4 GHz)" % (I, n, b, b * 1e6 / T * 2.4), flush=True)

    def timeit_code(code, reps=10):
        f = lambda: L.slk_gru_bar16_f32(x.data_ptr(), I, iW.data_ptr(), sW.data_ptr(), sW2.data_ptr(), bb.data_ptr(), y.data_ptr(), n, T, B, I, n, 2 * code, 1, 2, None, None, st)
        f(); torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps): f()
        e1.record(); torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps
    base = timeit_code(0)
    print("ablations (results garbage), cycles/step at 2.4 GHz; production %.0f" % (base * 1e6 / T * 2.4))
    for code, nm in ((2, "no s_barrier"), (3, "chain: no MFMAs"), (4, "cheap activations"), (5, "service waves idle"), (6, "no h_out stores"),
                     (7, "no s_barrier + service idle"), (8, "no s_barrier + no chain MFMAs"), (9, "no barrier, no chain MFMAs, service idle"), (10, "everything off"),
                     (16, "chain: no z products, no z epilogue"), (18, "chain: no projection share"),
                     (28, "chain: z products, no z epilogue"), (30, "chain: head of A without requests and stores"),
                     (32, "chain: no z epilogue + head without requests and stores"),
                     (20, "service: six tiles twice"), (22, "service: three tiles twice"),
                     (24, "chain: no projection share + service: six tiles twice"),
                     (26, "chain: no projection share + service: three tiles twice")):
        ms = timeit_code(code)
        print("   %-56s %6.0f" % (nm, ms * 1e6 / T * 2.4))
    L.slk_debug_read_bar16.argtypes = [ctypes.c_void_p]
    names = ["barrier A", "head of A up to the first MFMA", "own r and z blocks (+ what the head defers) + wait h", "r MFMAs", "z MFMAs + r epilogue + write + projection MFMAs", "barrier B",
             "reads + own c block + wait r*h (+ z epilogue where it is one block)", "c MFMAs (+ z epilogue where it is spread among them)", "tanh, blend, split, writes, stores"]
    for code, what in ((1, "production"), (17, "no z products, no z epilogue (results garbage)"),
                       (19, "chain: no projection share (results garbage)"),
                       (29, "z products, no z epilogue (results garbage)"), (31, "head of A without requests and stores (results garbage)"), (21, "service: six tiles twice"),
                       (23, "service: three tiles twice"), (25, "chain: no projection share + service: six tiles twice (results garbage)"),
                       (27, "chain: no projection share + service: three tiles twice (results garbage)")):
        L.slk_gru_bar16_f32(x.data_ptr(), I, iW.data_ptr(), sW.data_ptr(), sW2.data_ptr(), bb.data_ptr(), y.data_ptr(), n, T, B, I, n, 2 * code, 1, 2, None, None, st)
        torch.cuda.synchronize()
        stp = (ctypes.c_ulonglong * 64)()
        L.slk_debug_read_bar16(stp)
        print("stamps: %s" % what)
        for wv in range(4):
            v = [stp[wv * 16 + i] / T for i in range(16)]
            if wv < n // 32:
                print("chain wave %d: cycles per step, total %.0f" % (wv, sum(v[:9])))
                for i, nm in zip((0, 8, 1, 2, 3, 4, 5, 6, 7), names):       # stamp 8 splits section 1 at the first MFMA
                    print("   %-72s %7.0f" % (nm, v[i]))
            else:
                print("service wave %d: cycles per GROUP: work per interval %s   barrier wait per interval %s" % (
                    wv, " ".join("%5.0f" % (4 * a) for a in v[:8]), " ".join("%5.0f" % (4 * a) for a in v[8:])))
