"""A/B of two library builds on ONE device, one process: slk_softmax_viterbi_f32 (forward kernel + backtrace), interleaved rounds, and
whether the two builds decode the same paths and scores.     python tools/sv_ab.py tools/_build/libref_<rev>.so [other.so] [K ...]"""
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    import torch
    from sloika_amd import _lib
    _lib.require_gpu()
    paths = [a for a in sys.argv[1:] if a.endswith(".so")]
    if len(paths) == 1:
        paths.append(_lib.LIB_PATH)
    Ks = [int(a) for a in sys.argv[1:] if a.isdigit()] or [96]
    libs = [C.CDLL(p) for p in paths]
    vp = C.c_void_p
    T, B, S = 800, 1024, 1025
    rs = np.random.RandomState(1)
    for K in Ks:
        x = torch.tanh(torch.randn((T, B, K), device="cuda"))
        W = torch.from_numpy((rs.normal(size=(S, K)) * 0.5).astype(np.float32)).cuda()
        b = torch.from_numpy(rs.normal(size=S).astype(np.float32)).cuda()
        outs, fns = [], []
        for L in libs:
            L.slk_viterbi_kmer_workspace_bytes.restype = C.c_size_t
            L.slk_viterbi_kmer_workspace_bytes.argtypes = [C.c_int] * 4
            nws = L.slk_viterbi_kmer_workspace_bytes(T, B, 4, 5)
            ws = torch.empty(nws, dtype=torch.uint8, device="cuda")
            L.slk_softmax_viterbi_pack_bytes.restype = C.c_size_t
            L.slk_softmax_viterbi_pack_bytes.argtypes = [C.c_int] * 3
            pack = torch.empty(L.slk_softmax_viterbi_pack_bytes(K, 4, 5), dtype=torch.uint8, device="cuda")
            L.slk_softmax_viterbi_pack_f32.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, vp, vp]
            assert L.slk_softmax_viterbi_pack_f32(W.data_ptr(), b.data_ptr(), K, 4, 5, pack.data_ptr(), None) == 0
            f = L.slk_softmax_viterbi_f32
            f.argtypes = [vp, C.c_long, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, vp, C.c_int, vp,
                          C.c_size_t, vp, vp, vp, vp, vp]
            sc = torch.empty(B, dtype=torch.float32, device="cuda")
            pa = torch.full((B, T), -1, dtype=torch.int32, device="cuda")
            le = torch.empty(B, dtype=torch.int32, device="cuda")
            outs.append((sc, pa, le))

            def call(f=f, pack=pack, ws=ws, nws=nws, sc=sc, pa=pa, le=le):
                rc = f(x.data_ptr(), K, pack.data_ptr(), K, T, B, 4, 5, 0.0, 1e-5, None, 0, ws.data_ptr(), nws, sc.data_ptr(),
                       pa.data_ptr(), le.data_ptr(), None, None)
                assert rc == 0, rc
            fns.append(call)
        for c in fns:
            c()
        torch.cuda.synchronize()
        same = all(torch.equal(a, b_) for a, b_ in zip(outs[0], outs[1]))
        res = [[] for _ in libs]
        for rnd in range(-3, 9):                        # three untimed rounds first: the clock settles over the first ~50 launches
            for k, c in enumerate(fns):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(5):
                    c()
                e1.record()
                torch.cuda.synchronize()
                if rnd >= 0:
                    res[k].append(e0.elapsed_time(e1) / 5)
        a, b2 = float(np.median(res[0])), float(np.median(res[1]))
        # spread = largest - smallest of a build's own rounds: a difference between the builds counts from three times the first's
        sp = [max(r) - min(r) for r in res]
        diff = max(float((x_.float() - y_.float()).abs().max()) for x_, y_ in zip(outs[0], outs[1]))
        print("K=%d T=%d B=%d: %.4f -> %.4f ms per call incl. backtrace (%+.2f %%; spread of the rounds %.4f / %.4f ms), same paths / "
              "scores / lengths: %s (largest difference %g)" % (K, T, B, a, b2, (b2 / a - 1) * 100, sp[0], sp[1], same, diff), flush=True)
        for r in res:
            print("    rounds (ms per call, five calls each):", " ".join("%.4f" % v for v in r), flush=True)


if __name__ == "__main__":
    main()
