"""Reference model of the x-stationary projections (csrc/gemm_rows_f16x3.hip, csrc/gemm_rows.hip): numpy only, no GPU.

  split_f16x2       the row-scaled hi/lo fp16 split of slk_split_f16x2_f32 and of the kernel's own x split
  product_split64   float64 evaluation of exactly the terms the fp16 kernel sums, and the sum of their magnitudes
  product64         the plain float64 product, abs_product64 its magnitude sum
  row_stats64       softmax row statistics of given float32 logits
  paths             the kernel's dispatch restated: which x load, ring depth, epilogue and store path every workgroup and
                    tile takes (no numerics) -- the GPU tests assert with it that their shapes reach what they claim
and the shape lists of tests/test_gpu_projection_edges.py, so that tests/test_projection_ref.py can check their cover
without a GPU."""
import numpy as np

BM, BN = 128, 64                    # rows per workgroup, columns per tile (GH_BM, GH_BN; GR_BM, GR_BN)
K_MAX, N_MAX = 192, 2048            # slk_*_f16x3: K <= 192 (12 slabs of 16), N <= GH_BIASMAX
K_MAX_F32 = 128                     # slk_linear_rowstats_f32
E_MIN, E_MAX = 27, 227              # gh_pow2_scale: biased exponent of the row maximum is clamped to this interval
ACTS = {"linear": 0, "tanh": 1, "sigmoid": 2, "elu": 3, "relu": 4}


def round_up(v, m):
    return (v + m - 1) // m * m


# ------------------------------------------------------------------------------------------------ numerics
def pow2_scale(amax):
    """gh_pow2_scale: (scale, inverse scale) per row maximum; scale * amax is in [1, 2) for amax in [2^-100, 2^101)."""
    amax = np.ascontiguousarray(amax, dtype=np.float32)
    e = np.clip((amax.view(np.uint32) >> np.uint32(23)) & np.uint32(0xff), E_MIN, E_MAX).astype(np.uint32)
    inv = (e << np.uint32(23)).view(np.float32)
    sc = ((np.uint32(254) - e) << np.uint32(23)).view(np.float32)
    return sc, inv


def split_f16x2(w):
    """[rows][K] float32 -> hi, lo [rows][KP] float16 and inv [rows] float32, KP = K rounded up to 16 (zero padded):
    v = w * scale (exact), hi = float16(v), lo = float16(v - float32(hi)), both round to nearest even with fp16 subnormals.
    The row maximum is fmaxf's: a NaN entry does not take part in it."""
    w = np.ascontiguousarray(w, dtype=np.float32)
    rows, K = w.shape
    KP = round_up(K, 16)
    with np.errstate(all="ignore"):
        amax = np.fmax.reduce(np.abs(w), axis=1, initial=np.float32(0.0))
        amax = np.where(np.isnan(amax), np.float32(0.0), amax).astype(np.float32)
        sc, inv = pow2_scale(amax)
        v = np.zeros((rows, KP), np.float32)
        v[:, :K] = w * sc[:, None]
        hi = v.astype(np.float16)
        lo = (v - hi.astype(np.float32)).astype(np.float16)
    return hi, lo, inv


def product_split64(x, W, b=None):
    """What the fp16 kernel sums, in float64: (sum_k xh*wh + xh*wl + xl*wh) * xinv * winv + b.  Also S, the same sum over the
    magnitudes of the terms (times the scales, without the bias)."""
    xh, xl, xinv = (a.astype(np.float64) for a in split_f16x2(x))
    wh, wl, winv = (a.astype(np.float64) for a in split_f16x2(W))
    back = xinv[:, None] * winv[None, :]
    t = (xh @ wh.T + xh @ wl.T + xl @ wh.T) * back
    S = (np.abs(xh) @ np.abs(wh).T + np.abs(xh) @ np.abs(wl).T + np.abs(xl) @ np.abs(wh).T) * back
    if b is not None:
        t = t + np.asarray(b, np.float64)[None, :]
    return t, S


def product64(x, W, b=None):
    t = np.asarray(x, np.float64) @ np.asarray(W, np.float64).T
    return t if b is None else t + np.asarray(b, np.float64)[None, :]


def abs_product64(x, W, b=None):
    t = np.abs(np.asarray(x, np.float64)) @ np.abs(np.asarray(W, np.float64)).T
    return t if b is None else t + np.abs(np.asarray(b, np.float64))[None, :]


def row_stats64(logits_f32):
    """(maximum, sum exp(l - maximum)) per row, in float64, of the float32 logits given."""
    l = np.asarray(logits_f32, np.float32).astype(np.float64)
    m = l.max(axis=1)
    return m, np.exp(l - m[:, None]).sum(axis=1)


def act64(name, z):
    z = np.asarray(z, np.float64)
    return {"linear": lambda v: v, "tanh": np.tanh, "sigmoid": lambda v: 1.0 / (1.0 + np.exp(-v)),
            "relu": lambda v: np.maximum(v, 0.0), "elu": lambda v: np.where(v > 0, v, np.expm1(np.minimum(v, 0.0)))}[name](z)


# ------------------------------------------------------------------------------------------------ dispatch
STORES = ("patch", "acc4", "guard4", "tail4", "dword")


def paths(M, K, N, ldx, ldy, x_lead=0, y_lead=0, stats=False, act="linear"):
    """gemm_rows_f16x3_kernel's plan for one launch.  x_lead / y_lead: floats between a 16-byte boundary and the pointer.

    Returns a dict:
      ks, ring        K slabs of 16 and weight-ring depth
      xload           "vec16" (16-byte loads; for K % 16 == 8 the upper lane half of the last slab is masked) or "elem"
      xmask           True where the last slab has masked elements (K % 16 != 0)
      mode            "stats" or the activation
      ntiles, nfull   column tiles, and those whose 64 columns all exist
      wgs             per workgroup: dict(rows, fast, pairs, handover, tiles)
                        rows      rows of the workgroup that exist (1 .. 128)
                        fast      takes the branch-free loop at all (whole workgroup inside M, aligned y rows)
                        pairs     passes of the two-tile loop (each wave half runs its own instruction order)
                        handover  "single" when the guarded loop ends on one leftover tile (accA = accB), "double" when it ends
                                  on a pair, "none" when only the final epilogue is left
                        tiles     per tile (epilogue, store): epilogue "fast" / "guarded", store one of STORES
    Restated from the kernel text, not derived from it at run time: a change of the kernel's plan must be made here too."""
    assert 1 <= K <= K_MAX and 1 <= N <= N_MAX and M >= 1 and ldx >= K and ldy >= N
    assert not (stats and act != "linear")
    ks = (K + 15) // 16
    ring = 3 if ks <= 9 else 2
    xvec = K % 8 == 0 and ldx % 4 == 0 and x_lead % 4 == 0
    vec_ok = ldy % 4 == 0 and y_lead % 4 == 0
    tr = ks <= 8
    ntiles, nfull = (N + BN - 1) // BN, N // BN
    wgs = []
    for m0 in range(0, M, BM):
        fast = vec_ok and m0 + BM <= M
        tiles = [None] * ntiles
        nt = 1
        pairs = 0
        if fast:
            nfast = min(nfull, ntiles - 1)
            while nt + 1 <= nfast:
                tiles[nt - 1] = tiles[nt] = ("fast", "patch" if tr else "acc4")
                nt += 2
                pairs += 1
        handover = "none"
        while nt < ntiles:                              # the guarded loop
            handover = "double" if nt + 1 < ntiles else "single"
            nt += 2
        for t in range(ntiles):
            if tiles[t] is None:
                full = (t + 1) * BN <= N
                tiles[t] = ("guarded", "guard4" if full and vec_ok else "tail4" if vec_ok and N % 4 == 0 else "dword")
        wgs.append(dict(rows=min(BM, M - m0), fast=fast, pairs=pairs, handover=handover, tiles=tiles))
    return dict(ks=ks, ring=ring, xload="vec16" if xvec else "elem", xmask=K % 16 != 0, mode="stats" if stats else act,
                ntiles=ntiles, nfull=nfull, wgs=wgs)


def combos(p):
    """{(ks, ring, epilogue, store, xload, mode)} of one paths() result."""
    return {(p["ks"], p["ring"], e, s, p["xload"], p["mode"]) for wg in p["wgs"] for (e, s) in wg["tiles"]}


def paths_f32(M, K, N, w_lead=0):
    """gemm_rows_kernel's plan: A registers per lane half (None: unsupported) and the weight tile's load."""
    areg = 32 if K <= 64 else 48 if K <= 96 else 64 if K <= 128 else None
    return dict(areg=areg, wload="vec16" if (K % 4 == 0 and w_lead % 4 == 0) else "elem", ntiles=(N + BN - 1) // BN,
                rows_last=M - (M - 1) // BM * BM)


# ------------------------------------------------------------------------------------------------ layouts and shape lists
class Layout:
    """Row strides and pointer offsets of x and y for a shape: every stride leaves a gap behind its row."""

    def __init__(self, name, y_mod, x_lead, y_lead):
        self.name, self.y_mod, self.x_lead, self.y_lead = name, y_mod, x_lead, y_lead

    def ldx(self, K):
        return round_up(K, 4) + 4

    def ldy(self, N):
        ld = round_up(N, 4) + 4
        return ld if self.y_mod == 0 else ld + 1        # y_mod 1: an odd stride

    def paths(self, M, K, N, stats=False, act="linear"):
        return paths(M, K, N, self.ldx(K), self.ldy(N), self.x_lead, self.y_lead, stats, act)

    def __repr__(self):
        return self.name


ALIGNED = Layout("aligned", 0, 0, 0)        # 16-byte x loads where K allows, every float4 store
ODD_LDY = Layout("odd_ldy", 1, 0, 0)        # 16-byte x loads, dword stores only
OFF_ONE = Layout("off_one", 0, 1, 1)        # x and y one float past a 16-byte boundary: element x loads, dword stores
LAYOUTS = (ALIGNED, ODD_LDY, OFF_ONE)

SWEEP_M, SWEEP_N = 257, 193
KS_SWEEP_K = (1, 7, 8, 9, 15, 16, 17, 24, 31, 32, 33, 40, 48, 64, 65, 72, 80, 96, 97, 112, 127, 128, 129, 136, 144, 145, 160,
              161, 176, 177, 191, 192)
TILE_SWEEP_N = tuple(sorted({1, 3, 4, 63, 64, 65, 68} | {n + d for n in (64, 128, 192, 256, 320, 384) for d in (-1, 0, 1, 4)}))
TILE_SWEEP_K = (96, 176)                    # ring 3 and ring 2
ROW_SWEEP_M = (1, 31, 32, 33, 127, 128, 129, 255, 256, 257)
ROW_SWEEP_KN = ((96, 129), (176, 68))
ACT_SHAPES = ((257, 96, 193), (257, 176, 132), (129, 24, 64))
MODES = ("stats", "linear", "tanh", "sigmoid", "relu", "elu")
GHOST_N = (65, 129, 193)
ACCURACY_K = (16, 24, 40, 64, 72, 96, 112, 128, 136, 160, 176, 192)       # one K % 8 == 0 per slab count 1 .. 12
F32_SWEEP_K = (1, 3, 4, 5, 63, 64, 65, 95, 96, 97, 127, 128)
F32_TILE_K = (65, 128)
F32_ROW_KN = ((96, 129), (128, 68))
SPLIT_ROWS = (1, 4, 5, 8193)
SPLIT_K = (1, 15, 16, 17, 63, 64, 65, 192)


def mode_paths(lay, M, K, N, mode):
    return lay.paths(M, K, N, stats=mode == "stats", act="linear" if mode == "stats" else mode)
