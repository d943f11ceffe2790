"""csrc/decode.hip, the stand-alone Viterbi decoder, at the edges of every kernel it launches -- all through the C ABI, all bit for
bit (float32 score, int32 path with its -1 padding, length) against the oracle decoder run on the log-posteriors the device
itself consumed: the input in log mode, slk_log_post_f32 / slk_log_post_logits_f32 of the same buffers in the other modes.

Nothing about the dispatch is written down here: every test asks slk_viterbi_kmer_plan which kernel its shape takes and FAILS if
that is not the kernel it means to pin, and every edge length is computed from the plan's block sizes (tests/viterbi_cases.py).

  forward kernels   chunk lengths around one and two blocks of blank-column steps, around the staged traceback rows, and the first
                    trips of the time loops; all four input modes; skip penalties 0 and 2.5
  walker            1 to 5 staged blocks (every state of the DMA ring and of the plain staging loop), a workspace 8 bytes off
                    alignment, DMA-ring cases three times with the same bits
  shift-left        paths of length 1 and of length T past one and two tiles, ragged with Tpad > T
  ragged            lengths 1, 2, T and the block edges; every logit and statistic beyond a chunk's end is NaN
  argmax            slk_argmax_decode_f32 against numpy
"""
import numpy as np
import pytest

from tests import viterbi_cases as vc
from tests.gpu_util import need_gpu, dev, stream

pytestmark = pytest.mark.gpu
SKIPS = (0.0, 2.5)


def _planned(T, B, nbase, klen, kernel, ws_align=16):
    """The plan of this shape, which must be the kernel the test is about."""
    p, big = vc.plan(T, B, nbase, klen, ws_align), vc.plan(vc.LONG, B, nbase, klen, ws_align)
    assert p.kernel == kernel, "T=%d B=%d nbase=%d klen=%d runs kernel %d, the test is about kernel %d" % (T, B, nbase, klen, p.kernel, kernel)
    assert p[:4] == big[:4] and p.walker_rows == min(big.walker_rows, T) and p.walker_dma == big.walker_dma
    return p


def _decode(torch, mode, T, B, nbase, klen, skip, data, stats=None, ld=0, lens=None, ws_offset=0):
    """One call of the C ABI with outputs that start as garbage; the workspace `ws_offset` bytes behind a 16-byte boundary."""
    from sloika_amd import _lib
    L = _lib.lib()
    nbytes = L.slk_viterbi_kmer_workspace_bytes(T, B, nbase, klen)
    assert nbytes > 0
    ws = torch.empty(nbytes + 16, dtype=torch.uint8, device="cuda")
    assert ws.data_ptr() % 16 == 0 and 0 <= ws_offset <= 16
    sc = torch.full((B,), float("nan"), dtype=torch.float32, device="cuda")
    pa = torch.full((B, T), -7, dtype=torch.int32, device="cuda")
    le = torch.full((B,), -7, dtype=torch.int32, device="cuda")
    out = (ws.data_ptr() + ws_offset, nbytes, sc.data_ptr(), pa.data_ptr(), le.data_ptr(), stream())
    if mode == "logits" and lens is not None:
        rc = L.slk_viterbi_kmer_logits_ragged_f32(data.data_ptr(), ld, stats.data_ptr(), T, B, nbase, klen, skip, vc.MIN_PROB,
                                                  lens.data_ptr(), *out)
    elif mode == "logits":
        rc = L.slk_viterbi_kmer_logits_f32(data.data_ptr(), ld, stats.data_ptr(), T, B, nbase, klen, skip, vc.MIN_PROB, *out)
    else:
        assert lens is None, "the ragged entry takes logits"
        m = {"log": _lib.POST_LOG, "plain": _lib.POST_PLAIN, "raw": _lib.POST_RAW}[mode]
        rc = L.slk_viterbi_kmer_f32(data.data_ptr(), T, B, nbase, klen, skip, m, vc.MIN_PROB if mode == "raw" else 0.0, *out)
    assert rc == 0, rc
    return sc, pa, le


def _device_log_post(torch, mode, data, stats, ld, rows, nst):
    """The log-posteriors the decoder derives from this input, dense [rows, nst] (the conversion kernels share its device functions)."""
    from sloika_amd import _lib
    L = _lib.lib()
    lp = torch.empty((rows, nst), dtype=torch.float32, device="cuda")
    if mode == "logits":
        assert L.slk_log_post_logits_f32(data.data_ptr(), ld, stats.data_ptr(), lp.data_ptr(), rows, nst, vc.MIN_PROB, stream()) == 0
    else:
        m = {"plain": _lib.POST_PLAIN, "raw": _lib.POST_RAW}[mode]
        assert L.slk_log_post_f32(data.data_ptr(), lp.data_ptr(), rows * nst, m, vc.MIN_PROB if mode == "raw" else 0.0, stream()) == 0
    return lp


def _assert_same(got, want, what):
    s, p, n = (x.cpu().numpy() if hasattr(x, "cpu") else x for x in got)
    ws, wp, wn = (x.cpu().numpy() if hasattr(x, "cpu") else x for x in want)
    assert np.array_equal(n, wn), (what, "lengths", n, wn)
    bad = np.nonzero((p != wp).any(axis=1))[0]
    assert bad.size == 0, (what, "paths of chunks", bad[:8], p[bad[0]], wp[bad[0]])
    assert np.array_equal(s, ws), (what, "scores", s, ws)


def _small_case(oracle, mode, T, B, nbase, klen, skip, kernel, lens=None, ld_pad=0, ws_offset=0, seed=0):
    """One small batch of every chunk kind (tests/viterbi_cases.py), built on the host, decoded on the device and by the oracle.
    `lens`: a ragged batch of padded length T.  Returns the device's results."""
    torch = need_gpu()
    p = _planned(T, B, nbase, klen, kernel, 16 if ws_offset == 0 else ws_offset)
    assert p.walker_dma == (1 if nbase == 4 and ws_offset == 0 else 0)
    full, kmer = vc.tie_steps(T, p)
    L = vc.scores(T, B, nbase, klen, 1000 * T + 10 * B + klen + seed, full, kmer, log_mode=mode == "log")
    nst = L.shape[2]
    stats = lens_d = None
    ld = 0
    if mode == "log":
        data, lp = dev(L), L
    else:
        if mode == "logits":
            buf, st, ld = vc.logits_of(L, seed=T + B, ld=nst + ld_pad)
            if lens is not None:
                vc.poison(buf, st, lens, T, B)
                lens_d = dev(np.asarray(lens, dtype=np.int32))
            data, stats = dev(buf), dev(st)
            ref = vc.numpy_log_post(mode, buf, st, nst)
        else:
            post = vc.softmax(L)
            data = dev(post)
            ref = vc.numpy_log_post(mode, post).reshape(T * B, nst)
        lp = _device_log_post(torch, mode, data, stats, ld, T * B, nst).cpu().numpy()
        live = np.isfinite(ref).all(axis=1)
        assert live.sum() == (T * B if lens is None else int(np.sum(lens)))
        np.testing.assert_allclose(lp[live], ref[live], rtol=1e-6, atol=2e-6)      # the bounds of tests/test_gpu_decode.py
        lp = lp.reshape(T, B, nst)
    want = vc.expected(oracle, lp, klen, skip, nbase, lens)
    kinds = vc.kinds_of(B, mode == "log")
    own = np.full(B, T) if lens is None else np.asarray(lens)
    if "stay" in kinds:
        assert want[2][kinds.index("stay")] == 1
    if "move" in kinds:
        assert want[2][kinds.index("move")] == own[kinds.index("move")]
    what = (mode, T, B, nbase, klen, skip, ws_offset)
    got = _decode(torch, mode, T, B, nbase, klen, skip, data, stats, ld, lens_d, ws_offset)
    _assert_same(got, want, what)
    for rep in range(2 if p.walker_dma else 0):          # the ring's waits are counted by hand: same bits every time
        _assert_same(_decode(torch, mode, T, B, nbase, klen, skip, data, stats, ld, lens_d, ws_offset), got, what + ("repeat", rep))
    return got


# ---- viterbi_forward4_kernel: one workgroup per chunk, nbase 4 -------------------------------------------------------------------------

def _workgroup_lengths(klen, group):
    p = vc.plan(vc.LONG, 1, 4, klen)
    assert p.kernel == vc.WORKGROUP4 and p.staged_rows > 0 and p.blank_steps >= 64 and p.walker_dma == 1
    if group == "walker":
        return vc.walker_lengths(p.walker_rows)
    if group == "staging":
        return vc.staging_lengths(p.staged_rows)
    return vc.blank_lengths(p.blank_steps)


@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("group", ["walker", "staging", "blank"])
@pytest.mark.parametrize("klen", [3, 4, 5])
def test_workgroup_kernel_lengths(oracle, klen, group, B):
    for i, T in enumerate(_workgroup_lengths(klen, group)):
        _small_case(oracle, "log", T, B, 4, klen, SKIPS[i % 2], vc.WORKGROUP4)


@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("group", ["walker", "staging"])
def test_workgroup_kernel_lengths_4096_kmers(oracle, group, B):
    for i, T in enumerate(_workgroup_lengths(6, group)):
        _small_case(oracle, "log", T, B, 4, 6, SKIPS[i % 2], vc.WORKGROUP4)


def test_workgroup_kernel_4096_kmers_second_blank_block(oracle):
    """The one crossing of a blank block at klen 6 (1024 steps per block): two chunks, one step into the second block."""
    n = vc.plan(vc.LONG, 2, 4, 6).blank_steps
    _small_case(oracle, "log", n + 1, 2, 4, 6, 2.5, vc.WORKGROUP4)


@pytest.mark.parametrize("mode,ld_pad", [("plain", 0), ("raw", 0), ("logits", 0), ("logits", 31)])
@pytest.mark.parametrize("klen", [3, 4, 5])
def test_workgroup_kernel_input_modes_across_a_blank_block(oracle, klen, mode, ld_pad):
    n = vc.plan(vc.LONG, 5, 4, klen).blank_steps
    for T, skip in ((n, 0.0), (n + 1, 2.5), (2 * n + 1, 0.0)):
        _small_case(oracle, mode, T, 5, 4, klen, skip, vc.WORKGROUP4, ld_pad=ld_pad)


def _ragged_edges(p):
    return sorted(set(vc.walker_lengths(p.walker_rows)[:5] + vc.blank_lengths(max(p.blank_steps, 1))[:4]
                      + vc.staging_lengths(max(p.staged_rows, 2))[1:5]))


@pytest.mark.parametrize("klen", [3, 4, 5])
def test_workgroup_kernel_ragged(oracle, klen):
    p = vc.plan(vc.LONG, 1, 4, klen)
    edges = _ragged_edges(p)
    B = len(edges) + 3
    for T, skip, ld_pad in ((max(edges) + 3, 0.0, 0), (2 * p.walker_rows + 2, 2.5, 7)):
        lens = vc.ragged_lengths(T, B, edges)
        assert {1, 2, T} <= set(lens.tolist()) and set(e for e in edges if 2 < e < T) <= set(lens.tolist())
        _small_case(oracle, "logits", T, B, 4, klen, skip, vc.WORKGROUP4, lens=lens, ld_pad=ld_pad)


@pytest.mark.parametrize("nbase,klen", [(4, 3), (4, 5), (5, 3)])
def test_no_score_above_minus_infinity(oracle, nbase, klen):
    """A row that is all -inf kills every state: the score is -inf and the path ends in state 0, np.argmax's answer
    (the kernels' arg-max reduction starts from an index no state has).  The wave kernel's batches hold the same chunk kind."""
    kernel = vc.WORKGROUP4 if nbase == 4 else vc.GENERIC
    B = len(vc.KINDS)
    for T in (1, 2, 3, 40):
        sc, pa, le = _small_case(oracle, "log", T, B, nbase, klen, 0.0, kernel)
        dead = vc.KINDS.index("dead")
        assert np.isneginf(sc.cpu().numpy()[dead]) and pa.cpu().numpy()[dead, int(le[dead]) - 1] == 0


# ---- viterbi_forward4_wave_kernel: one wave per chunk, batches from the threshold up ----------------------------------------------------

def _wave_case(oracle, klen, T, skip, ragged, seed):
    """Batches of threshold + 1, + 2 and + 3 chunks (the last workgroup holds 1, 2 and 3 waves), made on the device with the
    host-built chunk kinds at both ends.  Every chunk must equal the workgroup kernel's result for it, a sample the oracle's."""
    torch = need_gpu()
    thr = vc.wave_threshold(klen)
    nst = 4 ** klen + 1
    g = torch.Generator(device="cuda").manual_seed(seed)
    lp_all = torch.log_softmax(3.0 * torch.randn((T, thr + 3, nst), device="cuda", generator=g), dim=2)
    K = len(vc.KINDS)
    mode = "logits" if ragged else "log"
    for B in (thr + 1, thr + 2, thr + 3):
        p = _planned(T, B, 4, klen, vc.WAVE4)
        full, kmer = vc.tie_steps(T, p)
        special = dev(vc.scores(T, K, 4, klen, seed + B, full, kmer, log_mode=not ragged))
        x = lp_all[:, :B].clone()
        x[:, :K] = special
        x[:, B - K:] = special.flip(1)                       # the last chunk is the one with the tied rows
        mid = thr // 2
        sample = list(range(8)) + list(range(mid, mid + 4)) + list(range(B - 8, B))
        assert len(set(sample)) >= 16 and {b % 4 for b in sample[-4:]} == {0, 1, 2, 3}
        stats = lens_d = lens = None
        ld = 0
        if ragged:
            ld = nst + (7 if B % 2 else 0)
            x += 3.0 * torch.randn((T, B, 1), device="cuda", generator=g)
            mx = x.max(dim=2).values
            stats = torch.stack([mx, 1.0 / torch.exp(x - mx[:, :, None]).sum(dim=2)], dim=2).contiguous()
            edges = [e for e in vc.blank_lengths(p.blank_steps) + [3, 4] if e < T]
            lens_d = torch.randint(1, T + 1, (B,), device="cuda", generator=g, dtype=torch.int32)
            lens_d[sample] = dev(vc.ragged_lengths(T, len(sample), edges))
            lens = lens_d.cpu().numpy()
            dead = torch.arange(T, device="cuda")[:, None] >= lens_d[None, :]
            x[dead] = float("nan")
            stats[dead] = float("nan")
            buf = torch.full((T, B, ld), float("nan"), dtype=torch.float32, device="cuda")
            buf[:, :, :nst] = x
            x = buf
        what = ("wave", klen, T, B, skip, ragged)
        got = _decode(torch, mode, T, B, 4, klen, skip, x, stats, ld, lens_d)
        assert p.walker_dma == 1
        for rep in range(2):                                 # the ring's waits are counted by hand: same bits every time
            _assert_same(_decode(torch, mode, T, B, 4, klen, skip, x, stats, ld, lens_d), got, what + ("repeat", rep))
        # the same chunks through the workgroup kernel, in slices below the threshold
        for lo, hi in ((0, B // 2), (B // 2, B)):
            _planned(T, hi - lo, 4, klen, vc.WORKGROUP4)
            part = _decode(torch, mode, T, hi - lo, 4, klen, skip, x[:, lo:hi].contiguous(),
                           None if stats is None else stats[:, lo:hi].contiguous(), ld,
                           None if lens_d is None else lens_d[lo:hi].contiguous())
            _assert_same(tuple(r[lo:hi] for r in got), part, what + ("workgroup kernel on chunks", lo, hi))
        # the oracle on a sample: first and last chunk, all four wave positions, every chunk kind, the ragged extremes
        xs = x[:, sample].contiguous()
        if ragged:
            lp = _device_log_post(torch, mode, xs, stats[:, sample].contiguous(), ld, T * len(sample), nst)
            lp = lp.cpu().numpy().reshape(T, len(sample), nst)
            assert {1, 2, T} <= set(lens[sample].tolist()) or T < 3
        else:
            lp = xs.cpu().numpy()
        want = vc.expected(oracle, lp, klen, skip, 4, None if lens is None else lens[sample])
        _assert_same(tuple(r[sample] for r in got), want, what + ("oracle on chunks", sample))
        del x, got


def _wave_lengths(group):
    p = vc.plan(vc.LONG, vc.wave_threshold(3), 4, 3)
    assert p.kernel == vc.WAVE4
    return {"walker": vc.walker_lengths(p.walker_rows), "blank": vc.blank_lengths(p.blank_steps), "first": [1, 2, 3, 4]}[group]


@pytest.mark.parametrize("ragged", [False, True])
@pytest.mark.parametrize("group", ["first", "blank", "walker"])
def test_wave_kernel_lengths(oracle, group, ragged):
    for i, T in enumerate(_wave_lengths(group)):
        _wave_case(oracle, 3, T, SKIPS[i % 2], ragged, seed=T)


@pytest.mark.parametrize("ragged", [False, True])
def test_wave_kernel_256_kmers_past_two_blank_blocks(oracle, ragged):
    n = vc.plan(vc.LONG, vc.wave_threshold(4), 4, 4).blank_steps
    _wave_case(oracle, 4, 2 * n + 1, 2.5, ragged, seed=4)


@pytest.mark.parametrize("ragged", [False, True])
@pytest.mark.parametrize("which", ["prefetch", "second_blank_block"])
def test_wave_kernel_1024_kmers(oracle, which, ragged):
    n = vc.plan(vc.LONG, vc.wave_threshold(5), 4, 5).blank_steps
    _wave_case(oracle, 5, 3 if which == "prefetch" else n + 2, 0.0 if ragged else 2.5, ragged, seed=5)


# ---- viterbi_forward_kernel<5>: the generic kernel and the walker's plain staging loop -------------------------------------------------

@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("klen", [3, 4, 5])
def test_generic_kernel_one_to_five_walker_blocks(oracle, klen, B):
    p = vc.plan(vc.LONG, B, 5, klen)
    assert p.kernel == vc.GENERIC and p.walker_dma == 0 and p.tb_row_bytes == 5 ** klen
    lengths = vc.walker_lengths(p.walker_rows)
    assert [-(-(T - 1) // p.walker_rows) for T in lengths] == [1, 1, 2, 2, 3, 3, 4, 5]
    for i, T in enumerate(lengths):
        _small_case(oracle, "log", T, B, 5, klen, SKIPS[i % 2], vc.GENERIC)
        _small_case(oracle, ("plain", "raw")[i % 2], T, B, 5, klen, SKIPS[1 - i % 2], vc.GENERIC)


@pytest.mark.parametrize("B", [1, 3, 9])
@pytest.mark.parametrize("klen", [3, 4, 5])
def test_generic_kernel_ragged(oracle, klen, B):
    p = vc.plan(vc.LONG, B, 5, klen)
    lengths = vc.walker_lengths(p.walker_rows)
    for i, T in enumerate(lengths[2:]):
        edges = lengths[i:] + lengths[:i]
        lens = vc.ragged_lengths(T, B, edges) if B > 1 else np.asarray([edges[0] if edges[0] < T else T], dtype=np.int32)
        _small_case(oracle, "logits", T, B, 5, klen, SKIPS[i % 2], vc.GENERIC, lens=lens, ld_pad=3 * (i % 2))


# ---- a workspace that is not 16-byte aligned: 4-byte traceback stores, no DMA ring -----------------------------------------------------

@pytest.mark.parametrize("klen", [3, 5])
def test_unaligned_workspace_workgroup_kernel(oracle, klen):
    p = vc.plan(vc.LONG, 5, 4, klen)
    r = p.walker_rows
    for T, skip in ((2 * r + 2, 0.0), (r, 2.5), (2 * p.staged_rows + 3, 0.0)):
        a = _small_case(oracle, "log", T, 5, 4, klen, skip, vc.WORKGROUP4)
        b = _small_case(oracle, "log", T, 5, 4, klen, skip, vc.WORKGROUP4, ws_offset=8)
        _assert_same(b, a, ("unaligned", klen, T))
    edges = _ragged_edges(vc.plan(vc.LONG, 1, 4, klen))
    T, B = 2 * r + 2, len(edges) + 3
    lens = vc.ragged_lengths(T, B, edges)
    a = _small_case(oracle, "logits", T, B, 4, klen, 2.5, vc.WORKGROUP4, lens=lens, ld_pad=5)
    b = _small_case(oracle, "logits", T, B, 4, klen, 2.5, vc.WORKGROUP4, lens=lens, ld_pad=5, ws_offset=8)
    _assert_same(b, a, ("unaligned ragged", klen, T))


def test_unaligned_workspace_wave_kernel(oracle):
    """The wave kernel stores its traceback as 8-byte words: 8 bytes off is the least aligned workspace it can take."""
    torch = need_gpu()
    klen = 3
    nst = 4 ** klen + 1
    B = vc.wave_threshold(klen) + 1
    p = vc.plan(vc.LONG, B, 4, klen)
    r = p.walker_rows
    g = torch.Generator(device="cuda").manual_seed(8)
    for T in (p.blank_steps + 2, r + 2):
        assert _planned(T, B, 4, klen, vc.WAVE4, 16).walker_dma == 1 and _planned(T, B, 4, klen, vc.WAVE4, 8).walker_dma == 0
        lp = torch.log_softmax(3.0 * torch.randn((T, B, nst), device="cuda", generator=g), dim=2)
        lp[T // 2] = lp[T // 2, :, :1]
        a = _decode(torch, "log", T, B, 4, klen, 2.5, lp)
        b = _decode(torch, "log", T, B, 4, klen, 2.5, lp, ws_offset=8)
        _assert_same(b, a, ("unaligned wave", T))
        sample = [0, 1, 2, 3, B // 2, B - 1]
        _assert_same(tuple(x[sample] for x in b), vc.expected(oracle, lp[:, sample].cpu().numpy(), klen, 2.5, 4), ("unaligned wave", T))


# ---- the walker's shift-left: tiles of path entries, paths of length 1 and of length T ------------------------------------------------

@pytest.mark.parametrize("T", [257, 513, 700])
@pytest.mark.parametrize("nbase,klen", [(4, 3), (5, 3)])
def test_shift_left_and_padding(oracle, nbase, klen, T):
    kernel = vc.WORKGROUP4 if nbase == 4 else vc.GENERIC
    sc, pa, le = _small_case(oracle, "log", T, 5, nbase, klen, 0.0, kernel)
    le = le.cpu().numpy()
    assert le[vc.KINDS.index("stay")] == 1 and le[vc.KINDS.index("move")] == T and 1 < le[0] < T
    # ragged, the padded length beyond every chunk's own: the all-move chunk's path fills its T entries, -1 from there to Tpad
    Tpad = T + 37
    lens = np.asarray([T, T, T, 2, T - 1, 256, 1], dtype=np.int32)
    sc, pa, le = _small_case(oracle, "logits", Tpad, 7, nbase, klen, 2.5, kernel, lens=lens, ld_pad=3)
    pa, le = pa.cpu().numpy(), le.cpu().numpy()
    assert le[1] == 1 and le[2] == T and (le <= lens).all()
    for b in range(7):
        assert (pa[b, le[b]:] == -1).all() and (pa[b, :le[b]] >= 0).all()


# ---- slk_argmax_decode_f32 -------------------------------------------------------------------------------------------------------------

def _argmax_ref(post, zero_is_blank):
    T, B, nst = post.shape
    am = post.argmax(axis=2)                               # first maximum
    blank = 0 if zero_is_blank else nst - 1
    paths = np.full((B, T), -1, dtype=np.int32)
    lens = np.zeros(B, dtype=np.int32)
    for b in range(B):
        seq = am[:, b][am[:, b] != blank] - (1 if zero_is_blank else 0)
        paths[b, :len(seq)] = seq
        lens[b] = len(seq)
    return paths, lens


@pytest.mark.parametrize("nst", [5, 64, 65, 1025])
def test_argmax_decode_vs_numpy(nst):
    torch = need_gpu()
    from sloika_amd import _lib
    L = _lib.lib()
    for T in (1, 3, 4, 5, 300):
        for zib in (0, 1):
            blank = 0 if zib else nst - 1
            rs = np.random.RandomState(nst + T + zib)
            # four levels only: most rows have several tied maxima, spread over the lanes and over a lane's own states
            base = (rs.randint(0, 4, size=(T, 7, nst)) / 4.0).astype(np.float32)
            base[:, 0, blank] = 2.0                        # all blank: length 0
            base[:, 1, blank] = -1.0                       # never blank: length T
            base[:, 2, :] = 0.5                            # everything tied: state 0 wins
            for post in (base, base[:, :1], base[:, 1:2], base[:, 3:4]):
                post = np.ascontiguousarray(post)
                B = post.shape[1]
                pd = dev(post)
                pa = torch.full((B, T), -7, dtype=torch.int32, device="cuda")
                le = torch.full((B,), -7, dtype=torch.int32, device="cuda")
                assert L.slk_argmax_decode_f32(pd.data_ptr(), T, B, nst, zib, pa.data_ptr(), le.data_ptr(), stream()) == 0
                want_p, want_l = _argmax_ref(post, zib)
                assert np.array_equal(le.cpu().numpy(), want_l), (nst, T, zib, B)
                assert np.array_equal(pa.cpu().numpy(), want_p), (nst, T, zib, B)
            want_p, want_l = _argmax_ref(base, zib)
            assert want_l[0] == 0 and want_l[1] == T
