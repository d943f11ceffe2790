"""The inputs of the stand-alone decoder's edge tests (tests/viterbi_cases.py) and the plan query they rely on, without a GPU:
the C oracle and the scalar python decoder agree bit for bit on every chunk kind, the kinds are what they claim to be (all-stay:
length 1, all-move: length T, tied rows tie), and slk_viterbi_kmer_plan reports the dispatch csrc/decode.hip documents."""
import numpy as np
import pytest

from tests import viterbi_cases as vc

SHAPES = [(4, 3), (4, 4), (4, 6), (5, 3), (5, 4), (5, 5)]


def _small_T(nbase, klen):
    return 12 if nbase ** klen <= 256 else (6 if nbase ** klen <= 1024 else 4)


@pytest.mark.parametrize("nbase,klen", SHAPES)
@pytest.mark.parametrize("skip", [0.0, 2.5])
def test_oracle_equals_python_decoder_on_every_chunk_kind(oracle, nbase, klen, skip):
    from oracle import oracle_np
    T = _small_T(nbase, klen)
    B = len(vc.KINDS)
    L = vc.scores(T, B, nbase, klen, seed=100 * klen + nbase, tied_full=[T // 2], tied_kmer=[1])
    o_s, o_p, o_l = oracle.viterbi_batch(L, klen, skip_pen=skip, nbase=nbase)
    for b, kind in enumerate(vc.kinds_of(B)):
        score, path = oracle_np.viterbi_py(L[:, b], klen, skip_pen=skip, log=True, nbase=nbase)
        assert list(o_p[b, :o_l[b]]) == path and (o_p[b, o_l[b]:] == -1).all(), kind
        assert np.float32(score) == o_s[b] or (np.isneginf(score) and np.isneginf(o_s[b])), kind
    assert o_l[vc.KINDS.index("stay")] == 1 and o_l[vc.KINDS.index("move")] == T
    dead = vc.KINDS.index("dead")
    assert np.isneginf(o_s[dead]) and o_p[dead, o_l[dead] - 1] == 0          # nothing above -inf: the first state


@pytest.mark.parametrize("nbase,klen", SHAPES)
@pytest.mark.parametrize("mode", vc.MODES)
def test_chunk_kinds_hold_in_every_input_mode(oracle, nbase, klen, mode):
    """all-stay decodes to length 1 and all-move to length T (ragged: its own length) after each mode's transform, at a length
    of several blocks; the tied rows tie after the transform as well."""
    T, B = 70, len(vc.KINDS)
    full, kmer = [16, 35], [15, 63]
    L = vc.scores(T, B, nbase, klen, seed=7 + klen, tied_full=full, tied_kmer=kmer, log_mode=mode == "log")
    nst = L.shape[2]
    if mode == "logits":
        buf, stats, ld = vc.logits_of(L, seed=3, ld=nst + 5)
        lp = vc.numpy_log_post(mode, buf, stats, nst).reshape(T, B, nst)
    else:
        lp = vc.numpy_log_post(mode, L if mode == "log" else vc.softmax(L))
    tied = vc.KINDS.index("tied")
    for t in full:
        assert (lp[t, tied] == lp[t, tied, 0]).all()
    for t in kmer:
        assert (lp[t, tied, 1:] == lp[t, tied, 1]).all() and lp[t, tied, 0] != lp[t, tied, 1]
    if mode == "log":
        ninf = np.isneginf(lp[:, vc.KINDS.index("ninf")]).mean()
        assert 0.25 < ninf < 0.35
    lens = vc.ragged_lengths(T, B, [16, 17, 33])
    for ln in (None, lens):
        for skip in (0.0, 2.5):
            s, p, n = vc.expected(oracle, lp, klen, skip, nbase, ln)
            assert n[vc.KINDS.index("stay")] == 1
            assert n[vc.KINDS.index("move")] == (T if ln is None else ln[vc.KINDS.index("move")])
            assert (p[np.arange(T)[None, :] >= n[:, None]] == -1).all()
    assert lens[0] == T and 1 in lens and 2 in lens and lens[vc.KINDS.index("move")] > 2


def test_poison_and_logit_layout():
    T, B = 9, 4
    L = vc.scores(T, B, 4, 3, seed=1, log_mode=False)
    buf, stats, ld = vc.logits_of(L, seed=2, ld=80)
    assert buf.shape == (T * B, 80) and np.isnan(buf[:, 65:]).all() and np.isfinite(buf[:, :65]).all()
    np.testing.assert_array_equal(stats[:, 0], buf[:, :65].max(axis=1))
    lens = np.asarray([9, 1, 4, 2], dtype=np.int32)
    vc.poison(buf, stats, lens, T, B)
    b3 = buf.reshape(T, B, 80)
    for b in range(B):
        assert np.isfinite(b3[:lens[b], b, :65]).all() and np.isnan(b3[lens[b]:, b]).all()
        assert np.isfinite(stats.reshape(T, B, 2)[:lens[b], b]).all() and np.isnan(stats.reshape(T, B, 2)[lens[b]:, b]).all()


def test_edge_length_lists():
    assert vc.walker_lengths(24) == [24, 25, 26, 49, 50, 73, 74, 98]
    assert vc.walker_lengths(3) == [3, 4, 5, 7, 8, 10, 11, 14]
    assert vc.blank_lengths(64) == [63, 64, 65, 66, 128, 129]
    assert vc.staging_lengths(16) == [2, 15, 16, 17, 18, 31, 32, 33]


# ---- the plan query (host only) ----------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module", autouse=True)
def built():
    from sloika_amd import build
    return build.build()


def test_plan_kernel_choice_on_both_sides_of_the_batch_threshold():
    for klen in (3, 4, 5):
        thr = vc.wave_threshold(klen)
        below, at = vc.plan(vc.LONG, thr - 1, 4, klen), vc.plan(vc.LONG, thr, 4, klen)
        assert below.kernel == vc.WORKGROUP4 and below.staged_rows == 16 and below.blank_steps == max(64, 4 ** klen // 4)
        assert at.kernel == vc.WAVE4 and at.staged_rows == 0 and at.blank_steps == 64
        # same traceback, same walker
        assert below[3:] == at[3:]
    # 4^6 k-mers do not fit a wave's LDS share: the workgroup kernel at every batch size
    assert vc.plan(vc.LONG, 1 << 16, 4, 6).kernel == vc.WORKGROUP4 and vc.plan(vc.LONG, 1 << 16, 4, 6).blank_steps == 1024
    for klen in (3, 4, 5):
        p = vc.plan(vc.LONG, 1 << 16, 5, klen)
        assert p.kernel == vc.GENERIC and p.blank_steps == 0 and p.staged_rows == 0


@pytest.mark.parametrize("nbase,klen,rowbytes,dma", [(4, 3, 32, 1), (4, 4, 128, 1), (4, 5, 512, 1), (4, 6, 2048, 1),
                                                     (5, 3, 125, 0), (5, 4, 625, 0), (5, 5, 3125, 0)])
def test_plan_walker_blocks(nbase, klen, rowbytes, dma):
    """Packed traceback: a 16-bit word per four states; generic: a byte per state.  The walker stages 12288 bytes per block."""
    p = vc.plan(vc.LONG, 3, nbase, klen)
    assert p.tb_row_bytes == rowbytes and p.walker_rows == 12288 // rowbytes and p.walker_dma == dma
    # a chunk shorter than a block: the block is the chunk
    assert vc.plan(2, 3, nbase, klen).walker_rows == 2 and vc.plan(1, 3, nbase, klen).walker_rows == 1
    assert vc.plan(p.walker_rows + 1, 3, nbase, klen).walker_rows == p.walker_rows
    # a workspace that is not 16-byte aligned: no DMA, everything else unchanged
    for align in (1, 4, 8):
        q = vc.plan(vc.LONG, 3, nbase, klen, ws_align=align)
        assert q.walker_dma == 0 and q[:5] == p[:5]
    assert vc.plan(vc.LONG, 3, nbase, klen, ws_align=256) == p


def test_plan_argument_errors():
    import ctypes
    from sloika_amd import _lib
    L, p = _lib.lib(), _lib.ViterbiPlan()
    assert L.slk_viterbi_kmer_plan(10, 1, 4, 5, 16, None) == _lib.SLK_ERR_INVALID_ARG
    for args in ((0, 1, 4, 5, 16), (10, 0, 4, 5, 16), (10, 1, 4, 2, 16), (10, 1, 4, 7, 16), (10, 1, 4, 5, 0), (10, 1, 4, 5, 12)):
        assert L.slk_viterbi_kmer_plan(*args, ctypes.byref(p)) == _lib.SLK_ERR_INVALID_ARG, args
    assert L.slk_viterbi_kmer_plan(10, 1, 3, 5, 16, ctypes.byref(p)) == _lib.SLK_ERR_UNSUPPORTED      # nbase 4 and 5 only
    assert L.slk_viterbi_kmer_plan(10, 1, 5, 6, 16, ctypes.byref(p)) == _lib.SLK_ERR_INVALID_ARG      # 5^6 k-mers: too many
