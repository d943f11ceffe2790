"""What the sequence loss decides on the host, without a GPU: the refusals of slk_softmax_seq_grad_f32 (csrc/seq_loss.hip) before it
touches a device, and the arguments train_loop(loss="sequence") turns down before it builds anything.  (design/sequence_loss.md)"""
import ctypes

import pytest


def test_c_entry_refusals():
    from sloika_amd import _lib, build
    build.build()
    L = _lib.lib()
    p = ctypes.c_void_p(256)
    bad, unsupported = _lib.SLK_ERR_INVALID_ARG, _lib.SLK_ERR_UNSUPPORTED
    call = lambda *a: L.slk_softmax_seq_grad_f32(*a)                               # noqa: E731
    assert call(None, 8, p, p, 8, p, p, 3, 2, 5, 0.0, None) == bad
    assert call(p, 8, p, None, 8, p, p, 3, 2, 5, 0.0, None) == bad
    assert call(p, 8, p, p, 8, None, p, 3, 2, 5, 0.0, None) == bad
    assert call(p, 8, p, p, 8, p, p, 3, 2, 1, 0.0, None) == bad                    # nstate < 2
    assert call(p, 4, p, p, 8, p, p, 3, 2, 5, 0.0, None) == bad                    # ld < nstate
    assert call(p, 8, p, p, 4, p, p, 3, 2, 5, 0.0, None) == bad                    # occ_ld < nstate
    assert call(p, 8, p, p, 8, p, p, 3, 2, 5, 1.0, None) == bad                    # min_prob
    assert call(p, 8, p, p, 8, p, p, 3, 2, 5, -1e-3, None) == bad
    assert call(p, 8, p, p, 8, p, p, 0, 2, 5, 0.0, None) == bad
    assert call(p, (1 << 24) + 1, p, p, 8, p, p, 3, 2, 5, 0.0, None) == unsupported   # wider than SLK_SEQ_GRAD_MAX_LD


def test_train_loop_turns_down_what_a_sequence_has_not():
    from sloika_amd import train
    with pytest.raises(ValueError, match="drop"):
        train.train_loop(None, {}, "unused", drop=20, loss="sequence")
    with pytest.raises(ValueError, match="transducer"):
        train.train_loop(None, {}, "unused", drop=0, transducer=False, loss="sequence")
    with pytest.raises(ValueError, match="loss"):
        train.train_loop(None, {}, "unused", loss="ctc")
