"""Host side of the decoder of non-transducer models (sloika_amd/olddecode.py, csrc/olddecode.hip): interface, argument checks that
must come before any device call, and the fixture tests/golden/olddecode.npz -- its inputs regenerate to the stored digests, and numpy
still sums a float32 row in the order the kernel restates.  No GPU needed."""
import os
import sys

import numpy as np
import pytest

from tests.conftest import ROOT

GOLDEN = os.path.join(ROOT, "tests", "golden")
if GOLDEN not in sys.path:
    sys.path.insert(0, GOLDEN)
import olddecode_cases as oc  # noqa: E402

NEW_SYMBOLS = ["slk_prepare_post_drop_bad_f32", "slk_estimate_transitions_f64", "slk_decode_profile_workspace_bytes",
               "slk_decode_profile_f64"]


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(os.path.join(GOLDEN, "olddecode.npz")))


@pytest.fixture(scope="module")
def built():
    from sloika_amd import build
    return build.build()


def test_module_and_compat_alias():
    import importlib
    from sloika_amd import compat, olddecode
    for fn in ("decode_profile", "decode_simple", "estimate_transitions", "decode_post_batch"):
        assert callable(getattr(olddecode, fn))
    assert not hasattr(olddecode, "decode_transition")          # raises in the reference; not mirrored
    assert "olddecode" in compat._SUBMODULES
    pkg = compat.install()
    if getattr(pkg, "__sloika_amd_alias__", False):
        assert importlib.import_module("sloika.olddecode") is olddecode


def test_symbols_in_header_library_and_prototypes(built):
    import ctypes
    from sloika_amd import _lib
    with open(os.path.join(ROOT, "include", "sloika_amd.h")) as fh:
        header = fh.read()
    lib = ctypes.CDLL(built)
    for name in NEW_SYMBOLS:
        assert "SLK_API" in header and (name + "(") in header, name
        assert hasattr(lib, name), name
        assert name in _lib.PROTOTYPES, name
    L = _lib.lib()
    # a traceback byte per state and step, the slip sources, the final states
    assert L.slk_decode_profile_workspace_bytes(800, 256, 4, 5) >= 800 * 256 * 1024 + 800 * 256 * 2 + 256 * 4
    for nbase, klen in ((4, 2), (4, 7), (5, 5), (4, 0)):
        assert L.slk_decode_profile_workspace_bytes(800, 4, nbase, klen) == 0
    # the entry points refuse what they have no kernel for before they touch a pointer (host-only calls, no device)
    assert L.slk_decode_profile_f64(None, 4, 1, 4, 5, 1, None, 0.0, None, None, 0, None, None, None, None) == _lib.SLK_ERR_INVALID_ARG
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf) & ~15
    for nbase, klen in ((5, 5), (4, 2), (4, 7)):
        assert L.slk_prepare_post_drop_bad_f32(p, 4, 1, nbase, klen, 1e-5, None, p + 16, p, None, None) == _lib.SLK_ERR_INVALID_ARG
        assert L.slk_estimate_transitions_f64(p, 4, 1, nbase, klen, 0, 0.0, 0.0, 0.0, 1e-10, None, p, None, None) == _lib.SLK_ERR_INVALID_ARG
        assert L.slk_decode_profile_f64(p, 4, 1, nbase, klen, 1, None, 0.0, None, p, 1 << 30, p, p, p, None) == _lib.SLK_ERR_INVALID_ARG


def test_argument_checks_come_before_the_device(monkeypatch):
    """Every refusal below is raised from shapes alone: the device layer is replaced by one that fails the test when reached."""
    from sloika_amd import basecall, device, olddecode, pipeline, layers

    def reached(*a, **k):
        raise AssertionError("the device must not be reached")
    monkeypatch.setattr(device, "to_dev", reached)
    monkeypatch.setattr(device, "device", reached)
    post = np.zeros((6, 1, 1025), dtype=np.float32)
    with pytest.raises(ValueError):
        olddecode.decode_post_batch(post, 5, nbase=5)                                   # basecall.py:48
    for klen in (2, 7):
        with pytest.raises(ValueError):
            olddecode.decode_post_batch(np.zeros((6, 1, 4 ** klen + 1), dtype=np.float32), klen)
    with pytest.raises(ValueError):
        olddecode.decode_post_batch(post, 5, bad=False)                                 # 1025 columns without a bad state
    with pytest.raises(ValueError):
        olddecode.decode_post_batch(post[:, :, :1024], 5, bad=True)
    with pytest.raises(ValueError):
        olddecode.decode_post_batch(post, 5, trans=[0.5, 0.5])
    with pytest.raises(ValueError):
        olddecode.decode_profile(np.zeros((6, 1000), dtype=np.float32))                 # not 4^k states
    with pytest.raises(ValueError):
        olddecode.decode_profile(np.zeros((6, 16), dtype=np.float32))                   # k = 2
    with pytest.raises(ValueError):
        olddecode.decode_profile(np.zeros((0, 1024), dtype=np.float32))                 # the reference: IndexError
    with pytest.raises(ValueError):
        olddecode.decode_profile(np.zeros((6, 1024), dtype=np.float32), trans=np.zeros((4, 3)))     # fewer than T - 1 rows
    with pytest.raises(ValueError):
        olddecode.decode_simple(np.zeros((6, 1, 1024), dtype=np.float32))
    with pytest.raises(ValueError):
        olddecode.estimate_transitions(np.zeros((6, 1024), dtype=np.float32), trans=[1.0])
    with pytest.raises(ValueError):
        olddecode.estimate_transitions(np.zeros((6, 100), dtype=np.float32))
    with pytest.raises(ValueError):
        basecall.decode_post(np.zeros((6, 1, 3126), dtype=np.float32), 5, transducer=False, bad=True, nbase=5)
    with pytest.raises(ValueError):
        basecall.decode_post(post[:, :, :1024], 5, transducer=False, bad=True)
    with pytest.raises(ValueError):
        basecall.decode_post(np.zeros((6, 2, 1025), dtype=np.float32), 5, transducer=False)
    # the Basecaller: what is refused with transducer=False
    net = layers.Serial([layers.FeedForward(4, 8), layers.Softmax(8, 1025)])
    with pytest.raises(NotImplementedError):
        pipeline.Basecaller(net, transducer=False, fused_decode=True)
    with pytest.raises(ValueError):
        pipeline.Basecaller(net, transducer=False, trans=[0.5, 0.5])
    bc = pipeline.Basecaller(net, transducer=False, bad=True, trans=oc.TRANS_PRIOR)
    assert bc.fused_decode is False and bc.trans == oc.TRANS_PRIOR
    with pytest.raises(NotImplementedError):
        bc.call_bases(np.zeros((2, 100), dtype=np.float32))
    with pytest.raises(NotImplementedError):
        next(iter(pipeline.Basecaller.call_batches(net, [np.zeros((2, 100), dtype=np.float32)], transducer=False)))
    for flow, args in ((pipeline.Basecaller.batch_slots, ()), (pipeline.Basecaller.read_lanes, (2,)),
                       (pipeline.Basecaller.run_read_batches, ([], 0)), (pipeline.Basecaller.call_reads_bucketed, ([np.zeros(500)],))):
        with pytest.raises(NotImplementedError):
            flow(net, *args, transducer=False)
    assert pipeline.Basecaller(net).transducer is True                                 # the default stays the transducer decoder


def test_fails_loudly_without_gpu(built):
    import torch
    from sloika_amd import _lib, basecall, decode, olddecode
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    lp, w = oc.log_posterior("t7")
    for call in (lambda: olddecode.decode_profile(lp, trans=w, log=True), lambda: olddecode.decode_simple(lp, log=True),
                 lambda: olddecode.estimate_transitions(np.exp(lp)),
                 lambda: olddecode.decode_post_batch(oc.posterior("t7"), 5, trans=oc.TRANS_PRIOR),
                 lambda: decode.prepare_post(oc.posterior("t7"), drop_bad=True),
                 lambda: basecall.decode_post(oc.posterior("t7"), 5, transducer=False, bad=True)):
        with pytest.raises(_lib.SloikaAmdError):
            call()


def test_file_level_workers_still_refuse():
    """basecall.events_worker / raw_worker keep refusing the non-transducer arguments; the read workers take them."""
    import inspect
    from sloika_amd import basecall
    for fn in (basecall.events_read_worker, basecall.raw_read_worker):
        sig = inspect.signature(fn).parameters
        assert (sig["transducer"].default, sig["bad"].default, sig["trans"].default) == (True, True, None)

    def calc_post(x):
        raise AssertionError("the model must not be reached")
    with pytest.raises(NotImplementedError):
        basecall.raw_worker("no_such_file.fast5", (0, 0), 0.0, 5, False, True, 1e-5, calc_post=calc_post)


def test_fixture_inputs_regenerate(gold):
    assert set(oc.CASES) == {k[:-len("_digest")] for k in gold if k.endswith("_digest")}
    for name, (T, klen, bad, prior, seed, kind) in oc.CASES.items():
        assert np.array_equal(oc.digest(name), gold[name + "_digest"]), "regenerated input of %s differs from the one the reference saw" % name
        post = oc.posterior(name)
        assert post.shape == (T, 1, 4 ** klen + bad) and post.dtype == np.float32
        prep, rows = oc.prepare_np(post, bad)
        assert np.array_equal(rows, gold[name + "_kept"])
        if kind == "allbad":
            assert len(rows) == 0 and name + "_post_path" not in gold
            continue
        assert bad or len(rows) == T
        assert np.array_equal(oc.sha256(prep), gold[name + "_prep_sha"]), name
        assert np.array_equal(prep[oc.row_picks(len(prep))], gold[name + "_prep_rows"])
        assert gold[name + "_trans"].shape == (len(rows), 3) and gold[name + "_trans"].dtype == np.float64
        assert np.abs(gold[name + "_trans"].sum(axis=1) - 1.0).max() < 1e-12
        assert len(gold[name + "_post_path"]) == len(rows)
        for i in range(len(oc.SLIPS)):
            assert len(gold["%s_prof_s%d_path" % (name, i)]) == T and len(gold["%s_simple_s%d_path" % (name, i)]) == T
    # what the issue asks the cases to cover
    rows = sorted(c[0] for c in oc.CASES.values())
    assert {1, 2, 7, 300, 2000} <= set(rows)
    assert {c[1] for c in oc.CASES.values() if c[0] == 50} == {3, 4, 6}
    assert {c[2] for c in oc.CASES.values()} == {True, False} and {str(c[3]) for c in oc.CASES.values()} == {"None", str(oc.TRANS_PRIOR)}
    fragile = [n for n in oc.CASES if name_has(gold, n + "_fragile") and int(gold[n + "_fragile"])]
    assert len(fragile) <= 0.1 * sum(name_has(gold, n + "_fragile") for n in oc.CASES)
    assert 0.0 < float(gold["e_ref"]) < 1e-5 and 0.0 < float(gold["score_rel_ref"]) < 1e-6


def name_has(gold, key):
    return key in gold


def test_tie_cases_do_tie(gold):
    """The quantised cases hold exact ties where the reference's order of candidates decides."""
    for name in ("tie_k3", "tie_k4", "tie_k5"):
        lp, w = oc.log_posterior(name)
        assert np.array_equal(lp * 4, np.round(lp * 4)) and np.array_equal(w * 4, np.round(w * 4))
        # equal neighbours among the step predecessors' scores of step 1 (pscore = lp[0])
        n = lp.shape[1]
        first = lp[0].reshape(4, n // 4)
        assert (np.sum(first == first.max(axis=0), axis=0) > 1).any(), name
        post = oc.posterior(name)[:, 0]
        assert np.array_equal(post * 4096, np.round(post * 4096))


def test_numpy_sums_a_row_in_the_restated_order(gold):
    """decode.prepare_post(drop_bad=True) divides by np.sum(row) in float32; the kernel restates numpy's summation tree.  A numpy that
    sums differently shows up here and not as a mystery on the GPU."""
    assert str(gold["numpy_version"]).split(".")[0] == np.__version__.split(".")[0], \
        "the fixture was made with numpy %s (its float64 promotion and float32 summation order are pinned)" % gold["numpy_version"]
    checked = 0
    for name in ("k3", "k4", "t7", "t300", "k6"):
        T, klen, bad, _, _, _ = oc.CASES[name]
        p = np.squeeze(oc.posterior(name), axis=1)
        kept = p[np.argmax(p, axis=1) > 0, 1:]                     # the fancy-indexed copy the reference sums (decode.py:33-34)
        want = np.sum(kept, axis=1, keepdims=True)
        for r in range(0, len(kept), max(1, len(kept) // 12)):
            got = oc.pairwise_sum32(kept[r])
            assert got.dtype == np.float32 and got.tobytes() == want[r, 0].tobytes(), (name, r)
            checked += 1
    assert checked >= 40
    # ... and the float64 sum rounded once is NOT that value on some row: the tree matters
    p = np.squeeze(oc.posterior("t300"), axis=1)[:, 1:]
    assert (np.sum(p, axis=1) != np.sum(p.astype(np.float64), axis=1).astype(np.float32)).any()


def test_generator_holds_its_caps():
    sys.path.insert(0, GOLDEN)
    import make_olddecode_goldens as gen
    size = os.path.getsize(os.path.join(GOLDEN, "olddecode.npz"))
    largest = max(os.path.getsize(os.path.join(GOLDEN, f)) for f in os.listdir(GOLDEN) if f.endswith(".npz") and f != "olddecode.npz")
    assert size <= min(gen.MAX_BYTES, largest) and gen.MAX_BYTES == 1 << 20 and gen.MAX_FRAGILE == 0.1
