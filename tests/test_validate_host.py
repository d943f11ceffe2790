"""Host logic of sloika_amd/validate.py that needs no GPU: label preparation against a literal restatement of
bin/validate_network.py:38-43, 70-73, the batching arithmetic of :75-110 with a stub step, the rank reduction on two gloo ranks, the
argument checks, the C ABI's new names, and the fixture tests/golden/validate.npz against a float64 numpy forward pass."""
import json
import os
import socket
import sys

import numpy as np
import pytest

from tests.conftest import GOLDEN, ROOT

if GOLDEN not in sys.path:
    sys.path.insert(0, GOLDEN)
import layer_cases as lc  # noqa: E402
import validate_cases as vc  # noqa: E402


def _reference_labels(labels, bad, transducer, bad_state):
    """validate_network.py:38-43 and :70-73 written out literally (with `bad` as the boolean mask the line was written for)."""
    labels = np.array(labels, dtype=np.int32)
    if not transducer:
        for lbl_ch in labels:
            for i in range(1, len(lbl_ch)):
                if lbl_ch[i] == 0:
                    lbl_ch[i] = lbl_ch[i - 1]
    if bad_state:
        for i in range(labels.shape[0]):
            for j in range(labels.shape[1]):
                if bad[i][j]:
                    labels[i][j] = 0
    return labels


@pytest.mark.parametrize("transducer", [True, False])
@pytest.mark.parametrize("bad_state", [True, False])
def test_prepare_validation_labels(transducer, bad_state):
    from sloika_amd import train, validate
    assert validate.remove_blanks is train.remove_blanks
    rs = np.random.RandomState(5)
    labels = rs.randint(0, 6, size=(7, 11)).astype(np.int32)
    labels[rs.uniform(size=labels.shape) < 0.5] = 0
    labels[0, 0], labels[1, :3] = 0, 0                                   # blanks at the start of a row stay blanks
    bad = (rs.uniform(size=labels.shape) < 0.2).astype('i1')             # int8, as the chunk file holds it
    keep = labels.copy()
    got = validate.prepare_validation_labels(labels, bad, transducer=transducer, bad_state=bad_state)
    assert got.dtype == np.int32 and np.array_equal(got, _reference_labels(keep, bad, transducer, bad_state))
    assert np.array_equal(labels, keep)                                  # the caller's array is left alone


class _StubNet(object):
    size = 9


class _StubStep(object):
    """fv whose answers depend on the batch it is shown, and which records the shapes it saw."""

    def __init__(self):
        self.seen = []

    def __call__(self, x, labels):
        self.seen.append((x.shape, labels.shape, float(x[0, 0, 0]), int(labels[0, 0])))
        assert x.flags["C_CONTIGUOUS"] and labels.flags["C_CONTIGUOUS"]
        return 0.25 + float(x[0, 0, 0]), int(labels.sum() % 7)


def _data(n, clen=6, llen=3, nfeat=2):
    chunks = np.zeros((n, clen, nfeat), dtype=np.float32)
    chunks[:, 0, 0] = np.arange(n)                                       # chunk id in its first sample
    labels = (np.arange(n * llen).reshape(n, llen) % 8 + 1).astype(np.int32)
    return {"chunks": chunks, "labels": labels, "bad": np.zeros((n, llen), dtype='i1')}


def test_validate_network_batching_arithmetic():
    from sloika_amd import validate
    data, step, lines = _data(23), _StubStep(), []
    res = validate.validate_network(_StubNet(), data, batch=5, bad=False, report=lines.append, step=step)
    # 23 // 5 = 4 whole batches, the last 3 chunks dropped; transposes of validate_network.py:83-84
    assert len(step.seen) == 4 and all(s[0] == (6, 5, 2) and s[1] == (3, 5) for s in step.seen)
    assert [s[2] for s in step.seen] == [0.0, 5.0, 10.0, 15.0] and [s[3] for s in step.seen] == [int(data["labels"][5 * k, 0]) for k in range(4)]
    losses = [0.25 + 5.0 * k for k in range(4)]
    counts = [int(data["labels"][5 * k: 5 * k + 5].sum() % 7) for k in range(4)]
    assert res["nbatch"] == 4 and res["nev"] == 4 * 15 and res["ncorrect"] == sum(counts) and isinstance(res["ncorrect"], int)
    assert res["score"] == sum(losses) / 4 and res["accuracy"] == sum(counts) / 60 and res["seconds"] > 0.0
    assert len(lines) == 1 and lines[0].startswith("\nFinal ") and lines[0].endswith(" kev/s)\n")
    assert lines[0].startswith('\nFinal {:5.3f}  {:5.2f}%  '.format(res["score"], 100.0 * res["ncorrect"] / res["nev"]))   # (:110's own form)


def test_validate_network_progress_lines_and_bad_state():
    from sloika_amd import validate
    data, step, lines = _data(101, llen=2), _StubStep(), []
    data["bad"][:, 0] = 1
    res = validate.validate_network(_StubNet(), data, batch=1, report=lines.append, step=step)
    assert res["nbatch"] == 101 and [s[3] for s in step.seen] == [0] * 101       # bad positions went to state 0
    assert len(lines) == 3 and lines[2].startswith("\nFinal ")
    for k, line in enumerate(lines[:2]):
        n = 50 * (k + 1)
        score, acc = sum(0.25 + i for i in range(n)) / n, sum(int(data["labels"][i, 1] % 7) for i in range(n))
        assert line.startswith(' {:5d} {:5.3f}  {:5.2f}%  '.format(k + 1, score, 100.0 * acc / (2 * n))) and line.endswith(" kev/s)\n")


def test_validate_network_argument_checks(tmp_path):
    from sloika_amd import layers, validate
    with pytest.raises(ValueError):                                      # not one whole batch
        validate.validate_network(_StubNet(), _data(4), batch=5, step=_StubStep())
    data = _data(10)
    data["labels"][7, 1] = 9
    with pytest.raises(ValueError, match=r"labels must lie in \[0, 9\)"):
        validate.validate_network(_StubNet(), data, batch=5, step=_StubStep())
    data["labels"][7, 1] = -1
    with pytest.raises(ValueError, match=r"labels must lie in \[0, 9\)"):
        validate.validate_network(_StubNet(), data, batch=5, step=_StubStep())
    # a label out of range among the dropped remainder does not matter, and a path is read with train.load_chunk_file
    data = _data(11)
    data["labels"][10, 0] = 50
    path = os.path.join(str(tmp_path), "held_out.npz")
    np.savez(path, weights=np.ones(11, dtype=np.float32), **data)
    assert validate.validate_network(_StubNet(), path, batch=5, step=_StubStep())["nbatch"] == 2
    for net in (layers.Serial([layers.Gru(4, 16)]), layers.Gru(4, 16), layers.Serial([layers.Softmax(4, 5), layers.FeedForward(5, 5)])):
        with pytest.raises(NotImplementedError, match="needs a Softmax output layer"):
            validate.wrap_network(net)
    # no training refusal is inherited: a Gru of 150 units is accepted here and refused by the training step's plan
    from sloika_amd import train
    wide = layers.Serial([layers.Gru(4, 150), layers.Softmax(150, 5)])
    assert isinstance(validate.wrap_network(wide), validate.ValidationStep)
    with pytest.raises(NotImplementedError):
        train._plan(wide)


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _sum_worker(rank, world, port, out_dir):
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    import torch.distributed as dist
    from sloika_amd import validate
    dist.init_process_group("gloo", rank=rank, world_size=world)
    # the sums alone, then the loop: rank r takes batches r, r + world, ... and every rank returns the global figures
    sums = validate.allreduce_validation_sums(0.1 + rank, 3 + rank, 2 ** 40 + rank, 2 ** 41 + 7 * rank)
    step = _StubStep()
    res = validate.validate_network(_StubNet(), _data(23), batch=5, bad=False, step=step)
    with open(os.path.join(out_dir, "r%d.json" % rank), "w") as fh:
        json.dump({"sums": sums, "res": {k: v for k, v in res.items() if k != "seconds"}, "first": [s[2] for s in step.seen]}, fh)
    dist.barrier()
    dist.destroy_process_group()


def test_rank_reduction_on_two_gloo_ranks(tmp_path):
    import torch.multiprocessing as mp
    from sloika_amd import validate
    assert validate.allreduce_validation_sums(1.5, 2, 3, 4) == (1.5, 2, 3, 4)       # not initialised: a no-op
    mp.spawn(_sum_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    got = [json.load(open(os.path.join(str(tmp_path), "r%d.json" % r))) for r in range(2)]
    single = validate.validate_network(_StubNet(), _data(23), batch=5, bad=False, step=_StubStep())
    for r in range(2):
        assert got[r]["sums"] == [0.1 + 1.1, 7, 2 ** 41 + 1, 2 ** 42 + 7]           # integers stay integers beyond 2^53's reach of a float sum
        assert got[r]["first"] == [5.0 * k for k in range(r, 4, 2)]
        assert got[r]["res"] == {k: v for k, v in single.items() if k != "seconds"}


def test_new_entry_points_are_declared_and_bound():
    from sloika_amd import _lib
    with open(os.path.join(ROOT, "include", "sloika_amd.h")) as fh:
        header = fh.read()
    for name, nargs in (("slk_linear_xent_eval_f16x3", 14), ("slk_softmax_xent_eval_f32", 10), ("slk_reduce_rows_sum_i32", 4)):
        assert "SLK_API int %s(" % name in header
        assert name in _lib.PROTOTYPES and len(_lib.PROTOTYPES[name][1]) == nargs


def test_fixture_is_reproduced_by_a_float64_numpy_forward_pass():
    """tests/golden/validate.npz (the reference's own wrap_network under the stand-in) against oracle_np's forward pass and
    validate_cases.loss_and_count: same labels from the same recipe, loss to float64 rounding, the count exactly wherever no row is
    fragile, and the fragile rows within the share the generator asserted."""
    from oracle import oracle_np
    with open(os.path.join(GOLDEN, "validate_cases.json")) as fh:
        meta = json.load(fh)
    arrays = np.load(os.path.join(GOLDEN, "validate.npz"))
    assert sorted(meta) == sorted(vc.cases())
    kinds = {name: {leaf["type"] for leaf in lc.walk(c["tree"])} for name, c in meta.items()}
    assert any("GRU" in k for k in kinds.values())
    assert any(n["type"] == "parallel" for c in meta.values() for n in c["tree"]["sublayers"])      # a birnn
    for name, c in meta.items():
        want = vc.cases()[name]
        assert c["x"] == want["x"] and c["label_seed"] == want["label_seed"]
        h = [lc.sha(lc.expand(c["x"]))] + [lc.sha(a) for a in lc.param_arrays(c["tree"])]
        assert lc.sha(np.frombuffer("".join(h).encode(), dtype=np.uint8).astype(np.float32)) == c["sha256"]
        post = oracle_np.run_network(lc.materialise(c["tree"], np.float64), lc.expand(c["x"], np.float64))
        labels, gap = arrays[name + "/labels"], arrays[name + "/gap"]
        assert 200 <= labels.size == c["rows"] <= 1000 and labels.dtype == np.int32
        np.testing.assert_allclose(vc.top_two_gap(post), gap, rtol=0, atol=1e-12)
        fragile = gap < vc.FRAGILE_GAP
        assert int(fragile.sum()) == c["fragile_rows"] <= vc.FRAGILE_SHARE * labels.size
        assert np.array_equal(vc.draw_labels(post, c["label_seed"])[~fragile], labels[~fragile])
        np.testing.assert_allclose(vc.loss_rows(post, labels), arrays[name + "/loss_rows"], rtol=1e-10)
        assert np.array_equal(vc.correct_rows(post, labels)[~fragile], arrays[name + "/correct_rows"][~fragile])
        loss, count = vc.loss_and_count(post, labels)
        assert loss == pytest.approx(c["loss"], rel=1e-10) and abs(count - c["ncorrect"]) <= c["fragile_rows"]
        assert int(arrays[name + "/correct_rows"].sum()) == c["ncorrect"]
        assert arrays[name + "/loss_rows"].mean() == pytest.approx(c["loss"], rel=1e-12)
