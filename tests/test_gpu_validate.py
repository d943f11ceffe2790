"""Validation on the device (sloika_amd/validate.py; slk_linear_xent_eval_f16x3, slk_softmax_xent_eval_f32, slk_reduce_rows_sum_i32):
the statistics pass alone against the training kernel it is cut from (same bits), against float64, the first-maximum rule, the
fallback through logits, the reference's own `fv` (tests/golden/validate.npz), validate_network end to end and train_loop's
validation lines."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.conftest import GOLDEN, ROOT
from tests.gpu_util import need_gpu, dev, stream

if GOLDEN not in sys.path:
    sys.path.insert(0, GOLDEN)
import layer_cases as lc  # noqa: E402
import validate_cases as vc  # noqa: E402

pytestmark = pytest.mark.gpu

LOSS_REL = 2e-5            # of the largest row loss: the loss tolerance of tests/test_gpu_train.py


def _split(torch, L, Wd, N, K):
    from sloika_amd import _lib
    kp = (K + 15) // 16 * 16
    hi = torch.empty((N, kp), dtype=torch.float16, device="cuda")
    lo = torch.empty_like(hi)
    inv = torch.empty(N, dtype=torch.float32, device="cuda")
    _lib.check(L.slk_split_f16x2_f32(Wd.data_ptr(), N, K, hi.data_ptr(), lo.data_ptr(), inv.data_ptr(), stream()), "split")
    return hi, lo, inv


def _problem(K, N, M, seed):
    rs = np.random.RandomState(seed)
    x = rs.normal(size=(M, K)).astype(np.float32)
    W = (rs.normal(size=(N, K)) * 0.4).astype(np.float32)
    b = rs.normal(size=N).astype(np.float32)
    labels = rs.randint(0, N, size=M).astype(np.int32)
    return x, W, b, labels


def _f64(x, W, b, labels):
    """(row loss, correct flag, gap between the two largest logits) of x.W^T + b in float64."""
    logits = x.astype(np.float64) @ W.astype(np.float64).T + b.astype(np.float64)
    mx = logits.max(axis=1, keepdims=True)
    logp = logits - mx - np.log(np.exp(logits - mx).sum(axis=1, keepdims=True))
    top = np.sort(logits, axis=1)[:, -2:]
    return -logp[np.arange(len(labels)), labels], (logits.argmax(axis=1) == labels).astype(np.int32), top[:, 1] - top[:, 0]


def _eval_f16x3(torch, L, xd, hi, lo, inv, bd, K, N, labels_d, T, B, guard=0):
    M = T * B
    loss = torch.full((M + 2 * guard,), -7.0, dtype=torch.float32, device="cuda")
    correct = torch.full((M + 2 * guard,), -7, dtype=torch.int32, device="cuda")
    rc = L.slk_linear_xent_eval_f16x3(xd.data_ptr(), K, hi.data_ptr(), lo.data_ptr(), inv.data_ptr(), bd.data_ptr(), K, N,
                                      labels_d.data_ptr(), T, B, loss[guard:].data_ptr(), correct[guard:].data_ptr(), stream())
    torch.cuda.synchronize()
    return rc, loss, correct


def _eval_f32(torch, L, xd, hi, lo, inv, bd, K, N, labels_d, T, B, guard=0):
    """logits + row statistics (slk_linear_rowstats_f16x3), then slk_softmax_xent_eval_f32; also returns the logits, before and after."""
    from sloika_amd import _lib
    M, ld = T * B, (N + 31) // 32 * 32
    logits = torch.full((M, ld), 7.0, dtype=torch.float32, device="cuda")
    stats = torch.empty((M, 2), dtype=torch.float32, device="cuda")
    _lib.check(L.slk_linear_rowstats_f16x3(xd.data_ptr(), K, hi.data_ptr(), lo.data_ptr(), inv.data_ptr(), bd.data_ptr(),
                                           logits.data_ptr(), ld, M, K, N, stats.data_ptr(), stream()), "rowstats")
    before = logits.clone()
    loss = torch.full((M + 2 * guard,), -7.0, dtype=torch.float32, device="cuda")
    correct = torch.full((M + 2 * guard,), -7, dtype=torch.int32, device="cuda")
    rc = L.slk_softmax_xent_eval_f32(logits.data_ptr(), ld, stats.data_ptr(), labels_d.data_ptr(), T, B, N, loss[guard:].data_ptr(),
                                     correct[guard:].data_ptr(), stream())
    torch.cuda.synchronize()
    assert torch.equal(before, logits)                                 # read only
    return rc, loss, correct, logits


@pytest.mark.parametrize("K,N,T,B", [(64, 1025, 32, 16), (96, 1025, 8, 64), (128, 2048, 4, 32)])
def test_same_arithmetic_as_the_training_kernel(K, N, T, B):
    """slk_linear_xent_grad_f16x3 at min_prob = 0, drop = 0 and unit weights divides each row's loss by T * B, a power of two here: the
    validation kernel's row loss is that term times T * B, bit for bit, and its flag is set where the training term is not zero."""
    torch = need_gpu()
    from sloika_amd import _lib
    L = _lib.lib()
    M, ld = T * B, (N + 31) // 32 * 32
    assert M & (M - 1) == 0
    x, W, b, labels = _problem(K, N, M, K + N + T)
    W[N - 3] = W[2]; b[N - 3] = b[2] = b.max() + 1.0                   # ties for the maximum on many rows, as in the training test
    labels[:M // 4] = 2
    labels[M // 4: M // 2] = N - 3
    xd, bd, ld_ = dev(x), dev(b), dev(labels)
    hi, lo, inv = _split(torch, L, dev(W), N, K)
    ones = torch.ones(M, dtype=torch.float32, device="cuda")
    grad = torch.empty((M, ld), dtype=torch.float32, device="cuda")
    rows = torch.empty((2, M), dtype=torch.float32, device="cuda")
    xrow = torch.empty((M, 4), dtype=torch.float32, device="cuda")
    _lib.check(L.slk_linear_xent_grad_f16x3(xd.data_ptr(), K, hi.data_ptr(), lo.data_ptr(), inv.data_ptr(), bd.data_ptr(), grad.data_ptr(), ld,
                                            K, N, ld_.data_ptr(), ones.data_ptr(), T, B, 0, 0.0, rows[0].data_ptr(), rows[1].data_ptr(),
                                            xrow.data_ptr(), stream()), "two passes")
    rc, loss, correct = _eval_f16x3(torch, L, xd, hi, lo, inv, bd, K, N, ld_, T, B)
    assert rc == 0
    assert torch.equal(loss, rows[0] * float(M))
    assert torch.equal(correct, (rows[1] != 0).to(torch.int32))
    assert 0 < int(correct.sum()) < M


@pytest.mark.parametrize("K,N,T,B", [(64, 1025, 5, 7), (112, 257, 3, 37)])
def test_row_terms_against_float64_and_no_row_beyond_m(K, N, T, B):
    torch = need_gpu()
    from sloika_amd import _lib
    L = _lib.lib()
    M, G = T * B, 64
    x, W, b, labels = _problem(K, N, M, K + N)
    want_loss, want_correct, gap = _f64(x, W, b, labels)
    labels[gap.argmax()] = int((x[gap.argmax()].astype(np.float64) @ W.astype(np.float64).T + b).argmax())   # at least one correct row
    want_loss, want_correct, gap = _f64(x, W, b, labels)
    hi, lo, inv = _split(torch, L, dev(W), N, K)
    rc, loss, correct = _eval_f16x3(torch, L, dev(x), hi, lo, inv, dev(b), K, N, dev(labels), T, B, guard=G)
    assert rc == 0
    loss, correct = loss.cpu().numpy(), correct.cpu().numpy()
    err = np.abs(loss[G:G + M].astype(np.float64) - want_loss).max()
    print("K %d N %d: largest row-loss error %.3g of largest row loss %.3g (allowed %.3g)" % (K, N, err, want_loss.max(), LOSS_REL * want_loss.max()))
    assert err <= LOSS_REL * want_loss.max()
    sure = gap > 1e-4                                                  # (float32 logits of size ~10 carry ~1e-6: a wide margin)
    assert sure.sum() > 0.9 * M and np.array_equal(correct[G:G + M][sure], want_correct[sure]) and want_correct.sum() >= 1
    assert set(np.unique(correct[G:G + M])) <= {0, 1}
    assert (loss[:G] == -7.0).all() and (loss[G + M:] == -7.0).all() and (correct[:G] == -7).all() and (correct[G + M:] == -7).all()
    # shapes outside the instantiated widths are refused, not computed some other way
    rc, _, _ = _eval_f16x3(torch, L, dev(x), hi, lo, inv, dev(b), 32, N, dev(labels), T, B)
    assert rc == _lib.SLK_ERR_UNSUPPORTED


@pytest.mark.parametrize("path", ["f16x3", "f32"])
def test_first_maximum_wins(path):
    """Two identical weight rows j < k with identical biases give the same logit bits; x is scaled so that they are the row maximum:
    label k scores 0 and label j scores 1 on every row (T.argmax returns the first maximum)."""
    torch = need_gpu()
    from sloika_amd import _lib
    L = _lib.lib()
    K, N, T, B, j, k = 96, 1025, 6, 25, 130, 900                      # (j and k in different 64-column tiles and column waves)
    M = T * B
    x, W, b, _ = _problem(K, N, M, 11)
    W[k] = W[j]; b[k] = b[j] = 0.5
    x = (0.1 * x + 3.0 * W[j] / np.linalg.norm(W[j])).astype(np.float32)       # x . W[j] ~ 3 |W[j]| ~ 12, the others ~ N(0, 4)
    for lab, want in ((k, 0), (j, 1)):
        labels = np.full(M, lab, dtype=np.int32)
        hi, lo, inv = _split(torch, L, dev(W), N, K)
        if path == "f16x3":
            rc, loss, correct = _eval_f16x3(torch, L, dev(x), hi, lo, inv, dev(b), K, N, dev(labels), T, B)
            _, _, _, logits = _eval_f32(torch, L, dev(x), hi, lo, inv, dev(b), K, N, dev(labels), T, B)
        else:
            rc, loss, correct, logits = _eval_f32(torch, L, dev(x), hi, lo, inv, dev(b), K, N, dev(labels), T, B)
        assert rc == 0
        lg = logits[:, :N]
        assert torch.equal(lg[:, j], lg[:, k]) and torch.equal(lg.max(dim=1).values, lg[:, j])     # the tie IS the maximum, same bits
        assert (correct == want).all(), (lab, int(correct.sum()))
        assert torch.isfinite(loss).all()


def _net_loss_f64(net, x, labels):
    """Row losses and flags in float64 from the float64 oracle's posterior of `net`."""
    from oracle import oracle_np
    post = oracle_np.run_network(net.spec(), np.asarray(x, dtype=np.float64))
    return vc.loss_rows(post, labels), vc.correct_rows(post, labels), vc.top_two_gap(post)


def test_fallback_small_k():
    """(K, N) = (24, 17): the split kernel refuses, ValidationStep goes through logits + slk_softmax_xent_eval_f32."""
    torch = need_gpu()
    from sloika_amd import _lib, layers, validate
    rs = np.random.RandomState(24)
    init = lambda shape: rs.normal(size=shape).astype(np.float32)
    net = layers.Serial([layers.Softmax(24, 17, init=init, has_bias=True)])
    net.layers[0].W.set_value((3.0 * rs.normal(size=(17, 24)) / np.sqrt(24)).astype(np.float32))
    T, B = 5, 7
    x = rs.normal(size=(T, B, 24)).astype(np.float32)
    labels = rs.randint(0, 17, size=(T, B)).astype(np.int32)
    hi, lo, inv = net.layers[0]._split_weights()
    L = _lib.lib()
    rc, _, _ = _eval_f16x3(torch, L, dev(x), hi, lo, inv, net.layers[0].b.dev(), 24, 17, dev(labels), T, B)
    assert rc == _lib.SLK_ERR_UNSUPPORTED
    step = validate.wrap_network(net)
    loss, ncorrect = step(x, labels)
    want_loss, want_correct, gap = _net_loss_f64(net, x, labels)
    err = np.abs(step.loss_rows.cpu().numpy().astype(np.float64) - want_loss).max()
    print("fallback (24, 17): largest row-loss error %.3g, allowed %.3g" % (err, LOSS_REL * want_loss.max()))
    assert err <= LOSS_REL * want_loss.max() and loss == pytest.approx(want_loss.mean(), rel=LOSS_REL)
    assert isinstance(ncorrect, int) and isinstance(loss, float)
    sure = gap > vc.FRAGILE_GAP
    assert np.array_equal(step.correct_rows.cpu().numpy()[sure], want_correct[sure]) and abs(ncorrect - want_correct.sum()) <= (~sure).sum()
    with pytest.raises(ValueError, match=r"labels must lie in \[0, 17\)"):      # checked before the row is indexed with the label
        bad = labels.copy()
        bad[2, 3] = 17
        step(x, bad)
    with pytest.raises(ValueError):
        step(x, labels[:-1])
    with pytest.raises(ValueError):
        step(x[:, :, :5], labels)


_CHILD = r"""
import json, sys
sys.path.insert(0, %(root)r); sys.path.insert(0, %(golden)r)
import numpy as np
import layer_cases as lc, validate_cases as vc
from tests import ref_layers
from sloika_amd import layers, validate
assert layers.SPLIT_F16 is False
c = vc.cases()["softmax_1025"]
net = ref_layers.build_amd(c["tree"])
assert net.layers[-1].split_f16 is False
labels = np.load(%(npz)r)["softmax_1025/labels"]
step = validate.wrap_network(net)
loss, ncorrect = step(lc.expand(c["x"]), labels)
print(json.dumps({"loss": loss, "ncorrect": ncorrect, "loss_rows": step.loss_rows.cpu().numpy().astype(float).tolist(),
                  "correct_rows": step.correct_rows.cpu().numpy().tolist()}))
"""


def test_fallback_exact_f32_in_a_child_process():
    """SLOIKA_AMD_EXACT_F32=1 (read once at import): the 96 -> 1025 output layer goes through fp32 logits + slk_softmax_xent_eval_f32."""
    need_gpu()
    npz = os.path.join(GOLDEN, "validate.npz")
    r = subprocess.run([sys.executable, "-c", _CHILD % {"root": ROOT, "golden": GOLDEN, "npz": npz}], cwd=ROOT,
                       env=dict(os.environ, SLOIKA_AMD_EXACT_F32="1"), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    got = json.loads(r.stdout.strip().splitlines()[-1])
    arrays = np.load(npz)
    want, gap = arrays["softmax_1025/loss_rows"], arrays["softmax_1025/gap"]
    err = np.abs(np.asarray(got["loss_rows"]) - want).max()
    print("exact-f32 fallback: largest row-loss error %.3g, allowed %.3g" % (err, LOSS_REL * want.max()))
    assert err <= LOSS_REL * want.max() and got["loss"] == pytest.approx(want.mean(), rel=LOSS_REL)
    sure = gap >= vc.FRAGILE_GAP
    assert np.array_equal(np.asarray(got["correct_rows"])[sure], arrays["softmax_1025/correct_rows"][sure])
    assert abs(got["ncorrect"] - int(arrays["softmax_1025/correct_rows"].sum())) <= int((~sure).sum())


@pytest.mark.parametrize("name", sorted(vc.cases()))
def test_end_to_end_against_the_reference_fixture(name):
    """validate.wrap_network(net)(x, labels) against what bin/validate_network.py:wrap_network returned for the same network (float64,
    under the stand-in): loss within 2e-5; the flags equal on every row that is not fragile (top-two posterior gap >= 2e-4, twice the
    1e-4 allowed on posteriors), the count within the number of fragile rows."""
    need_gpu()
    from sloika_amd import validate
    from tests import ref_layers
    with open(os.path.join(GOLDEN, "validate_cases.json")) as fh:
        c = json.load(fh)[name]
    arrays = np.load(os.path.join(GOLDEN, "validate.npz"))
    labels, gap, ref_flags = arrays[name + "/labels"], arrays[name + "/gap"], arrays[name + "/correct_rows"]
    ref_layers.check_inputs(c)
    net = ref_layers.build_amd(c["tree"])
    step = validate.wrap_network(net)
    loss, ncorrect = step(lc.expand(c["x"]), labels)
    fragile = gap < vc.FRAGILE_GAP
    assert fragile.sum() <= vc.FRAGILE_SHARE * gap.size
    flags = step.correct_rows.cpu().numpy()
    print("%s: loss %.9g (reference %.9g, rel %.3g), ncorrect %d (reference %d), fragile rows %d, flags differing %d" % (
        name, loss, c["loss"], abs(loss - c["loss"]) / c["loss"], ncorrect, c["ncorrect"], fragile.sum(), (flags != ref_flags).sum()))
    assert loss == pytest.approx(c["loss"], rel=LOSS_REL)
    assert isinstance(ncorrect, int) and ncorrect == int(flags.sum())
    assert np.array_equal(flags[~fragile], ref_flags[~fragile])
    assert abs(ncorrect - c["ncorrect"]) <= int(fragile.sum())


def _raw_gru(rs, n=32, nstate=9, width=None):
    from sloika_amd import activation, layers
    init = lambda shape: (rs.normal(size=shape) * 0.4).astype(np.float32)
    width = n if width is None else width
    return layers.Serial([layers.Convolution(1, n, 5, 2, init=init, has_bias=True, fun=activation.elu),
                          layers.Reverse(layers.Gru(n, width, init=init, has_bias=True)), layers.Gru(width, n, init=init, has_bias=True),
                          layers.Softmax(n, nstate, init=init, has_bias=True)])


def _chunk_data(rs, n, clen, llen, nfeat, nstate):
    labels = rs.randint(1, nstate, size=(n, llen)).astype(np.int32)
    labels[rs.uniform(size=labels.shape) < 0.4] = 0
    return {"chunks": rs.normal(size=(n, clen, nfeat)).astype(np.float32), "labels": labels,
            "bad": (rs.uniform(size=labels.shape) < 0.1).astype('i1')}


@pytest.mark.parametrize("model", ["tiny_gru", "raw_gru"])
@pytest.mark.parametrize("transducer,bad", [(True, True), (False, False)])
def test_validate_network_end_to_end(model, transducer, bad):
    """5 batches of 16 chunks (3 more dropped): the figures are those assembled from fv batch by batch."""
    need_gpu()
    from sloika_amd import models, validate
    rs = np.random.RandomState(6)
    if model == "tiny_gru":
        net = models.randomise_zero_layers(models.build_model("tiny_gru", klen=3, sd=0.5, seed=5))
        data = _chunk_data(rs, 83, 30, 30, net.insize, net.size)
    else:
        net = _raw_gru(rs)
        data = _chunk_data(rs, 83, 60, 30, 1, net.size)
    lines = []
    res = validate.validate_network(net, data, batch=16, transducer=transducer, bad=bad, report=lines.append)
    fv = validate.wrap_network(net)
    labels = validate.prepare_validation_labels(data["labels"], data["bad"], transducer, bad)
    losses, counts = [], []
    for k in range(5):
        sl = slice(16 * k, 16 * k + 16)
        loss, n = fv(np.ascontiguousarray(data["chunks"][sl].transpose(1, 0, 2)), np.ascontiguousarray(labels[sl].T))
        losses.append(loss)
        counts.append(n)
    score = 0.0
    for v in losses:
        score += v
    assert res["nbatch"] == 5 and res["nev"] == 5 * 16 * 30 and res["ncorrect"] == sum(counts)
    assert res["score"] == score / 5 and res["accuracy"] == sum(counts) / float(res["nev"])
    # the percentage as validate_network.py:110 forms it, 100.0 * acc / wacc from the integer sums: 100.0 * (acc / wacc) can round to
    # the other side of a half (345 of 2400: 14.375 exactly against 14.374999...)
    assert len(lines) == 1 and lines[0].startswith('\nFinal {:5.3f}  {:5.2f}%  '.format(res["score"], 100.0 * res["ncorrect"] / res["nev"]))
    # the same batch against the device's own posterior (Layer.run), in float64
    import torch
    post = net.run(torch.from_numpy(np.ascontiguousarray(data["chunks"][:16].transpose(1, 0, 2))).cuda()).cpu().numpy()
    want, _ = vc.loss_and_count(post, labels[:16].T)
    assert losses[0] == pytest.approx(want, rel=LOSS_REL)


def test_out_of_range_labels_raise_and_wide_gru_validates():
    need_gpu()
    import torch
    from sloika_amd import train, validate
    rs = np.random.RandomState(7)
    net = _raw_gru(rs, n=64, nstate=40)                                 # K = 64: the split kernel, which only compares columns
    data = _chunk_data(rs, 32, 60, 30, 1, net.size)
    fv = validate.wrap_network(net)
    x, labels = np.ascontiguousarray(data["chunks"][:16].transpose(1, 0, 2)), np.ascontiguousarray(data["labels"][:16].T)
    loss, _ = fv(x, labels)
    for value in (40, -1):
        wrong = labels.copy()
        wrong[7, 3] = value
        with pytest.raises(ValueError, match=r"labels must lie in \[0, 40\)"):
            fv(x, wrong)
    assert fv(x, labels)[0] == loss                                      # ... and the step is usable afterwards
    data["labels"][20, 5] = 40
    with pytest.raises(ValueError, match=r"labels must lie in \[0, 40\)"):
        validate.validate_network(net, data, batch=16, bad=False)
    # a Gru of 150 units has no reverse scan (training refuses it) and validates
    wide = _raw_gru(rs, n=32, nstate=9, width=150)
    with pytest.raises(NotImplementedError):
        train.wrap_network(wide)
    data = _chunk_data(rs, 16, 60, 30, 1, wide.size)
    res = validate.validate_network(wide, data, batch=16)
    labels = validate.prepare_validation_labels(data["labels"], data["bad"])
    post = wide.run(torch.from_numpy(np.ascontiguousarray(data["chunks"].transpose(1, 0, 2))).cuda()).cpu().numpy()
    want, _ = vc.loss_and_count(post, labels.T)
    assert res["score"] == pytest.approx(want, rel=LOSS_REL) and 0 <= res["ncorrect"] <= res["nev"] == 16 * 30


def _strip_times(log):
    import re
    return re.sub(r"[ \d.]+s \([\d.]+ kev/s\)", " <time>", log)


def test_train_loop_validation_lines(tmp_path):
    """The toy task of tests/test_gpu_train.py (label = quantised local signal level, half of the positions blank) with held-out chunks:
    one `* Validation` line every `validate_every` iterations, accuracy rising; without the arguments the log is the one of a run
    without them for the same seed (timings aside), and with them the other lines are those."""
    need_gpu()
    from sloika_amd import activation, layers, train

    def toy(seed, n):
        rs = np.random.RandomState(seed)
        clen, stride = 200, 2
        level = rs.randint(1, 5, size=(n, clen // stride))
        chunks = (np.repeat(level, stride, axis=1).astype(np.float32) - 2.5 + 0.1 * rs.normal(size=(n, clen)))[:, :, None]
        labels = level.astype(np.int32)
        labels[:, 1::2] = 0
        chunks[:, 2::4, 0] += 3.0
        chunks[:, 3::4, 0] += 3.0
        return {"chunks": chunks.astype(np.float32), "labels": labels, "bad": np.zeros_like(labels, dtype='i1'),
                "weights": np.ones(n, dtype='float64'), "kmer": 1, "alphabet": b"ACGT"}

    def net():
        rs = np.random.RandomState(4)
        init = lambda shape: (rs.normal(size=shape) * 0.3).astype(np.float32)
        return layers.Serial([layers.Convolution(1, 32, 5, 2, init=init, has_bias=True, fun=activation.elu),
                              layers.Reverse(layers.Gru(32, 32, init=init, has_bias=True)), layers.Gru(32, 32, init=init, has_bias=True),
                              layers.Softmax(32, 5, init=init, has_bias=True)])

    logs = {}
    for tag, extra in (("plain", {}), ("validated", dict(validation=toy(33, 32), validate_every=40))):
        out = os.path.join(str(tmp_path), tag)
        train.train_loop(net(), toy(3, 64), out, niteration=120, batch_size=32, drop=4, adam=(4e-3, 0.9, 0.999), save_every=100, seed=9,
                         quiet=True, **extra)
        logs[tag] = open(os.path.join(out, "model.log")).read()
    assert "Validation" not in logs["plain"]
    vlines = [l for l in logs["validated"].splitlines() if l.startswith("* Validation")]
    assert len(vlines) == 3 and [int(l.split()[2]) for l in vlines] == [40, 80, 120]
    pct = lambda line: float([tok for tok in line.split() if tok.endswith("%")][0].rstrip("%"))
    print("validation accuracy over the run:", [pct(l) for l in vlines])
    assert pct(vlines[-1]) > pct(vlines[0])
    rest = "\n".join(l for l in logs["validated"].split("\n") if not l.startswith("* Validation"))
    # (a validation line that does not follow a progress line starts on a line of its own: that newline goes with it)
    assert _strip_times(rest).replace("\n", "") == _strip_times(logs["plain"]).replace("\n", "")
