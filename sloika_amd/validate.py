"""Score a trained network on held-out chunks: loss and accuracy, forward only (bin/validate_network.py).

`wrap_network(network)` returns `fv(x, labels) -> (loss, ncorrect)` like the Theano function of validate_network.py:46-54: the mean
categorical cross-entropy over all positions and the NUMBER of positions whose arg-max is the label.  The layers in front of the
output layer run on the inference kernels exactly as pipeline.Basecaller runs them -- no tape, no saved gates, none of the training
step's refusals -- and the final Softmax goes through csrc/gemm_rows_f16x3.hip's statistics pass alone (slk_linear_xent_eval_f16x3:
no logits tensor, no gradient) or, for the shapes that kernel does not take and under SLOIKA_AMD_EXACT_F32=1, through logits + row
statistics and slk_softmax_xent_eval_f32.  The loss sum is a fixed-order float64 reduction, the count an integer end to end.

`validate_network(network, data, ...)` is the loop of validate_network.py:75-110 over a chunk file (train.load_chunk_file).  There is
no CPU fallback.
"""
import time

import numpy as np

from . import _lib, layers, profiler
from .train import rank_and_world, remove_blanks  # noqa: F401  (remove_blanks: validate_network.py:38-43, re-exported)

PROGRESS_LINE = ' {:5d} {:5.3f}  {:5.2f}%  {:5.2f}s ({:.2f} kev/s)\n'          # validate_network.py:102
FINAL_LINE = '\nFinal {:5.3f}  {:5.2f}%  {:5.2f}s ({:.2f} kev/s)\n'             # validate_network.py:109


class ValidationStep(object):
    """fv(x, labels) -> (loss, ncorrect).

    x      : [T, B, insize] float32 (numpy or device tensor), time-major like validate_network.py:83
    labels : [T', B] int32, T' = the network's output length (validate_network.py:84)
    loss   : float, the mean over the T' * B positions of -log posterior[label]
    ncorrect : int, positions whose first arg-max is the label
    After a call, `loss_rows` (float32) and `correct_rows` (int32) hold its terms per position as [T', B] device tensors.
    """

    def __init__(self, network):
        from . import pipeline
        subs = list(network.layers) if isinstance(network, layers.Serial) else [network]
        if not subs or not isinstance(subs[-1], layers.Softmax):
            raise NotImplementedError("the training loss needs a Softmax output layer (train_network.py:128-133)")
        self.network, self.softmax, self._nbody = network, subs[-1], len(subs) - 1
        # the body is the basecaller's forward pass (a [T, B, features] tensor is taken as it is: nothing is normalised)
        self._body = pipeline.Basecaller(network, fused_decode=False)
        self._sums = None

    def __call__(self, x, labels):
        import torch
        from . import device as D
        L, st, sm = _lib.lib(), layers._stream, self.softmax
        x = D.to_dev(x)
        if x.dim() != 3 or x.shape[2] != self.network.insize:
            raise ValueError("x must be [T, B, %d]" % self.network.insize)
        B = int(x.shape[1])
        h_top = layers._check_input(self._body._hidden(x, self._nbody), sm.insize)
        To = int(h_top.shape[0])
        M = To * B
        labels = D.to_dev(np.ascontiguousarray(labels) if not isinstance(labels, torch.Tensor) else labels, torch.int32)
        if tuple(labels.shape) != (To, B):
            raise ValueError("labels must be [%d, %d] (the network's output length x batch)" % (To, B))
        if self._sums is None:
            # [loss sum (float64 bits), ncorrect, bad-label flag]: one buffer, read back once per batch
            self._sums = torch.zeros(3, dtype=torch.int64, device=x.device)
            self._scratch = torch.empty(256, dtype=torch.float64, device=x.device)
        sums = self._sums
        sums[2] = ((labels < 0) | (labels >= sm.size)).any()
        loss_rows = torch.empty(M, dtype=torch.float32, device=x.device)
        correct_rows = torch.empty(M, dtype=torch.int32, device=x.device)
        rc = _lib.SLK_ERR_UNSUPPORTED
        if sm.split_f16 and sm.insize <= 128 and sm.size <= 2048:
            # only compares columns with the label: a label out of range reads nothing out of bounds, the flag is read with the sums
            hi, lo, inv = sm._split_weights()
            flops = 2.0 * M * sm.insize * sm.size
            with profiler.region("validate_softmax_xent", flops, 4.0 * M * (sm.insize + 3), f16x3_flops=flops) as reg:
                rc = L.slk_linear_xent_eval_f16x3(h_top.data_ptr(), layers._row_stride(h_top), hi.data_ptr(), lo.data_ptr(), inv.data_ptr(),
                                                  sm.b.dev().data_ptr(), sm.insize, sm.size, labels.data_ptr(), To, B,
                                                  loss_rows.data_ptr(), correct_rows.data_ptr(), st())
                if rc == _lib.SLK_ERR_UNSUPPORTED and reg is not None:
                    reg.cancel()
        if rc == _lib.SLK_ERR_UNSUPPORTED:
            # the logits form indexes the row with the label: the answer is needed first
            if bool(sums[2].item()):
                raise ValueError("labels must lie in [0, %d)" % sm.size)
            logits, stats, ld = sm.logits_and_stats(h_top)
            with profiler.region("validate_xent", 0.0, 4.0 * M * ld):
                rc = L.slk_softmax_xent_eval_f32(logits.data_ptr(), ld, stats.data_ptr(), labels.data_ptr(), To, B, sm.size,
                                                 loss_rows.data_ptr(), correct_rows.data_ptr(), st())
        _lib.check(rc, "softmax_xent (validation)")
        with profiler.region("validate_sums", 0.0, 8.0 * M):
            _lib.check(L.slk_reduce_rows_sum_f32(loss_rows.data_ptr(), 1, M, sums.data_ptr(), self._scratch.data_ptr(), st()), "reduce")
            _lib.check(L.slk_reduce_rows_sum_i32(correct_rows.data_ptr(), M, sums[1:].data_ptr(), st()), "reduce")
        self.loss_rows, self.correct_rows = loss_rows.view(To, B), correct_rows.view(To, B)     # the last call's terms per position
        s = sums.cpu().numpy()
        if s[2] != 0:
            raise ValueError("labels must lie in [0, %d)" % sm.size)
        return float(s[:1].view(np.float64)[0]) / M, int(s[1])


def wrap_network(network):
    """validate_network.py:46-54."""
    return ValidationStep(network)


def prepare_validation_labels(labels, bad, transducer=True, bad_state=True):
    """validate_network.py:70-73: blank removal for non-transducer models, bad positions to state 0.  Returns a new int32 array.

    One deliberate difference, the same as train.prepare_training_data documents: `full_labels[full_bad] = 0` (:73) indexes with the
    int8 array HDF5 returns, i.e. it fancy-indexes ROWS 0 and 1 of the labels instead of masking the flagged positions; here `bad` is
    used as the boolean mask the line was written for."""
    labels = np.array(labels, dtype=np.int32)
    if not transducer:
        remove_blanks(labels)                                                       # :70-71
    if bad_state:
        labels[np.asarray(bad).astype(bool)] = 0                                    # :72-73 (see above)
    return labels


def allreduce_validation_sums(loss_sum, nbatch, ncorrect, nev):
    """The four sums of a validation run over all ranks, (float, int, int, int): ONE collective (an all-gather of four 64-bit words per
    rank, the loss sum travelling as its float64 bits), then every rank adds the ranks' figures in rank order -- the counts exactly, the
    loss in float64 -- so every rank holds the same global figures.  A no-op without an initialised process group or with one rank."""
    import torch
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size() == 1:
        return float(loss_sum), int(nbatch), int(ncorrect), int(nev)
    mine = np.array([0, nbatch, ncorrect, nev], dtype=np.int64)
    mine[:1].view(np.float64)[0] = loss_sum
    dev = "cuda" if dist.get_backend() == "nccl" else "cpu"
    part = torch.from_numpy(mine).to(dev)
    parts = [torch.empty_like(part) for _ in range(dist.get_world_size())]
    dist.all_gather(parts, part)
    rows = np.stack([p.cpu().numpy() for p in parts])
    loss = 0.0
    for v in rows[:, :1].copy().view(np.float64)[:, 0]:
        loss += float(v)
    return loss, int(rows[:, 1].sum()), int(rows[:, 2].sum()), int(rows[:, 3].sum())


def validate_network(network, data, batch=200, transducer=True, bad=True, report=None, step=None):
    """validate_network.py:75-110.  `data`: a chunk-file dict (train.load_chunk_file) or the path of one; `network`: anything inference
    accepts that ends in a Softmax.  Whole batches of `batch` chunks are scored, the remainder is dropped (:80).  Returns
    {"score": sum of batch losses / nbatch, "accuracy": ncorrect / nev, "ncorrect", "nev", "nbatch", "seconds"}.

    report: callable taking the reference's progress line (every 50 batches, :99-106) and its `Final` line (:108-110).
    step: the `fv` to use (default: wrap_network(network)).
    With several ranks (train.rank_and_world) rank r scores batches r, r + world, ...; the sums are combined once at the end
    (allreduce_validation_sums) and every rank returns the global figures.  Labels are checked on the host, identically on every rank,
    so that no rank can fail alone and leave the others waiting in the collective."""
    if isinstance(data, str):
        from .train import load_chunk_file
        data = load_chunk_file(data)
    batch = int(batch)
    if batch < 1:
        raise ValueError("batch must be positive")
    full_chunks = data["chunks"]
    nbatch = len(full_chunks) // batch                                              # :80
    if nbatch == 0:
        raise ValueError("%d chunks do not fill one batch of %d" % (len(full_chunks), batch))
    full_labels = prepare_validation_labels(data["labels"], data["bad"], transducer, bad)     # :70-73
    used = full_labels[:nbatch * batch]
    if used.min() < 0 or used.max() >= network.size:
        raise ValueError("labels must lie in [0, %d)" % network.size)
    fv = wrap_network(network) if step is None else step
    rank, world = rank_and_world()
    line_ev = 0
    score, wscore, acc, wacc = 0.0, 0, 0, 0
    t1 = t0 = time.time()
    for k, i in enumerate(range(rank, nbatch, world)):
        idx = i * batch
        events = np.ascontiguousarray(full_chunks[idx: idx + batch].transpose((1, 0, 2)))     # :83
        labels = np.ascontiguousarray(full_labels[idx: idx + batch].transpose())             # :84
        fval, ncorr = fv(events, labels)
        nev = int(np.size(labels))
        line_ev += nev
        score += float(fval)
        wscore += 1
        acc += int(ncorr)
        wacc += nev
        if (k + 1) % 50 == 0 and report is not None:                                # :99-106 (this rank's figures so far)
            tn = time.time()
            dt = max(tn - t1, 1e-9)
            report(PROGRESS_LINE.format((k + 1) // 50, score / wscore, 100.0 * acc / wacc, dt, line_ev / 1000.0 / dt))
            line_ev = 0
            t1 = tn
    score, wscore, acc, wacc = allreduce_validation_sums(score, wscore, acc, wacc)
    dt = max(time.time() - t0, 1e-9)
    if report is not None:
        report(FINAL_LINE.format(score / wscore, 100.0 * acc / wacc, dt, wacc / 1000.0 / dt))
    return {"score": score / wscore, "accuracy": acc / wacc, "ncorrect": acc, "nev": wacc, "nbatch": wscore, "seconds": dt}
