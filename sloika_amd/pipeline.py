"""The hot path end to end, resident on one GPU:

    raw chunks [B, chunk_len] (HBM)  --normalise-->  --conv-->  --GRU/LSTM stack-->  --softmax-->
    --prepare_post + log + k-mer Viterbi + backtrace-->  (scores[B], paths[B,T'], lens[B])

This is the batched restatement of bin/basecall_network.py `raw` (sloika/basecall.py:88-121, 26-51) that
BASELINE.json's metric is quoted on.  All arithmetic happens in the HIP kernels behind include/sloika_amd.h;
torch only owns the buffers and the stream.
"""
import contextlib
import os
import sys

import numpy as np

from . import _lib, batch, decode, layers

_NO_ARENA = contextlib.nullcontext()


class Basecaller(object):
    def __init__(self, network, kmer_len=5, nbase=4, min_prob=1e-5, skip=0.0, normalisation='per-chunk', in_flight=1,
                 fused_decode=None, deterministic=True, borrow=False, transducer=True, bad=True, trans=None):
        """skip default 0.0 is the CLI default (bin/basecall_network.py:38).

        transducer=False (bin/basecall_network.py --no-transducer): the network is a k-mer model without a blank state, decoded as
        basecall.decode_post(transducer=False, bad=bad, trans=trans) does (basecall.py:44, 47-50) -- call_chunks, call_events and
        call_reads materialise the posterior (Softmax.run) and hand it to olddecode.decode_post_batch (csrc/olddecode.hip): float64
        scores, one state per row that is not called bad, each read bit for bit what the single-read worker gives.  `bad`: the
        model has a bad state in column 0; `trans`: None or the [stay, step, skip] prior (--trans).  The throughput flows
        (call_batches, the bucketed / streamed read flows), call_bases and fused_decode=True raise NotImplementedError then.

        in_flight: how many batches the caller keeps in flight at a time, each on a HIP stream of its own (one Basecaller
        per stream).  With two or more, a Gru layer runs eight chunks per workgroup (csrc/gru_bar16d.hip) whenever that lets
        the layers of all the batches share the chip -- batch 1024, two in flight: 2 x 128 workgroups on 256 CUs -- instead of
        one workgroup per four chunks each taking the whole device in turn.

        deterministic (default): a chunk is called the same whatever the batch size and however many batches are in flight (the
        reference calls one read at a time: one read, one answer, basecall.py:88-121).  Every execution plan but one computes the same
        bits; the exception is the sixteen-chunk Gru plan (csrc/gru_bar16q.hip, three-term recurrent products: states equal to float32
        rounding, up to 2 % of chunks called differently), which calls of more than 2048 chunks and four batches in flight would take.
        With deterministic=True they run eight chunks per workgroup instead; deterministic=False lets the faster plan in (the
        price of the switch is in the bench line: `in_flight.deterministic`)."""
        self.deterministic = bool(deterministic)
        self.transducer, self.bad, self.trans = bool(transducer), bool(bad), (None if trans is None else [float(v) for v in trans])
        if not self.transducer:
            if fused_decode:
                raise NotImplementedError("fused_decode=True is the transducer decoder (csrc/softmax_viterbi.hip)")
            if self.trans is not None and len(self.trans) != 3:
                raise ValueError("Incorrect number of transitions")                  # olddecode.py:98
            fused_decode = False
        # borrow: the reference compiles its networks with In(borrow=True) / Out(borrow=True) (layers.py:34-36): what a call returns
        # may be overwritten by a later call, the caller consumes or copies it first.  Here: every buffer of a call (layer outputs,
        # workspaces, results) comes out of an arena this Basecaller keeps, so a call whose shapes repeat allocates nothing, and what a
        # call returns stays intact until TWO further calls have been issued on this Basecaller (device.Arena).  One Basecaller = one
        # stream of work: issue its calls in order on one stream.
        self._arena = None
        if borrow:
            from . import device as D
            self._arena = D.Arena(generations=2)
        if not isinstance(network, layers.Layer):
            raise TypeError("network must be a sloika_amd.layers.Layer")
        self.network = network
        self.kmer_len, self.nbase, self.min_prob, self.skip = kmer_len, nbase, min_prob, skip
        self.normalisation = normalisation
        self.in_flight = max(1, int(in_flight))
        if self.in_flight > 2:
            from . import device as D
            D.want_hw_queues(4 * self.in_flight)
        # fused_decode (None = True): decode straight from the Softmax layer's input (csrc/softmax_viterbi.hip: projection, softmax,
        # prepare_post, log and the Viterbi forward pass in one kernel, the logits never written) where that kernel applies; False
        # keeps the projection kernel + decoder pair
        self.fused_decode = True if fused_decode is None else bool(fused_decode)
        self._ws = decode.ViterbiWorkspace()
        _lib.lib()
        try:                                   # one-time host work that does not belong into the first call (layers._cu_count)
            import torch
            if torch.cuda.is_available():
                layers._cu_count(torch.device("cuda", torch.cuda.current_device()))
        except (ImportError, RuntimeError):
            pass

    def _hidden(self, chunks, upto, scaling=None):
        """Run the network on [B, chunk_len] device signal up to (not including) layer index `upto`.  With `scaling`, `chunks` are int16
        ADC samples with one (offset, range, digitisation) per row (batch.adc_scaling), scaled to picoamperes on the device first."""
        from . import device as D
        cd = D.to_dev(chunks) if scaling is None else batch.adc_chunks_to_pa(chunks, scaling)
        net = self.network
        seq = net.layers if isinstance(net, layers.Serial) else [net]
        first = seq[0]
        if cd.dim() == 3:
            # event-feature models (models/baseline_lstm.py, baseline_gru.py: Window over 4 features per event): the input is the
            # [T, B, features] tensor itself, as `calc_post` takes it (basecall.py:73-75); nothing to normalise
            if cd.shape[2] != first.insize:
                raise ValueError("feature input has %d features per step, the network takes %d" % (cd.shape[2], first.insize))
            x, rest = cd, seq[:upto]
        elif first.insize != 1:
            raise ValueError("this network takes %d features per step: hand over a [T, B, %d] feature tensor, not raw chunks"
                             % (first.insize, first.insize))
        elif (self.normalisation == 'per-chunk' and isinstance(first, layers.Convolution) and first.insize == 1
                and len(seq) > 1):
            # the conv front end reads the chunk-major normalised signal directly: no [T,B,1] transpose
            norm = batch.normalise_chunks(cd, 'per-chunk', out_layout='chunk')
            B, T = norm.shape
            x = first.run_strided(norm.data_ptr(), T, B, 1, T, norm.device)
            rest = seq[1:upto]
        else:
            x = batch.normalise_chunks(cd, self.normalisation, out_layout='network')
            rest = seq[:upto]
        return self._forward(rest, x, self.in_flight)[0]

    def _scope(self):
        """What a pass runs inside: the arena its buffers come out of (borrow=True), or nothing.  Every public entry enters it ONCE per
        pass and nothing below does: Arena.__enter__ begins a pass, which rotates the result generation."""
        return _NO_ARENA if self._arena is None else self._arena

    def _forward(self, seq, x, in_flight, lengths=None):
        """The layers `seq` on the [T, B, features] device tensor x under this Basecaller's plan hints: -> (output, None).  With
        `lengths`, the per-column step counts of a zero-padded batch (layers.ragged): -> (output, int32 device tensor of the columns'
        output steps)."""
        # (the hints are thread local: one forward pass per host thread at a time)
        with layers._HINTS.override(in_flight=in_flight, deterministic=self.deterministic):
            if lengths is None:
                return layers.run_layers(seq, x), None
            with layers.ragged(lengths):
                x = layers.run_layers(seq, x)
                return x, layers.ragged.current.contiguous()

    def _ragged_run(self, x, lengths, upto=None):
        """The network up to (not including) layer index `upto` -- None: all of it, Softmax.run included -- on the zero-padded
        [T, B, features] input x with per-read step counts: -> (output [T', B, .], int32 device tensor of the reads' output steps)."""
        # ragged batches side by side keep the four-chunk plan: their workgroups queue for the CUs and a batch of short reads hands its
        # CUs on early, which a plan that packs more chunks into fewer, slower workgroups would not let it do
        return self._forward(self.network.layers[:upto], x, 1, lengths)

    def _call_ragged(self, x, lengths, fused=True):
        """Network and decoder on the zero-padded [T, B, features] input x with per-read step counts -> (scores, paths, lens)."""
        if not self.transducer:
            return self._decode_profile(*self._ragged_run(x, lengths))
        hid, steps = self._ragged_run(x, lengths, -1)
        return self._decode(self.network.layers[-1], hid, steps, fused=fused)

    def _decode(self, last, hid, lengths=None, lp_dump=None, fused=True):
        """The transducer decoder behind the hidden state `hid` that the Softmax layer `last` takes: csrc/softmax_viterbi.hip where
        it applies and `fused` lets it, else the layer's logits + row statistics.  lengths: None or the columns' steps (int32, device).
        -> (scores, paths, lens)."""
        packed = self._fused_pack(last, hid) if fused else None
        if packed is not None:
            return decode.viterbi_fused_batch(packed[1], packed[0], self.kmer_len, skip_pen=self.skip, nbase=self.nbase,
                                              min_prob=self.min_prob, workspace=self._ws, lengths=lengths, lp_dump=lp_dump)
        if lp_dump is not None:
            raise ValueError("lp_dump needs the fused decoder (csrc/softmax_viterbi.hip does not cover this network)")
        logits, stats, ld = last.logits_and_stats(hid)
        return decode.viterbi_logits_batch(logits, stats, self.kmer_len, hid.shape[0], hid.shape[1], ld=ld, skip_pen=self.skip,
                                           nbase=self.nbase, min_prob=self.min_prob, workspace=self._ws, lengths=lengths)

    def posteriors(self, chunks, scaling=None):
        """[B, chunk_len] device signal -> [T', B, nstate] posteriors (network layout).  `scaling`: as in call_chunks."""
        net = self.network
        n = len(net.layers) if isinstance(net, layers.Serial) else 1
        return self._hidden(chunks, n, scaling)

    #: row widths csrc/softmax_viterbi.hip is instantiated for; any narrower Softmax input is decoded from rows with zero columns up to
    #: the next of them (free when the rows come out of a zero-padded Gru twin, otherwise one padded copy of the hidden state: 0.3 ms
    #: at B = 1024 against the 2 ms of the projection + logits decoder pair)
    FUSED_WIDTHS = (64, 96, 112, 128)

    def _fused_pack(self, last, hid):
        """(the Softmax layer's weights packed for csrc/softmax_viterbi.hip, the hidden state with the row width the kernel reads), or
        None when that kernel does not apply."""
        import torch
        if not self.fused_decode or hid.stride(2) != 1 or hid.stride(0) != hid.shape[1] * hid.stride(1):
            return None
        kp = next((k for k in self.FUSED_WIDTHS if k >= last.insize), None)
        if kp is None:
            return None
        if kp == last.insize:
            if hid.stride(1) % 4 or hid.data_ptr() % 16:
                return None
            pack = last.viterbi_pack(self.nbase, self.kmer_len)
            return None if pack is None else (pack, hid)
        pack = last.viterbi_pack(self.nbase, self.kmer_len, kpad=kp)
        if pack is None:
            return None
        if getattr(hid, "_slk_zero_padded", 0) >= kp and hid.stride(1) >= kp and hid.stride(1) % 4 == 0 and hid.data_ptr() % 16 == 0:
            # straight out of a zero-padded Gru twin (layers.Gru._forward): the columns behind insize exist and are zero
            return pack, hid.as_strided((hid.shape[0], hid.shape[1], kp), hid.stride())
        wide = torch.zeros((hid.shape[0], hid.shape[1], kp), dtype=hid.dtype, device=hid.device)
        wide[:, :, :last.insize] = hid
        return pack, wide

    def call_chunks(self, chunks, lp_dump=None, scaling=None):
        """-> device tensors (scores float32 [B], paths int32 [B, T'] (-1 padded), lens int32 [B]).

        scaling: None (the default) takes `chunks` as they are (picoamperes; any other dtype is cast to float32).  Otherwise `chunks` are
        [B, L] int16 ADC samples (host array or device tensor) and `scaling` one (offset, range, digitisation) per row -- triples, an
        [B, 3] array or fast5 channel_meta dicts (batch.adc_scaling): slk_adc_to_pa_i16 scales them on the device, bit for bit what the
        float32 cast of fast5.Fast5.get_read()'s float64 picoamperes gives.

        When the network ends in a Softmax layer whose shape csrc/softmax_viterbi.hip covers, the decoder starts from that
        layer's INPUT and neither the logits nor the posterior (3.4 GB each at B=1024) are ever written; `lp_dump`, a float32
        device tensor [T', B, nstate], then receives the log-posteriors the dynamic programme consumed (tests).  Otherwise
        (and with fused_decode=False) the decoder consumes the layer's logits + row statistics, bit-identical to decoding
        `posteriors()`."""
        with self._scope():
            if not self.transducer:
                if lp_dump is not None:
                    raise ValueError("lp_dump belongs to the fused transducer decoder")
                return self._decode_profile(self.posteriors(chunks, scaling), None)
            net = self.network
            last = net.layers[-1] if isinstance(net, layers.Serial) else None
            if type(last) is layers.Softmax and len(net.layers) > 1:
                return self._decode(last, self._hidden(chunks, len(net.layers) - 1, scaling), lp_dump=lp_dump)
            post = self.posteriors(chunks, scaling)
            return decode.viterbi_batch(post, self.kmer_len, skip_pen=self.skip, nbase=self.nbase,
                                        min_prob=self.min_prob, workspace=self._ws)

    def _decode_profile(self, post, lengths):
        """basecall.decode_post(transducer=False) over the batch axis of a materialised posterior [T, B, nstate]."""
        from . import olddecode
        return olddecode.decode_post_batch(post, self.kmer_len, bad=self.bad, min_prob=self.min_prob, trans=self.trans, lengths=lengths,
                                           nbase=self.nbase, workspace=self._ws)

    _BATCH_STREAMS = {}

    @classmethod
    def batch_slots(cls, network, in_flight=8, **kwargs):
        """The slots of call_batches, for reuse over several streams of batches: (Basecallers with arenas of their own, their pinned
        result buffers -- two sets per slot, like the arena's two device sets)."""
        cls._transducer_only(kwargs, "call_batches")
        nslot = max(1, int(in_flight))
        return [cls(network, in_flight=nslot, borrow=True, **kwargs) for _ in range(nslot)], [[None, None] for _ in range(nslot)]

    @classmethod
    def call_batches(cls, network, batches, in_flight=8, copy=True, slots=None, **kwargs):
        """A stream of batches with `in_flight` of them on the device at a time: generator over `batches` (an iterable of [B, chunk_len]
        signal batches -- device tensors, or host arrays that are uploaded -- or [T, B, features] tensors for event models), yielding
        (scores float32 [B], paths int32 [B, T'] (-1 padded), lens int32 [B]) as numpy arrays ON THE HOST, one per batch, in the order
        of the input.  A batch may also be an (adc, scaling) pair: [B, L] int16 ADC samples (host array or device tensor) and one scaling per
        row, as call_chunks(adc, scaling=scaling) takes them; such batches and float batches may follow each other in one stream.

        What the reference does with a pool of worker processes (bin/basecall_network.py:100-104, one read per call) a GPU does with
        batches side by side: at the north star's batch of 256 chunks one batch fills 64 of 256 CUs, so several must run at once.  The
        set of streams is FIXED: `in_flight` slots, each with a Basecaller(borrow=True) (a call allocates nothing), a stream (plus the
        side stream the directions of a birnn share their batch's stream with, layers.Parallel), pinned result buffers, and ONE copy
        stream; batch i runs in slot i % in_flight.  Once batch i is queued in its slot the generator hands out batch i - in_flight, the
        slot's batch before (waits for its copy; the slot's two result sets, on the device and on the host, take turns): the host is a
        consumer, a slot holds the batch that runs and at most one queued behind it, the device is never without work -- not even with
        one slot.  8 slots use 17
        streams: below the 32 hardware queues sloika_amd asks for (device.want_hw_queues), so no queue is time-sliced.

        copy=False yields views of the slot's pinned buffers instead of copies: valid until `in_flight` further batches have been
        yielded.  slots: what batch_slots(network, in_flight, ...) returned, for a caller that runs stream after stream (a server): the
        Basecallers keep their arenas and the pinned buffers between the streams, so a later stream allocates nothing at all."""
        import torch
        from . import device as D
        cls._transducer_only(kwargs, "call_batches")
        if slots is None:
            slots = cls.batch_slots(network, in_flight, **kwargs)
        bcs, host = slots
        nslot = len(bcs)
        D.want_hw_queues(2 * nslot + 1)
        # the streams are kept per device and slot count: torch hands out streams from a pool of 32 round robin, and a process that has
        # USED more streams than the runtime has hardware queues (32) gets every queue time-sliced (measured: baseline_raw_gru, eight in
        # flight, 640 M samples/s with 17 streams used, 150-210 M once another leg's 17 had been used before)
        key = (torch.cuda.current_device(), nslot)
        if key not in cls._BATCH_STREAMS:
            cls._BATCH_STREAMS[key] = ([torch.cuda.Stream() for _ in range(nslot)], torch.cuda.Stream())
        streams, copy_stream = cls._BATCH_STREAMS[key]
        pending = [None] * nslot
        ncall = [0] * nslot

        def collect(p):
            ev, bufs, B, T = p
            ev.synchronize()
            sc, pa, le = bufs[0][:B].numpy(), bufs[1][:B, :T].numpy(), bufs[2][:B].numpy()
            return (sc.copy(), pa.copy(), le.copy()) if copy else (sc, pa, le)

        for i, item in enumerate(batches):
            chunks, scaling = item if isinstance(item, tuple) and len(item) == 2 else (item, None)
            k = i % nslot
            before = pending[k]                            # batch i - in_flight: handed out once batch i is queued behind it
            cur = torch.cuda.current_stream()
            s = streams[k]
            s.wait_stream(cur)                             # (whatever produced the batch on the caller's stream)
            with torch.cuda.stream(s):
                # (int16 batches go to the device inside the call, out of the slot's arena)
                cd = D.to_dev(chunks) if scaling is None else chunks
                if isinstance(chunks, torch.Tensor) and chunks.is_cuda:
                    chunks.record_stream(s)
                scores, paths, lens = bcs[k].call_chunks(cd, scaling=scaling)
                done = torch.cuda.Event()
                done.record(s)
            B, T = paths.shape
            g = ncall[k] & 1
            ncall[k] += 1
            bufs = host[k][g]
            if bufs is None or bufs[1].shape[0] < B or bufs[1].shape[1] < T:
                bufs = host[k][g] = (torch.empty((B,), dtype=torch.float32).pin_memory(),
                                     torch.empty((B, T), dtype=torch.int32).pin_memory(),
                                     torch.empty((B,), dtype=torch.int32).pin_memory())
            with torch.cuda.stream(copy_stream):
                copy_stream.wait_event(done)
                bufs[0][:B].copy_(scores, non_blocking=True)
                bufs[1][:B, :T].copy_(paths, non_blocking=True)
                bufs[2][:B].copy_(lens, non_blocking=True)
                ev = torch.cuda.Event()
                ev.record(copy_stream)
            pending[k] = (ev, bufs, B, T)
            if before is not None:
                yield collect(before)
        # the batches still on the device, oldest first
        n = sum(ncall)
        for i in range(n - min(n, nslot), n):
            if pending[i % nslot] is not None:
                yield collect(pending[i % nslot])
                pending[i % nslot] = None

    def call_bases(self, chunks, alphabet='ACGT'):
        """call_chunks + states -> bases on the device (what basecall.SeqPrinter.write does per read, basecall.py:157-163,
        with always_move as for a transducer model): -> (scores device [B], list of B base strings)."""
        from . import bio
        if not self.transducer:
            raise NotImplementedError("call_bases is built on the transducer decoder")
        scores, paths, lens = self.call_chunks(chunks)
        return scores, bio.paths_to_bases(paths, lens, self.kmer_len, alphabet, always_move=True)

    def _marginals(self, post, lengths=None, checkpoint=None, workspace_limit=None):
        """decode.viterbi_marginals_batch on a materialised posterior with this Basecaller's decoder settings."""
        return decode.viterbi_marginals_batch(post, self.kmer_len, skip_pen=self.skip, nbase=self.nbase, min_prob=self.min_prob,
                                              lengths=lengths, checkpoint=checkpoint, workspace_limit=workspace_limit)

    def _qual_check(self, who):
        if not self.transducer:
            raise NotImplementedError("%s is built on the transducer decoder's lattice" % who)

    def call_chunks_qual(self, chunks, scaling=None):
        """call_chunks with a confidence per called position (design/lattice_marginals.md): the decoder's lattice is summed over all its
        paths on the posterior posteriors() leaves (csrc/lattice_marginals.hip).  chunks, scaling: as in call_chunks.
        -> device tensors (scores, paths, lens: the bits Basecaller(fused_decode=False).call_chunks returns; move_row int32 [B, T'], the
        row at which the path enters each state; conf float64 [B, T'], per position the largest marginal of its state over its dwell;
        logz float64 [B], the log of the summed weight of all paths).  bio.paths_to_bases_qual turns paths and conf into letters with
        Phred values."""
        self._qual_check("call_chunks_qual")
        with self._scope():
            return self._marginals(self.posteriors(chunks, scaling))

    def call_reads_qual(self, signals, trim=(0, 0), open_pore_fraction=0.0, scaling=None):
        """call_reads with a confidence per called position: the same upload, trimming and failures, the network on the zero-padded batch
        with per-read lengths, then the lattice of every read over its own rows of the posterior -- each read gets what a batch-1 call
        gives.  -> (scores, paths, lens, move_row, conf, logz) as call_chunks_qual returns them, and the per-read sample counts."""
        self._qual_check("call_reads_qual")
        padded, nsamp = self._padded_reads(signals, trim, open_pore_fraction, scaling, "call_reads_qual")
        with self._scope():
            post, steps = self._read_posteriors(padded, nsamp)
            return self._marginals(post, steps) + (nsamp,)

    def call_fastq(self, signals, names=None, trim=(0, 0), open_pore_fraction=0.0, scaling=None, alphabet='ACGT', qmax=60):
        """Whole reads -> FASTQ records (call_reads_qual, bio.paths_to_bases_qual, bio.fastq_text): a list with one four-line record
        per read, qualities as Phred + 33 capped at qmax; names default to read0, read1, ...  ''.join(records) is the file."""
        from . import bio
        res = self.call_reads_qual(signals, trim=trim, open_pore_fraction=open_pore_fraction, scaling=scaling)
        calls = bio.paths_to_bases_qual(res[1], res[2], res[4], self.kmer_len, alphabet, qmax=qmax)
        if names is None:
            names = ["read%d" % r for r in range(len(calls))]
        return [bio.fastq_text([n], [seq], [q]) for n, (seq, q) in zip(names, calls)]

    def score_chunks(self, chunks, sequences, full=True, scaling=None):
        """How likely is each sequence under the network's posterior of its chunk, summed over all alignments: decode.forwards
        (decode.py:108-139) of basecall.decode_post's prepared posterior (min_prob as in call_chunks), for the whole batch in one
        launch.  The posterior is read where posteriors() leaves it (network layout, no transpose or copy).

        sequences: one entry per chunk, either an integer array (or tensor) of k-mer states -- what paths[b, :lens[b]] of
        call_chunks holds, so a call can be scored against its own chunk -- or a base string, cut into its k-mers (bio.seq_to_kmers)
        and numbered by bio.kmer_mapping.  full, scaling: as decode.forwards / call_chunks.
        -> device float64 [B], natural-log likelihoods."""
        cols = self._sequence_columns(chunks, sequences, "score_chunks", "forward score")
        with self._scope():
            post = self.posteriors(chunks, scaling)
            return decode.forwards_batch(post, cols, full=full, blank=0, min_prob=self.min_prob)

    def occupancy_chunks(self, chunks, sequences, full=True, scaling=None):
        """With what probability each row of a chunk's posterior emits each state under a sequence, summed over all alignments
        (decode.forwards_backwards_batch, design/forward_backward.md): the soft counterpart of the remap's one best alignment.
        chunks, sequences, full, scaling: as score_chunks, on the same prepared posterior.
        -> (ll device float64 [B], the bits score_chunks returns; occ device float32 [T', B, nstate]: occ - posterior is the gradient of
        ll by the logits; emit_row, emit_prob: lists of B device views, per position the row that most probably emits it and that
        probability)."""
        cols = self._sequence_columns(chunks, sequences, "occupancy_chunks", "occupancy")
        with self._scope():
            post = self.posteriors(chunks, scaling)
            return decode.forwards_backwards_batch(post, cols, full=full, blank=0, min_prob=self.min_prob)

    def _polish_check(self, chunks, drafts, who):
        if not self.transducer:
            raise NotImplementedError("%s needs a transducer model: without a blank state there is no forward score" % who)
        if self.nbase != 4:
            raise ValueError("%s reads drafts in the alphabet ACGT (nbase=%d)" % (who, self.nbase))
        if len(drafts) != len(chunks):
            raise ValueError("%s needs one draft per chunk (%d for %d)" % (who, len(drafts), len(chunks)))

    def rescore_chunks(self, chunks, drafts, group=None, kinds=('sub', 'del', 'ins'), scaling=None):
        """What would the signal gain from each single-letter edit of a draft: polish.rescore_drafts on the prepared posterior of
        score_chunks (posteriors(), blank 0, columns state + 1, min_prob as in call_chunks; csrc/rescore_edits.hip,
        design/rescore_edits.md).

        drafts: one base string per chunk; group[b] names the draft chunk b is a read of (the chunks of one group carry the same
        string; None: every chunk is its own group).  The edits are enumerated once per group (bio.single_letter_edits).
        -> per group, in the order of its first chunk, a polish.Rescored: `edits` the rows (kind, letter_pos, letter, edited_string),
        `gain` device float64 [len(edits)]: the sum over the group's chunks of (log-likelihood of the edited string - that of the
        draft), `score` the summed log-likelihood of the draft."""
        from . import polish
        self._polish_check(chunks, drafts, "rescore_chunks")
        with self._scope():
            post = self.posteriors(chunks, scaling)
            return polish.rescore_drafts(post, drafts, self.kmer_len, group=group, kinds=kinds, blank=0, min_prob=self.min_prob)

    def polish_chunks(self, chunks, drafts, group=None, min_gain=0.0, max_rounds=8, kinds=('sub', 'del', 'ins'), scaling=None):
        """polish.polish on the prepared posterior of the chunks (one network pass, then rounds of rescore_chunks' scoring): per group a
        polish.Polished with the polished string, the applied edits with their gains, the rounds and the final summed score."""
        from . import polish
        self._polish_check(chunks, drafts, "polish_chunks")
        with self._scope():
            post = self.posteriors(chunks, scaling)
            return polish.polish(post, drafts, self.kmer_len, group=group, min_gain=min_gain, max_rounds=max_rounds, kinds=kinds,
                                 blank=0, min_prob=self.min_prob)

    def _padded_reads(self, signals, trim, open_pore_fraction, scaling, who):
        """Whole reads on their way to the network, for call_reads_qual and rescore_reads alike: the upload, trimming and failures
        of call_reads.  -> (zero-padded batch on the device, sample counts)."""
        net = self.network
        if not isinstance(net, layers.Serial) or type(net.layers[-1]) is not layers.Softmax:
            raise ValueError("%s needs a Serial network ending in a Softmax layer" % who)
        if min(len(s) for s in signals) < 100:
            raise ValueError("a read is shorter than one window of 100 samples")
        dev, start, nsamp, flags = self._trimmed_read_set(signals, trim, open_pore_fraction, scaling)
        for r, f in enumerate(flags):
            if f:
                raise ValueError(batch.read_failure(f)[2].format(r))
        return batch.pack_batch(dev, start, nsamp, max(nsamp)), nsamp

    def _read_posteriors(self, padded, nsamp):
        """The network on the zero-padded batch with per-read lengths, as call_reads_qual runs it (inside _scope): -> (post
        [T', B, nstate], int32 device tensor of the reads' rows)."""
        lengths = layers.ragged_lengths(nsamp)
        return self._ragged_run(batch.normalise_reads_ragged(padded, lengths), lengths)

    def _read_bands(self, post, steps, drafts, center, slip):
        """The drafts and centre lines rescore_reads / polish_reads hand to polish: -> (drafts, [centre per read])."""
        import numpy as np
        import torch
        from . import bio, device as D, transducer
        k, B = self.kmer_len, int(post.shape[1])
        rows = steps.cpu().numpy().astype(np.int64)
        if drafts is None:
            if center is not None:
                raise ValueError("a read's own call brings its centre line from its moves: center is for given drafts")
            _, paths, lens, move_row, _, _ = self._marginals(post, steps)
            paths, lens, move_row = paths.cpu().numpy(), lens.cpu().numpy(), move_row.cpu().numpy()
            drafts, centers = [], []
            for b in range(B):
                states = paths[b, :lens[b]].astype(np.int64)
                if not len(states):
                    raise ValueError("read %d has no call to polish" % b)
                nemit = np.concatenate([[k], np.minimum(bio.moves_of_states(states, k, self.nbase, False), k)])
                drafts.append(bio.sequence_of_states(states, k, self.nbase, nemit[1:], 'ACGT'))
                centers.append(decode.band_center_from_moves(move_row[b, :lens[b]], nemit, int(rows[b]), k))
            return drafts, centers
        drafts = [d.decode('utf-8') if isinstance(d, bytes) else d for d in drafts]
        if isinstance(center, str):
            if center != "remap":
                raise ValueError("center is a list of centre lines, or 'remap'")
            # the existing remap DP on the same posterior (its cost is the remap's, not the rescoring's)
            ev_off = np.concatenate([[0], np.cumsum(rows)]).astype(np.int64)
            pc = post if post.stride(2) == 1 else post.contiguous()
            ltrans = torch.empty((int(ev_off[-1]), int(pc.shape[2])), dtype=torch.float32, device=pc.device)
            ev_d = torch.from_numpy(ev_off).to(pc.device)
            _lib.check(_lib.lib().slk_remap_pack_log_post_f32(pc.data_ptr(), pc.stride(0), pc.stride(1), int(pc.shape[0]), B,
                                                              int(pc.shape[2]), steps.data_ptr(), ev_d.data_ptr(),
                                                              float(self.min_prob), ltrans.data_ptr(), D.stream_ptr()), "rescore_reads.pack")
            seqs = [bio.seq_to_states(d, k) + 1 for d in drafts]
            _, paths = transducer.map_to_sequence_packed(ltrans, ev_off, seqs, slip, long_reference=True)
            return drafts, [decode.band_center_from_path(p) for p in paths]
        if center is None or len(center) != B:
            raise ValueError("given drafts need one centre line per read (center=[...]), or center='remap'")
        return drafts, list(center)

    def rescore_reads(self, signals, drafts=None, group=None, width=512, center=None, trim=(0, 0), open_pore_fraction=0.0,
                      scaling=None, kinds=('sub', 'del', 'ins'), slip=5.0):
        """rescore_chunks for whole reads (csrc/rescore_band.hip, design/rescore_band.md): the posterior of every read over its own
        rows, as call_reads_qual gets it, and polish.rescore_drafts with banded lattices of `width` states per row.

        drafts None: every read is rescored against its own call, the band laid round the call's moves
        (decode.band_center_from_moves).  Given drafts (base strings, for example genome.read_references records; group as in
        rescore_chunks) come with center=[one centre line per read] or center="remap", which aligns each read to its draft by
        transducer.map_to_sequence_packed(long_reference=True) with slip penalty `slip` first.  Refusals are rescore_chunks'.
        -> [polish.Rescored]; `score` and `gain` are the banded ones."""
        from . import polish
        self._polish_check(signals, signals if drafts is None else drafts, "rescore_reads")
        padded, nsamp = self._padded_reads(signals, trim, open_pore_fraction, scaling, "rescore_reads")
        with self._scope():
            post, steps = self._read_posteriors(padded, nsamp)
            drafts, centers = self._read_bands(post, steps, drafts, center, slip)
            return polish.rescore_drafts(post, drafts, self.kmer_len, group=group, kinds=kinds, blank=0, min_prob=self.min_prob,
                                         lengths=steps, band=(centers, width))

    def polish_reads(self, signals, drafts=None, group=None, width=512, center=None, trim=(0, 0), open_pore_fraction=0.0,
                     scaling=None, kinds=('sub', 'del', 'ins'), min_gain=0.0, max_rounds=8, slip=5.0):
        """polish_chunks for whole reads: one network pass, then rounds of rescore_reads' banded scoring; the centre lines follow the
        applied edits (polish.shifted_centers), nothing is re-aligned between rounds.  -> [polish.Polished]."""
        from . import polish
        self._polish_check(signals, signals if drafts is None else drafts, "polish_reads")
        padded, nsamp = self._padded_reads(signals, trim, open_pore_fraction, scaling, "polish_reads")
        with self._scope():
            post, steps = self._read_posteriors(padded, nsamp)
            drafts, centers = self._read_bands(post, steps, drafts, center, slip)
            return polish.polish(post, drafts, self.kmer_len, group=group, min_gain=min_gain, max_rounds=max_rounds, kinds=kinds,
                                 blank=0, min_prob=self.min_prob, lengths=steps, band=(centers, width))

    def _genome_reads(self, signals, trim, open_pore_fraction, scaling, who):
        """Whole reads for rescore_genome / polish_genome (inside _scope): the posterior of every read over its own rows and the call
        with its moves, as call_reads_qual makes them.  -> (post, steps, paths, lens, move_row)."""
        self._polish_check(signals, signals, who)
        self._qual_check(who)
        padded, nsamp = self._padded_reads(signals, trim, open_pore_fraction, scaling, who)
        post, steps = self._read_posteriors(padded, nsamp)
        _, paths, lens, move_row, _, _ = self._marginals(post, steps)
        return post, steps, paths, lens, move_row

    def rescore_genome(self, signals, index, width=512, margin=None, kinds=('sub', 'del', 'ins'), keep=None, region=None, trim=(0, 0),
                       open_pore_fraction=0.0, scaling=None, workspace_limit=None, **map_kwargs):
        """What the signal of whole reads says about every single-letter edit of a genome (design/polish_genome.md): the reads are
        called (call_reads_qual's posterior and moves), the calls placed on `index` (genome.Index.map_paths(ops=True, **map_kwargs)),
        and polish.rescore_genome scores each read's window under its own rows and sums the gains on genome coordinates.
        keep: None, a bool mask of the reads, or a function (res, strand, info) -> mask (info['edge'] == 0 is the usual filter).
        Refusals are rescore_chunks'.  -> polish.GenomeRescored."""
        from . import polish
        with self._scope():
            post, steps, paths, lens, move_row = self._genome_reads(signals, trim, open_pore_fraction, scaling, "rescore_genome")
            got = index.map_paths(paths, lens, self.kmer_len, ops=True, **map_kwargs)
            res, strand, info, ops = got[0], got[1], got[2], got[4]
            mask = keep(res, strand, info) if callable(keep) else keep
            return polish.rescore_genome(post, steps, paths, lens, move_row, index, res, strand, info, ops, self.kmer_len, width=width,
                                         margin=margin, kinds=kinds, keep=mask, region=region, blank=0, min_prob=self.min_prob,
                                         workspace_limit=workspace_limit)

    def rescore_variants(self, signals, index, variants, width=512, margin=None, keep=None, trim=(0, 0), open_pore_fraction=0.0,
                         scaling=None, workspace_limit=None, **map_kwargs):
        """What the signal of whole reads says about proposed variants of any length (design/polish_variants.md): rescore_genome's
        calls, mapping and windows, each variant -- (contig, pos, ndel, alt) rows, a polish.VariantSet or 'repeats' -- put to every
        read that covers it as ONE hypothesis (polish.rescore_variants).  keep as rescore_genome.
        -> polish.GenomeVariantsRescored."""
        from . import polish
        with self._scope():
            post, steps, paths, lens, move_row = self._genome_reads(signals, trim, open_pore_fraction, scaling, "rescore_variants")
            got = index.map_paths(paths, lens, self.kmer_len, ops=True, **map_kwargs)
            res, strand, info, ops = got[0], got[1], got[2], got[4]
            mask = keep(res, strand, info) if callable(keep) else keep
            return polish.rescore_variants(post, steps, paths, lens, move_row, index, res, strand, info, ops, self.kmer_len, variants,
                                           width=width, margin=margin, keep=mask, blank=0, min_prob=self.min_prob,
                                           workspace_limit=workspace_limit)

    def call_variants(self, signals, index, min_count=2, min_fraction=0.2, min_depth=3, max_del=8, max_ins=4, het=1e-3, prior=None,
                      scale=1.0, variants=None, region=None, keep=None, width=512, margin=None, trim=(0, 0), open_pore_fraction=0.0,
                      scaling=None, workspace_limit=None, **map_kwargs):
        """Call the variants of a sample against a reference from whole reads (design/genotypes.md): one network pass and decode, one
        mapping (genome.Index.map_paths(ops=True, **map_kwargs)), a pileup of the kept reads, the alleles it proposes -- the minority
        ones too -- with `variants` (rows, a polish.VariantSet or 'repeats') added, each put to the reads' signal on the same mapping
        (polish.rescore_variants) and genotyped (polish.genotypes; het, prior, scale).  keep as rescore_genome.  The likelihood ratios
        are the network's own and are not calibrated: what `scale` should be on real reads has not been measured.
        -> polish.VariantCalls (rows(), vcf())."""
        from . import polish
        with self._scope():
            post, steps, paths, lens, move_row = self._genome_reads(signals, trim, open_pore_fraction, scaling, "call_variants")
            got = index.map_paths(paths, lens, self.kmer_len, ops=True, **map_kwargs)
            res, strand, info, ops = got[0], got[1], got[2], got[4]
            mask = keep(res, strand, info) if callable(keep) else keep
            return polish.call_variants(post, steps, paths, lens, move_row, index, res, strand, info, ops, self.kmer_len,
                                        min_count=min_count, min_fraction=min_fraction, min_depth=min_depth, max_del=max_del,
                                        max_ins=max_ins, het=het, prior=prior, scale=scale, variants=variants, region=region, width=width,
                                        margin=margin, keep=mask, blank=0, min_prob=self.min_prob, workspace_limit=workspace_limit)

    def polish_genome(self, signals, index, width=512, margin=None, kinds=('sub', 'del', 'ins'), keep=None, min_gain=0.0,
                      min_support=2, max_rounds=4, trim=(0, 0), open_pore_fraction=0.0, scaling=None, workspace_limit=None,
                      proposals=None, **map_kwargs):
        """polish.polish_genome on whole reads: one network pass and one decode, then rounds of mapping the same calls onto the
        current strings, rescore_genome's sums and the edits the signal prefers.  `index` may be the reference or
        genome.Index(dict(consensus.sequences())).  -> ([polish.GenomePolished] per contig, the last round's polish.GenomeRescored).
        proposals: as polish.polish_genome takes it (variants of any length beside the cells; a third value is then returned)."""
        from . import polish
        with self._scope():
            post, steps, paths, lens, move_row = self._genome_reads(signals, trim, open_pore_fraction, scaling, "polish_genome")
            more = {} if proposals is None else {'proposals': proposals}
            return polish.polish_genome(post, steps, paths, lens, move_row, index, self.kmer_len, width=width, margin=margin,
                                        kinds=kinds, keep=keep, min_gain=min_gain, min_support=min_support, max_rounds=max_rounds,
                                        blank=0, min_prob=self.min_prob, workspace_limit=workspace_limit, map_kwargs=map_kwargs, **more)

    def _sequence_columns(self, chunks, sequences, who, what):
        """The posterior columns of one sequence per chunk, each k-mer states or a base string (score_chunks): state + 1, column 0 is
        the blank (variables.nstate, transducer=True)."""
        import numpy as np
        from . import bio
        if not self.transducer:
            raise NotImplementedError("%s needs a transducer model: without a blank state there is no %s" % (who, what))
        if len(sequences) != len(chunks):
            raise ValueError("%s needs one sequence per chunk (%d for %d)" % (who, len(sequences), len(chunks)))
        mapping = None
        cols = []
        for q in sequences:
            if isinstance(q, (str, bytes)):
                if self.nbase != 4:
                    raise ValueError("base strings are read in the alphabet ACGT: hand over states for nbase=%d" % self.nbase)
                if mapping is None:
                    mapping = bio.kmer_mapping(self.kmer_len)
                text = q.decode('utf-8') if isinstance(q, bytes) else q
                try:
                    st = np.array([mapping[k] for k in bio.seq_to_kmers(text, self.kmer_len)], dtype=np.int64)
                except KeyError as exc:
                    raise ValueError("k-mer %s is outside the model's alphabet" % exc)
            else:
                st = np.asarray(q.cpu() if hasattr(q, "cpu") else q).astype(np.int64).reshape(-1)
                if st.size and (st.min() < 0 or st.max() >= self.nbase ** self.kmer_len):
                    raise ValueError("k-mer states must lie in 0 .. %d" % (self.nbase ** self.kmer_len - 1))
            cols.append(st + 1)
        return cols

    def _call_padded(self, padded, nsamp):
        """One padded batch of trimmed reads resident on the device ([B, Lmax], read b in its first nsamp[b] samples): per-read
        normalisation, network and decoder with per-read lengths.  -> (scores, paths, lens) on the device."""
        with self._scope():
            lengths = layers.ragged_lengths(nsamp)
            # per-read normalisation (basecall.py:117-118)
            return self._call_ragged(batch.normalise_reads_ragged(padded, lengths), lengths)

    def call_reads(self, signals, trim=(0, 0), open_pore_fraction=0.0, scaling=None):
        """Whole reads of different lengths in ONE batch (the reference calls them one at a time, basecall.py:88-121):
        `signals` is a list of 1-D float arrays (already scaled, e.g. fast5.Fast5.get_read()); each is trimmed as raw_worker does, median/MAD
        normalised over its own length, zero-padded to the longest, and the network + decoder run on the padded batch
        with per-read lengths (layers.ragged), so every read gets exactly what a batch-1 call would give.
        -> device tensors (scores [B], paths [B, T'max] (-1 padded), lens [B]) and the per-read sample counts.
        A read that cannot be called (shorter than one window, a sample that is not finite, no window livelier than the open-pore
        threshold, nothing left after trimming) raises ValueError.

        scaling: None takes `signals` as picoamperes.  Otherwise `signals` are 1-D int16 ADC reads (fast5.Fast5.get_read(scale=False)) and
        `scaling` one (offset, range, digitisation) per read (fast5.Fast5.scaling(), batch.adc_scaling): the samples go to the device as
        they are and are scaled there (slk_adc_to_pa_i16) -- the same calls as on the picoamperes."""
        net = self.network
        if not isinstance(net, layers.Serial) or type(net.layers[-1]) is not layers.Softmax:
            raise ValueError("call_reads needs a Serial network ending in a Softmax layer")
        if min(len(s) for s in signals) < 100:
            raise ValueError("a read is shorter than one window of 100 samples")
        dev, start, nsamp, flags = self._trimmed_read_set(signals, trim, open_pore_fraction, scaling)
        for r, f in enumerate(flags):
            if f:
                raise ValueError(batch.read_failure(f)[2].format(r))
        scores, paths, lens = self._call_padded(batch.pack_batch(dev, start, nsamp, max(nsamp)), nsamp)
        return scores, paths, lens, nsamp

    def call_events(self, tables, trim=(0, 0), tag=''):
        """Event tables of different lengths in ONE batch, for the models that take event features (the reference calls them one at a
        time, basecall.py:54-85): `tables` is a list of event tables (numpy structured arrays or dicts of columns tag + 'mean',
        tag + 'stdv', 'length'); each is trimmed as events_worker does (basecall.py:77) and its features, studentised over its own
        events, are written by slk_event_features_f32 straight into the zero-padded [T, B, 4] network input -- all tables in one launch.
        Network and decoder run with per-read lengths (layers.ragged); the decoder is the one that reads the Softmax layer's logits,
        which is bit for bit basecall.decode_post on the posterior, so every read gets exactly what basecall.events_read_worker gives
        for it alone.
        -> device tensors (scores [B], paths [B, Tmax] (-1 padded), lens [B]) and the per-read event counts after trimming.
        A table with no event left after trimming, or one that holds a value that is not finite, is left out of the batch and reported
        on stderr as the reference's worker reports a read it skips (basecall.py:78-80): score NaN, no path, event count 0; the other
        reads are unaffected."""
        import torch
        from . import device as D, features
        net = self.network
        if not isinstance(net, layers.Serial) or type(net.layers[-1]) is not layers.Softmax:
            raise ValueError("call_events needs a Serial network ending in a Softmax layer")
        if net.layers[0].insize != 4:
            raise ValueError("call_events needs a network that takes the 4 event features, this one takes %d" % net.layers[0].insize)
        assert trim[0] >= 0 and trim[1] >= 0
        cols = [features.event_columns(ev, tag) for ev in tables]
        nev = [max(0, c.shape[1] - trim[0] - trim[1]) for c in cols]
        flags = [(0 if np.isfinite(c).all() else 1) | (0 if n > 0 else 4) for c, n in zip(cols, nev)]
        self._report_failures(flags)
        nev = [0 if f else n for f, n in zip(flags, nev)]
        good = [r for r, f in enumerate(flags) if not f]
        ntab = len(tables)
        if not good:
            dev = D.device()
            return (torch.full((ntab,), float("nan"), device=dev), torch.full((ntab, 0), -1, dtype=torch.int32, device=dev),
                    torch.zeros((ntab,), dtype=torch.int32, device=dev), nev)
        kept = [nev[r] for r in good]
        with self._scope():
            # table good[b]'s events trim[0] .. trim[0] + kept[b] - 1 become column b.  Never the fused kernel: the events' contract is
            # the decoder that reads the Softmax layer's logits, which is bit for bit basecall.decode_post on the posterior
            x = features.network_input([{"mean": cols[r][0], "stdv": cols[r][1], "length": cols[r][2]} for r in good], kept,
                                       int(trim[0]))
            scores, paths, lens = self._call_ragged(x, kept, fused=False)
        if len(good) == ntab:
            return scores, paths, lens, nev
        idx = torch.as_tensor(good, device=scores.device)
        all_scores = torch.full((ntab,), float("nan"), dtype=scores.dtype, device=scores.device)
        all_paths = torch.full((ntab, paths.shape[1]), -1, dtype=paths.dtype, device=scores.device)
        all_lens = torch.zeros((ntab,), dtype=lens.dtype, device=scores.device)
        all_scores[idx], all_paths[idx], all_lens[idx] = scores, paths, lens
        return all_scores, all_paths, all_lens, nev

    @staticmethod
    def _transducer_only(kwargs, what):
        """The throughput flows are built on the transducer decoders; a non-transducer model goes through call_chunks / call_events /
        call_reads."""
        if not kwargs.get("transducer", True):
            raise NotImplementedError("%s is not available with transducer=False: use call_chunks, call_events or call_reads" % what)

    @staticmethod
    def _trimmed_read_set(signals, trim, open_pore_fraction, scaling):
        """The read set in ONE upload (batch.upload_read_set), the trimming bounds out of one launch over all windows
        (basecall.py:111-112).  -> (device set, first sample of every read after trimming, its sample count, its flags
        (batch.read_spans: 0 for a read that can be called))."""
        dev, off, lens, bad = batch.upload_read_set(signals, scaling=scaling)
        bounds = batch.open_pore_bounds_many(dev, off, lens, open_pore_fraction)
        start, nsamp, flags = batch.read_spans(bounds, bad, trim)
        return dev, [int(o) + s for o, s in zip(off, start)], nsamp, flags

    @staticmethod
    def _report_failures(flags, ids=None):
        """A line on stderr for every read that cannot be called, as the reference's worker reports a read it skips (basecall.py:103-115),
        with the reason of its first flag bit (batch.READ_FAILURES)."""
        for r, f in enumerate(flags):
            if f:
                sys.stderr.write("Failure calling read {}: {}\n".format(r if ids is None else ids[r], batch.read_failure(f)[1]))

    @staticmethod
    def length_buckets(nsamp, max_batch=256, max_waste=0.08, footprint=None):
        """Group read indices into batches of similar length: reads sorted by length, a batch closed when it holds `max_batch`
        reads or when padding every member to the longest would waste more than `max_waste` of the batch's steps.  -> list of
        index lists (longest reads first: the big batches start while the host still packs the small ones).

        footprint (default: off): a pair (bytes_of, limit) -- bytes_of(longest sample count, reads) gives the device bytes a batch of
        that shape holds; a batch is also closed before one more read would take it past `limit`."""
        order = sorted(range(len(nsamp)), key=lambda i: -nsamp[i])
        buckets, cur = [], []
        for i in order:
            if cur:
                lmax = nsamp[cur[0]]
                used = sum(nsamp[j] for j in cur) + nsamp[i]
                if (len(cur) >= max_batch or 1.0 - used / float(lmax * (len(cur) + 1)) > max_waste
                        or (footprint is not None and footprint[0](lmax, len(cur) + 1) > footprint[1])):
                    buckets.append(cur)
                    cur = []
            cur.append(i)
        if cur:
            buckets.append(cur)
        return buckets

    @classmethod
    def prepare_read_batches(cls, network, signals, trim=(0, 0), open_pore_fraction=0.0, max_batch=256, max_waste=0.08, ids=None,
                             scaling=None, footprint=None, **kwargs):
        """Preparation of the whole-read mode: the read set goes to the device in one upload, trimming bounds come from one launch over
        all windows (basecall.py:111-112), reads are bucketed by length and every bucket becomes a zero-padded device batch (one launch
        per bucket).  -> (batches, nsamp): batches = [(read indices, padded device tensor [B, Lmax], their sample counts)], nsamp =
        sample count of every read after trimming.

        A read that cannot be called -- no sample left after trimming, shorter than one open-pore window, no window livelier than
        the threshold, or a sample that is not finite -- is left out of every batch and gets nsamp 0; `failed_reads(nsamp)` lists
        them.  The reference's worker does the same one read at a time: it reports the read on stderr, returns None and the pool goes
        on (basecall.py:103-115).  The other reads of the set are unaffected.

        scaling: as in call_reads -- int16 reads go to the device as they are and are scaled there (batch.upload_read_set), the
        check for samples that are not finite coming out of the same kernel.

        footprint: as in length_buckets; a read whose batch of one is past the limit raises ValueError before any batch is packed."""
        # the host touches every sample once; the padded batches are built on the device (a launch per bucket)
        dev, start, nsamp, flags = cls._trimmed_read_set(signals, trim, open_pore_fraction, scaling)
        cls._report_failures(flags, ids)
        good = [r for r in range(len(nsamp)) if nsamp[r] > 0]
        if footprint is not None:
            cls._check_footprints([nsamp[r] for r in good], [r if ids is None else ids[r] for r in good], footprint)
        batches = []
        for sub in cls.length_buckets([nsamp[r] for r in good], max_batch, max_waste, footprint):
            idx = [good[j] for j in sub]
            ns = [nsamp[i] for i in idx]
            batches.append((idx, batch.pack_batch(dev, [start[i] for i in idx], ns, max(ns)), ns))
        return batches, nsamp

    @staticmethod
    def failed_reads(nsamp):
        """Indices of the reads prepare_read_batches left out (their sample count after trimming is 0)."""
        return [i for i, n in enumerate(nsamp) if n < 1]

    @classmethod
    def run_read_batches(cls, network, batches, nreads, in_flight=None, lanes=None, **kwargs):
        """Device side: every prepared batch through normalisation, network and decoder, the batches spread over `in_flight`
        streams (default: one per batch, at most 8 -- a batch of 200 long reads occupies 50 of the 256 CUs for tens of
        milliseconds, so the chip only fills up with several of them side by side).  `lanes`: a list of (Basecaller, stream)
        pairs to reuse (read_lanes(); torch's allocator caches device memory per stream, so a server that keeps its lanes does
        not pay for gigabytes of fresh allocations on every call).  -> (scores [N] float32, list of N int32 path arrays) on the
        host; a read that is in no batch (failed_reads) has score NaN and path None."""
        import torch
        cls._transducer_only(kwargs, "run_read_batches")
        if lanes is None:
            lanes = cls.read_lanes(network, max(1, min(8, len(batches)) if in_flight is None else in_flight), **kwargs)
        # every batch queued on its lane (batch k on lane k % lanes) with its results' way to the host behind it, then collected
        cur = torch.cuda.current_stream()
        pending = []
        for k, (idx, padded, ns) in enumerate(batches):
            bc, s = lanes[k % len(lanes)]
            s.wait_stream(cur)
            with torch.cuda.stream(s):
                padded.record_stream(s)
                res = bc._call_padded(padded, ns)
                host = tuple(t.to("cpu", non_blocking=True) for t in res)
                ev = torch.cuda.Event()
                ev.record(s)
            pending.append((idx, host, ev, res))
        return cls._collect_reads(pending, nreads)

    @staticmethod
    def _collect_reads(pending, nreads):
        """Waits for every queued batch -- (read indices, its results on their way to the host: scores, paths, lens first, the event
        behind them, the device tensors they are copied from) -- and hands each read its own: -> (scores [nreads] float32, NaN for a
        read in no batch; list of nreads int32 path arrays, None for such a read)."""
        scores = np.full(nreads, np.nan, dtype=np.float32)
        paths = [None] * nreads
        for idx, host, ev, _ in pending:
            ev.synchronize()
            sc, pa, le = (h.numpy() for h in host[:3])
            for j, i in enumerate(idx):
                scores[i] = sc[j]
                paths[i] = pa[j, :le[j]].copy()
        return scores, paths

    @classmethod
    def read_lanes(cls, network, n, **kwargs):
        """n (Basecaller, stream) pairs sharing one network, for run_read_batches / call_reads_bucketed."""
        import torch
        cls._transducer_only(kwargs, "read_lanes")
        return [(cls(network, in_flight=n, **kwargs), torch.cuda.Stream()) for _ in range(max(1, n))]

    @classmethod
    def call_reads_bucketed(cls, network, signals, trim=(0, 0), open_pore_fraction=0.0, max_batch=256, max_waste=0.08, in_flight=None,
                            lanes=None, stream_buckets=True, scaling=None, **kwargs):
        """Whole-read mode for MANY reads (what bin/basecall_network.py does with a pool of workers, basecall_network.py:100-104):
        reads are bucketed by length (length_buckets), every bucket is one padded ragged batch, and the buckets run side by side
        on streams of their own (one Basecaller each, sharing the network).  Each read gets bit for bit what call_reads([read])
        gives.  -> (scores [N] float32, list of N int32 path arrays, sample counts [N], stats) all on the host; stats holds the
        padded-step waste and the indices of the reads that could not be called (`failed`: score NaN, path None, sample count 0 --
        each reported on stderr as the reference's worker reports a read it skips, basecall.py:103-115).

        scaling: as in call_reads (int16 ADC reads, one (offset, range, digitisation) per read, scaled on the device): the same results
        as on the float64 picoamperes fast5.Fast5.get_read() returns, for half the bytes over the bus and a quarter of the host memory."""
        cls._transducer_only(kwargs, "call_reads_bucketed")
        streamed = open_pore_fraction == 0 and len(signals) > 2 * max_batch and stream_buckets
        if streamed:
            scores, paths, nsamp, nbatch, padded = cls._call_reads_streamed(network, signals, trim, max_batch, max_waste, in_flight, lanes,
                                                                            scaling=scaling, **kwargs)
        else:
            batches, nsamp = cls.prepare_read_batches(network, signals, trim, open_pore_fraction, max_batch, max_waste, scaling=scaling,
                                                      **kwargs)
            scores, paths = cls.run_read_batches(network, batches, len(nsamp), in_flight, lanes, **kwargs)
            nbatch, padded = len(batches), sum(ns[0] * len(idx) for idx, _, ns in batches)
        used = sum(nsamp)
        stats = {"reads": len(nsamp), "batches": nbatch, "samples": used, "padded_samples": padded,
                 "padded_step_waste": 1.0 - used / float(max(padded, 1)), "failed": cls.failed_reads(nsamp)}
        if streamed:
            stats["streamed"] = True
        return scores, paths, nsamp, stats

    #: the share of the device's free memory call_reads_bucketed_qual gives its resident buckets when no memory_limit is named
    QUAL_MEMORY_FRACTION = 0.5

    @staticmethod
    def _check_footprints(nsamp, names, footprint):
        bytes_of, limit = footprint
        for n, name in zip(nsamp, names):
            if bytes_of(n, 1) > limit:
                raise ValueError("read {}: its {} samples need {} bytes on the device on their own, above its lane's share of {}"
                                 .format(name, n, bytes_of(n, 1), limit))

    def _out_steps(self, nsamp):
        """Rows of the posterior for a read of `nsamp` samples: the sample count mapped through every Convolution's stride."""
        steps = int(nsamp)
        for layer in self.network.layers:
            if isinstance(layer, layers.Convolution):
                steps = max(1, int(layer.out_len(steps)))
        return steps

    def qual_footprint(self, nsamp, reads, checkpoint=True):
        """Device bytes a ragged batch of `reads` reads, the longest of `nsamp` samples, holds while its qualities are made: the
        posterior [T', reads, nstate] float32 and the marginals' workspace (computed from the shapes, nothing is measured)."""
        steps = self._out_steps(nsamp)
        return (4 * steps * reads * (self.nbase ** self.kmer_len + 1)
                + decode.marginals_workspace_bytes(steps, reads, self.nbase, self.kmer_len, checkpoint))

    def _call_padded_qual(self, padded, nsamp, checkpoint=True):
        """_call_padded with qualities: the posterior of the ragged batch, then the checkpointed lattice marginals of every read over
        its own rows, in one launch.  -> (scores, paths, lens, move_row, conf, logz) on the device."""
        with self._scope():
            lengths = layers.ragged_lengths(nsamp)
            post, steps = self._ragged_run(batch.normalise_reads_ragged(padded, lengths), lengths)
            one_launch = decode.marginals_workspace_bytes(post.shape[0], post.shape[1], self.nbase, self.kmer_len, checkpoint)
            return self._marginals(post, steps, checkpoint=checkpoint, workspace_limit=one_launch)

    @classmethod
    def _queue_read_batches_qual(cls, batches, lanes, checkpoint, to_host=True):
        """Every prepared batch queued on its lane (batch k on lane k % lanes), with `to_host` its results' way to the host behind it:
        into pinned memory, so that the copies do not hold the host up and every batch is queued before the first one is done.
        Nothing waits: a lane's posterior and workspace go back to the allocator in stream order, where the lane's next batch finds
        them.  -> [(read indices, host tensors, event, device tensors, lane)]."""
        import torch
        cur = torch.cuda.current_stream()
        pending = []
        for k, (idx, padded, ns) in enumerate(batches):
            bc, s = lanes[k % len(lanes)]
            s.wait_stream(cur)
            with torch.cuda.stream(s):
                padded.record_stream(s)
                res = bc._call_padded_qual(padded, ns, checkpoint)
                host = ()
                if to_host:
                    host = tuple(torch.empty(t.shape, dtype=t.dtype, pin_memory=True).copy_(t, non_blocking=True) for t in res)
                ev = torch.cuda.Event()
                ev.record(s)
            pending.append((idx, host, ev, res, k % len(lanes)))
        return pending

    @classmethod
    def _bucketed_qual(cls, network, signals, trim, open_pore_fraction, max_batch, max_waste, in_flight, lanes, scaling, memory_limit,
                       kwargs, to_host=True):
        """The shared body of call_reads_bucketed_qual and fastq_bucketed -> (pending batches, lanes, nsamp, stats)."""
        import torch
        cls._transducer_only(kwargs, "call_reads_bucketed_qual")
        if not isinstance(network, layers.Serial) or type(network.layers[-1]) is not layers.Softmax:
            raise ValueError("call_reads_bucketed_qual needs a Serial network ending in a Softmax layer")
        kwargs = dict(kwargs)
        checkpoint = kwargs.pop("checkpoint", True)
        if checkpoint is None:
            raise ValueError("call_reads_bucketed_qual runs the checkpointed marginals: checkpoint is True or the rows per checkpoint")
        if lanes is None:
            # as many lanes as the set has buckets by length alone, at most 8 (run_read_batches)
            raw = [len(s) - trim[0] - trim[1] for s in signals if len(s) > trim[0] + trim[1]]
            nlane = max(1, min(8, len(cls.length_buckets(raw, max_batch, max_waste)))) if in_flight is None else in_flight
            lanes = cls.read_lanes(network, nlane, **kwargs)
        bc = lanes[0][0]
        if memory_limit is None:
            # free memory, and what torch's allocator holds without using it (it hands that back when a request needs it)
            idle = torch.cuda.memory_reserved() - torch.cuda.memory_allocated()
            memory_limit = int(cls.QUAL_MEMORY_FRACTION * (torch.cuda.mem_get_info()[0] + idle))
        share = int(memory_limit) // len(lanes)

        def bytes_of(nsamp, reads):
            return bc.qual_footprint(nsamp, reads, checkpoint)

        if open_pore_fraction == 0:
            # what the host knows without a launch: trimming takes exactly trim[0] + trim[1] samples off a read that can be called
            cls._check_footprints([max(1, len(s) - trim[0] - trim[1]) for s in signals], range(len(signals)), (bytes_of, share))
        batches, nsamp = cls.prepare_read_batches(network, signals, trim, open_pore_fraction, max_batch, max_waste, scaling=scaling,
                                                  footprint=(bytes_of, share), **kwargs)
        pending = cls._queue_read_batches_qual(batches, lanes, checkpoint, to_host)
        used, padded = sum(nsamp), sum(ns[0] * len(idx) for idx, _, ns in batches)
        every = decode.marginals_rows_per_checkpoint(checkpoint)
        stats = {"reads": len(nsamp), "batches": len(batches), "samples": used, "padded_samples": padded,
                 "padded_step_waste": 1.0 - used / float(max(padded, 1)), "failed": cls.failed_reads(nsamp),
                 "lanes": len(lanes), "memory_limit": int(memory_limit),
                 "peak_bucket_bytes": max([bytes_of(ns[0], len(idx)) for idx, _, ns in batches] or [0]),
                 "rows_per_checkpoint": every or decode.marginals_default_rows(bc.nbase, bc.kmer_len)}
        return pending, lanes, nsamp, stats

    @classmethod
    def call_reads_bucketed_qual(cls, network, signals, trim=(0, 0), open_pore_fraction=0.0, max_batch=256, max_waste=0.08,
                                 in_flight=None, lanes=None, scaling=None, memory_limit=None, **kwargs):
        """call_reads_bucketed with a confidence per called position (design/lattice_marginals.md 8): the same preparation
        (prepare_read_batches), buckets and lanes; per bucket the ragged posterior (_ragged_run) and the checkpointed lattice marginals
        (slk_viterbi_marginals_ckpt_f32) of every read over its own rows.  Each read gets bit for bit what call_reads_qual([read])
        gives.  -> (scores [N] float32, paths, move_rows, confs: lists of N host arrays (int32, int32, float64, one entry per called
        position), logz [N] float64, sample counts [N], stats), all on the host.  A read that cannot be called is reported and left
        out as call_reads_bucketed does it: score and logz NaN, path, move rows and confidences None, sample count 0, listed in
        stats["failed"].

        memory_limit: the bytes of posterior plus marginals workspace that the buckets resident at one time -- one per lane -- may
        hold together (default: QUAL_MEMORY_FRACTION of the device's free memory, what torch's allocator holds idle counted as free,
        read once per call).  It is a condition on computed sizes:
        a bucket is closed before it outgrows its lane's share, memory_limit / lanes (length_buckets' footprint), and a read that
        exceeds the share on its own raises ValueError naming the read before the network or the marginals are launched for any
        read.  stats holds "memory_limit", "peak_bucket_bytes" (the largest bucket's computed footprint), "lanes" and
        "rows_per_checkpoint".  The set is always prepared first (no streamed upload).  kwargs: Basecaller's, and `checkpoint` (True,
        or the rows per checkpoint) for decode.viterbi_marginals_batch."""
        pending, _, nsamp, stats = cls._bucketed_qual(network, signals, trim, open_pore_fraction, max_batch, max_waste, in_flight, lanes,
                                                      scaling, memory_limit, kwargs)
        n = len(nsamp)
        scores, logz = np.full(n, np.nan, dtype=np.float32), np.full(n, np.nan, dtype=np.float64)
        paths, rows, confs = [None] * n, [None] * n, [None] * n
        for idx, host, ev, _, _ in pending:
            ev.synchronize()
            sc, pa, le, mr, cf, lz = (h.numpy() for h in host)
            for j, i in enumerate(idx):
                scores[i], logz[i] = sc[j], lz[j]
                paths[i], rows[i], confs[i] = pa[j, :le[j]].copy(), mr[j, :le[j]].copy(), cf[j, :le[j]].copy()
        return scores, paths, rows, confs, logz, nsamp, stats

    @classmethod
    def fastq_bucketed(cls, network, signals, names=None, trim=(0, 0), open_pore_fraction=0.0, max_batch=256, max_waste=0.08,
                       in_flight=None, lanes=None, scaling=None, memory_limit=None, alphabet='ACGT', qmax=60, **kwargs):
        """Whole read sets -> FASTQ records: call_reads_bucketed_qual's flow, letters and Phred values per bucket on the device
        (bio.paths_to_bases_qual).  -> a list with one four-line record per read -- character for character the record call_fastq
        gives for that read -- and None for a read that could not be called; names default to read0, read1, ..."""
        import torch
        from . import bio
        pending, lanes, nsamp, _ = cls._bucketed_qual(network, signals, trim, open_pore_fraction, max_batch, max_waste, in_flight, lanes,
                                                      scaling, memory_limit, kwargs, to_host=False)
        if names is None:
            names = ["read%d" % r for r in range(len(nsamp))]
        records = [None] * len(nsamp)
        for idx, _, ev, res, lane in pending:                  # every bucket is queued by now: the lanes run while the host reads
            bc, s = lanes[lane]
            with torch.cuda.stream(s):
                calls = bio.paths_to_bases_qual(res[1], res[2], res[4], bc.kmer_len, alphabet, qmax=qmax)
            for i, (seq, q) in zip(idx, calls):
                records[i] = bio.fastq_text([names[i]], [seq], [q])
        return records

    _UPLOAD_STREAMS = {}

    @classmethod
    def _call_reads_streamed(cls, network, signals, trim, max_batch, max_waste, in_flight, lanes, window_size=100, scaling=None, **kwargs):
        """call_reads_bucketed for a big set with the CLI's open-pore fraction of 0 (bin/basecall_network.py:71), WITHOUT a round trip to
        the host between the upload of a read and its call: reads are bucketed by their RAW lengths (what the host knows without touching
        a sample; trimming takes at most a few windows off); bucket after bucket the host packs the reads into pinned memory and queues
        the upload on a copy stream, and the bucket's lane does the rest in stream order -- the check for samples that are not finite,
        the window spreads, trim_open_pore + trim_array on the device (slk_open_pore_trim_f32), the zero-padded batch, normalisation,
        network, decoder, results and trimmed lengths to the host.  The host packs bucket k + 1 while the device runs bucket k: what is
        left in front of the network is the first bucket's upload (round 5: 85 ms of packing, upload and trimming for 4096 reads before
        the first network kernel).  A read that fails on the device keeps its place in its bucket with length 0 (columns of a batch never
        mix); a read shorter than one window goes into no bucket.  Every failed read is reported on stderr like the reference's worker
        does (basecall.py:103-115) and comes back with score NaN and path None.
        With `scaling` (int16 reads, call_reads_bucketed) the staging area and the upload hold int16 samples, and the lane's first kernel
        scales them (slk_adc_to_pa_i16), its flags standing in for the check for samples that are not finite.
        -> (scores, paths, nsamp, number of batches, padded samples)."""
        import concurrent.futures
        import torch
        from . import device as D
        dev = D.device()
        nread = len(signals)
        raw = [len(s) for s in signals]
        dtype, offset, scale = batch.read_set_scaling(signals, scaling)
        # a read shorter than one window has no window to trim by: the reference's function fails on it (flag 2), after the check for
        # samples that are not finite (flag 1), taken here on the host for these few samples as the device would take it
        flags = [0] * nread
        with np.errstate(all="ignore"):
            for i in (i for i in range(nread) if raw[i] < window_size):
                pa = ((np.asarray(signals[i], dtype=np.float64) + offset[i]) * scale[i]).astype(np.float32)
                flags[i] = 2 | int(not np.isfinite(pa).all())
        live = [i for i in range(nread) if not flags[i]]
        buckets = [[live[j] for j in sub] for sub in cls.length_buckets([raw[i] for i in live], max_batch, max_waste)]
        if lanes is None:
            lanes = cls.read_lanes(network, max(1, min(8, len(buckets))) if in_flight is None else in_flight, **kwargs)
        up = cls._UPLOAD_STREAMS.get(dev.index)
        if up is None:
            up = cls._UPLOAD_STREAMS[dev.index] = torch.cuda.Stream()
        # the whole set in one pinned staging area, laid out bucket after bucket
        order = [i for idx in buckets for i in idx]
        sigs = [signals[i] for i in order]
        strides, off = batch.read_layout([raw[i] for i in order], window_size)
        assert trim[0] >= 0 and trim[1] >= 0
        pending, widths, lo = [], [], 0
        with concurrent.futures.ThreadPoolExecutor(min(8, os.cpu_count() or 1)) as pool, \
                batch.staging(int(off[-1]), dtype, up) as buf:
            hv = buf.numpy()
            for k, idx in enumerate(buckets):
                n, hi = len(idx), lo + len(idx)
                step = max(1, -(-n // 8))
                list(pool.map(lambda a: batch.fill_staging(hv, sigs, off, a, min(hi, a + step)), range(lo, hi, step)))
                base, max_stride = int(off[lo]), int(strides[lo:hi].max())
                with torch.cuda.stream(up):
                    # (`upload` lives until the next bucket's replaces it: int16 samples released right after their conversion made
                    #  about one call in three 60 ms slower)
                    upload = buf[base: int(off[hi])].to(dev, non_blocking=True)
                    meta = batch._read_meta(off[lo:hi] - base, [raw[i] for i in idx], strides[lo:hi], offset[idx], scale[idx], dev)
                    uploaded = torch.cuda.Event()
                    uploaded.record(up)
                bc, lane = lanes[k % len(lanes)]
                with torch.cuda.stream(lane):
                    lane.wait_event(uploaded)
                    upload.record_stream(lane)
                    meta[0].record_stream(lane)
                    sig, fl = batch.picoamperes(upload, meta, max_stride)
                    first_sample, rawlen = meta[0], meta[1]
                    spread = batch._window_spread(sig.view(-1, window_size))
                    first_win, nwin = first_sample // window_size, rawlen // window_size
                    start = torch.empty((n,), dtype=torch.int64, device=dev)
                    ln = torch.empty((n,), dtype=torch.int32, device=dev)
                    _lib.check(_lib.lib().slk_open_pore_trim_f32(spread.data_ptr(), first_win.data_ptr(), nwin.data_ptr(),
                                                                 first_sample.data_ptr(), n, window_size, int(trim[0]), int(trim[1]),
                                                                 start.data_ptr(), ln.data_ptr(), fl.data_ptr(), D.stream_ptr()),
                               "open_pore_trim")
                    lmax = max(raw[i] for i in idx)                    # (an upper bound of the trimmed lengths: the batch's row width)
                    # a failed read (length 0) runs as one zero sample: its column is garbage nobody reads
                    res = bc._call_padded(batch.pack_batch(sig, start, ln, lmax), ln.clamp(min=1))
                    host = tuple(t.to("cpu", non_blocking=True) for t in res + (ln, fl))
                    ev = torch.cuda.Event()
                    ev.record(lane)
                pending.append((idx, host, ev, res))
                widths.append(lmax)
                lo = hi
        scores, paths = cls._collect_reads(pending, nread)
        # the trimmed lengths and the flags came down behind the results; a read that failed on the device has neither score nor path
        nsamp = [0] * nread
        for idx, host, _, _ in pending:
            ns, fb = host[3].numpy(), host[4].numpy()
            for j, i in enumerate(idx):
                flags[i] = int(fb[j])
                if flags[i]:
                    scores[i], paths[i] = np.nan, None
                else:
                    nsamp[i] = int(ns[j])
        cls._report_failures(flags)
        return scores, paths, nsamp, len(buckets), sum(w * len(p[0]) for w, p in zip(widths, pending))

    def call_chunks_host(self, chunks):
        scores, paths, lens = self.call_chunks(chunks)
        scores, paths, lens = scores.cpu().numpy(), paths.cpu().numpy(), lens.cpu().numpy()
        return scores, [paths[i, : lens[i]].tolist() for i in range(len(lens))]


def synthetic_chunks(nchunk, chunk_len=4000, seed=0xdeadbeef, dwell=10.0, noise=0.15, first_chunk=0):
    """Synthetic raw signal: per chunk, piecewise-constant levels ~N(0,1) with geometric dwell
    (mean `dwell` samples) plus N(0, noise^2), RandomState(seed + chunk_id), scaled to a pA-like range so that
    normalisation does real work.  float32 [nchunk, chunk_len]."""
    out = np.empty((nchunk, chunk_len), dtype=np.float32)
    for c in range(nchunk):
        rs = np.random.RandomState((seed + first_chunk + c) % (2 ** 32))
        nseg = int(chunk_len / dwell * 2) + 16
        d = rs.geometric(1.0 / dwell, size=nseg)
        while d.sum() < chunk_len:
            d = np.concatenate([d, rs.geometric(1.0 / dwell, size=nseg)])
        levels = rs.normal(size=len(d))
        sig = np.repeat(levels, d)[:chunk_len]
        sig = sig + rs.normal(scale=noise, size=chunk_len)
        out[c] = (sig * 12.0 + 90.0).astype(np.float32)
    return out
