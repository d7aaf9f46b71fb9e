"""
Train-step contract of the reference trainer, on the HIP engine.

Mirrors `ecg_transformer/models/train.py`:
  get_train_args (:407-436)  -- same defaults, same `steps_per_epoch = ceil(n_train // bsz)` floor-first quirk (:433)
  the optimiser / scheduler wiring of MyTrainer.train (:241-252)
  the step body (:268-283): zero_grad -> forward -> backward -> clip_grad_norm_(1.0, error_if_nonfinite) -> AdamW -> sched

`HipTrainStep` runs that body fused on flat HBM buffers: one sum-of-squares pass over the flat gradient, one
clip+AdamW pass that also refreshes the bf16 weight shadow, no per-parameter launches.  `error_if_nonfinite=True` is
honoured in the SAME step, as the reference does (train.py:281): the kernel skips the whole update on a non-finite norm and
the step reads the flag back before it returns (`sync_nonfinite=False` defers that read by one step to keep the host running
ahead of the device).  Data parallel (reference has none): one process per GPU; the replicas are made identical
once (broadcast of rank 0's flat parameter buffer), every rank draws its own dropout masks (rank folded into the seed), and
gradients are all-reduced over RCCL in per-layer buckets of the flat gradient buffer (28 MB f32 / 14 MB bf16 each for base),
each launched asynchronously the moment the backward pass has finished that layer (head, layers L-1..0, embedding), so the
exchange overlaps the remaining backward.

Logging / TensorBoard / sklearn metrics / datasets of MyTrainer are host-side and out of scope here.
"""
import math
import numbers
import sys

import torch
import torch.distributed as dist

from .check_args import ca
from . import hip
from . import ddp
from .engine import check_lengths, ragged_slice, RawPaddedBatch, LN_EPS


def get_train_args(args=None, n_train=None):
    """the reference's defaults, key for key.  One key of this project rides along when given: micro_batch_size (the default of
    HipTrainStep.step / step_masked; absent = None, the whole batch in one pass) -- the reference's TODO at train.py:431"""
    default_args = dict(
        num_train_epoch=3,
        train_batch_size=64,
        eval_batch_size=64,
        do_eval=True,
        optimizer='AdamW',
        learning_rate=3e-4,
        weight_decay=1e-2,
        warmup_ratio=0.05,
        schedule='cosine',
        n_sample=None,
        augment_timeout=False,
        patience=8,
        precision=16 if torch.cuda.is_available() else 'bf16',  # carried, unused by the reference's live trainer too
        log_per_epoch=False,
        log_to_console=True,
        save_every_n_epoch=False,
        save_top_k=-1,
        tqdm=False
    )
    args_ = default_args
    if args is not None:
        args_.update(args)
    args_['steps_per_epoch'] = steps_per_epoch = math.ceil((n_train or int(sys.maxsize)) // args_['train_batch_size'])
    args_['n_step'] = steps_per_epoch * args_['num_train_epoch']
    ca(optimizer=args_['optimizer'], schedule=args_['schedule'])
    check_micro_batch_size(args_.get('micro_batch_size'))
    return args_


def lr_multiplier(schedule, n_warmup, n_step):
    """HF get_constant_schedule_with_warmup / get_cosine_schedule_with_warmup (num_cycles=0.5) lambdas (train.py:245-252)."""
    ca(schedule=schedule)

    def f(step):
        if step < n_warmup:
            return float(step) / float(max(1, n_warmup))
        if schedule == 'constant':
            return 1.0
        progress = float(step - n_warmup) / float(max(1, n_step - n_warmup))
        return max(0.0, 0.5 * (1.0 + math.cos(math.pi * 0.5 * 2.0 * progress)))
    return f


def check_micro_batch_size(value):
    """None (the whole batch in one pass) or a positive int, else ValueError"""
    if value is None:
        return None
    if isinstance(value, bool) or not isinstance(value, numbers.Integral) or value <= 0:
        raise ValueError(f'micro_batch_size must be a positive int or None, got {value!r}')
    return int(value)


class HipTrainStep:
    """
    step(sample_values, labels) == reference train.py:271-283 for one batch, fused.

    args: dict as produced by `get_train_args` (uses optimizer, learning_rate, weight_decay, warmup_ratio, schedule, n_step, and
    micro_batch_size: the default of `step` / `step_masked`).

    Every step, `step` and `step_masked` alike, is ONE loop over passes (`_run`): the record ranges [s, e) of `_cuts` -- the whole batch, or
    with micro_batch_size=m < B (gradient accumulation) the ceil(B/m) consecutive slices [s, s+m), the last maybe shorter, at the activation
    memory of m records -- then ONE clip + AdamW update (`_update`).  A pass draws its dropout seed, runs the objective's forward and then its
    backward; the objective (`_Supervised`, `_Masked`) says how a pass's inputs are cut, where its output rows land, what it weighs and how the
    whole batch's loss comes about, nothing else.  The one-pass step touches no accumulator.  In a split step each backward pass overwrites
    the flat gradient buffer as usual; `ecgvit_grad_accumulate` sums it into a second flat buffer (`gacc`, allocated on the first split
    batch) and folds the sum back before the norm, the data-parallel exchange (armed in the last pass only) and the optimiser.  Up to f32
    summation order this is the full batch's step when dropout is 0.  With dropout every pass draws its own seed, so the masks are not those
    of the unsplit batch.
    """

    def __init__(self, model, args=None, max_grad_norm=1.0, sync_nonfinite=True, process_group=None, overlap_allreduce=True,
                 grad_comm_dtype=torch.float32, single_rank_collectives=False):
        """grad_comm_dtype: torch.float32 (exact exchange) or torch.bfloat16 (each bucket is cast to bf16, all-reduced at half the
        bytes over xGMI and added back into the f32 gradient buffer; the optimiser still sees f32).
        single_rank_collectives: run the start broadcast and the gradient exchange on a 1-rank group too (skipped otherwise), so
        that the whole RCCL path -- collective stream, staging buffers, chunked GEMM launches -- can be exercised on one GPU"""
        self.model = model
        self.args = {**get_train_args(), **(args or dict())}
        ca(optimizer=self.args['optimizer'], schedule=self.args['schedule'])
        self.lr0, self.wd = self.args['learning_rate'], self.args['weight_decay']
        n_step = self.args['n_step']
        self.mult = lr_multiplier(self.args['schedule'], round(n_step * self.args['warmup_ratio']), n_step)
        self.decoupled = self.args['optimizer'] == 'AdamW'
        self.max_grad_norm = max_grad_norm
        self.sync_nonfinite = sync_nonfinite
        self.step_count = 0       # optimiser steps taken == scheduler.step() calls
        self.m = self.v = None
        self.norm_out = self.sumsq = self.ws = None
        self.last_loss = None
        self.pg = process_group
        self.world = dist.get_world_size(process_group) if (dist.is_available() and dist.is_initialized()) else 1
        self.rank = dist.get_rank(process_group) if self.world > 1 else 0
        self.collectives = self.world > 1 or (bool(single_rank_collectives) and dist.is_available() and dist.is_initialized())
        self.overlap = overlap_allreduce
        if grad_comm_dtype not in (torch.float32, torch.bfloat16):
            raise ValueError('grad_comm_dtype must be torch.float32 or torch.bfloat16')
        self.comm_dtype = grad_comm_dtype
        self._xchg = self._xchg_layout = None
        self._replicas_synced = False
        # frozen parameters (requires_grad=False), read every step: the flags the span table below was built for, per-parameter step offsets
        # (a parameter's own optimiser step = step_count + lag, as torch keeps state['step'] per parameter), the span table
        self._flags = None
        self._flags_dirty = False
        self._lag = None
        self._spans = None          # None: every parameter trainable at the global step -> the whole-buffer kernels
        self._trainable = None      # names (None = all), for the backward plan and the weight-shadow refresh
        # gradient accumulation: the default micro-batch size, the accumulator (flat f32, the gradient buffer's layout), its span tables
        self.micro_batch_size = check_micro_batch_size(self.args.get('micro_batch_size'))
        self.gacc = None
        self._acc_tables = None     # (key, whole table, {bucket tag: table}) -- a table is (device int64 [n][3], n, total)

    # -- lr as the reference logs it: scheduler.get_last_lr() after `step_count` scheduler steps
    def get_last_lr(self):
        return self.lr0 * self.mult(self.step_count)

    def _alloc_state(self, numel, device):
        """the optimiser moments over `numel` elements and what the norm and its readbacks need; True when they were (re)allocated"""
        if self.m is not None and self.m.device == device and self.m.numel() == numel:
            return False
        self.m = torch.zeros(numel, device=device, dtype=torch.float32)
        self.v = torch.zeros_like(self.m)
        self.norm_out = torch.zeros(2, device=device, dtype=torch.float32)
        self.norm_host = torch.ones(2, dtype=torch.float32).pin_memory()
        self.sumsq_host = torch.zeros(1, dtype=torch.float32).pin_memory()
        self._flag_event = torch.cuda.Event()
        self._norm_event = torch.cuda.Event()
        self.sumsq = torch.zeros(1, device=device, dtype=torch.float32)
        self.ws = torch.empty(hip.lib().ecgvit_sumsq_workspace(numel), device=device, dtype=torch.uint8)
        return True

    def _state(self):
        m = self.model.encoder if hasattr(self.model, 'encoder') else self.model
        m._engine()
        if self._alloc_state(m._pflat.numel(), m._pflat.device):
            self._replicas_synced = False
            self._flags_dirty = True
        if self.collectives and not self._replicas_synced:
            # data-parallel replicas must start from the same weights whatever each rank's RNG produced: rank 0's flat buffer wins
            ddp.broadcast_flat_(m._pflat, src=0, group=self.pg, single_rank=True)
            if m._wlow is not None:
                m.refresh_low_precision_weights(force=True)
            self._replicas_synced = True

    # -- frozen parameters: host work only, every step
    def _read_flags(self, model):
        """read the requires_grad flags (before any launch: a step with no trainable parameter raises ValueError); a changed set is
        applied by `_apply_flags` once the buffers exist"""
        flags = tuple(p.requires_grad for p in model._param_list)
        if not any(flags):
            raise ValueError('no trainable parameter: every parameter has requires_grad=False')
        if self._lag is None or len(self._lag) != len(flags):
            self._lag = [0] * len(flags)
            self._flags = None
        if flags != self._flags:
            self._flags, self._flags_dirty = flags, True

    def _apply_flags(self, model):
        """the frozen set changed: agree on it with the other ranks, rebuild the span table, the trainable names and the exchange layout"""
        if not self._flags_dirty:
            return
        flags = self._flags
        if self.collectives:
            # every rank's bucket sequence follows its frozen set: ranks that disagreed would post mismatched collectives and hang
            ddp.check_same_frozen_set(flags, group=self.pg, device=model._pflat.device, single_rank=True)
        names = model._param_names
        rows = span_table(model._layout, names, flags, self._lag)
        if rows is None:
            self._spans, self._trainable = None, None
        else:
            self._spans = (torch.tensor(rows, dtype=torch.int64, device=model._pflat.device), len(rows), sum(r[1] for r in rows))
            self._trainable = [n for n, f in zip(names, flags) if f]
            need = hip.lib().ecgvit_sumsq_spans_workspace(len(rows))
            if need > self.ws.numel():
                self.ws = torch.empty(need, device=model._pflat.device, dtype=torch.uint8)
        self._xchg = None   # the exchange layout follows the frozen set
        self._flags_dirty = False

    def _dropout_seed(self, model):
        """one fresh seed per step from the host RNG; the rank is folded in so that replicas seeded identically (as DDP scripts
        do) still drop different units of their different records"""
        if not model._has_dropout:
            return 0
        base = int(torch.randint(0, 2 ** 31 - 1, (1,)).item())
        return (base + 0x3C6EF35F * self.rank) % (2 ** 31 - 1)

    # -- gradient all-reduce (RCCL over xGMI): ddp.GradExchange over the flat gradient buffer
    def _arm_overlap(self, model):
        eng = model._engine()
        if self.collectives:
            if self._xchg is None or self._xchg_layout is not model._layout:
                ranges = model._layout.buckets_in_ready_order(eng.Ly)
                if self._trainable is not None:   # frozen parameters: only the trainable part of a bucket travels; frozen buckets never do
                    ranges = trainable_ranges(model._layout, ranges, self._trainable)
                self._xchg = ddp.GradExchange(ranges, group=self.pg, overlap=self.overlap,
                                              comm_dtype=self.comm_dtype, single_rank_collectives=True)
                self._xchg_layout = model._layout
            self._xchg.begin(model._gflat)
            eng.on_grads_ready = self._xchg.bucket_ready if self.overlap else None
            # RCCL kernels will hold CUs while the rest of the backward runs: hand the GEMM tiles out in small chunks instead of
            # static per-CU shares (profiles/r02_contention.txt: 8 held CUs cost a static launch +52 %, a chunked one +9 %) -- an argument of
            # THIS backward pass, not process state
            return 2 if self.overlap else 0
        eng.on_grads_ready = None
        return 0

    def step_masked(self, sample_values, mask_idx, micro_batch_size=None, lengths=None, mask_counts=None):
        """the same fused step for the masked pre-train objective; `self.model` must be a MaskedEcgVit.
        micro_batch_size: as `step` (None: the default given in args); the loss is the whole batch's mean.
        lengths, mask_counts: records of unequal length (MaskedEcgVit.forward) -- sample_values (B, C, L') or a ragged (C, S) batch, mask_idx
        flat; micro-batches are then record ranges (a ragged one a ragged batch of its own), pass j weighted by its share of the masked
        patches.  Under a per-record input transform lengths are RAW sample counts and record b has padded_length(l_b) / P patches; the
        targets are the transformed patches.  Returns (loss, reconstruction (sum m_b, C*P))."""
        wrapper, model = self.model, self.model.encoder
        # (host work only, before anything launches)
        mb, eng, geo = self._begin(model, micro_batch_size, lambda: wrapper.check_varlen_input(sample_values, mask_idx, lengths, mask_counts))
        if geo is not None:
            rect = geo.as_rectangular(model.config.max_signal_length)
            if rect is not None:   # every record full-width with one mask count: the rectangular step itself
                mask_idx, geo = rect, None
        cuts = _cuts(sample_values.shape[0] if geo is None else geo.B, mb)
        return self._run(model, eng, _Masked(self, wrapper, eng, sample_values, mask_idx, geo, cuts))

    def _device_mask_idx(self, mask_idx, device):
        """the (B, m) mask indices as a contiguous int32 device tensor"""
        if mask_idx.is_cuda:
            return mask_idx.to(dtype=torch.int32).contiguous()
        # host indices (checked on the host by the caller) travel through a pinned staging buffer: a pageable-memory copy would block the host
        # until the device has drained the stream, i.e. once per step.  The buffer is rewritten only after its last copy has left it (an event:
        # normally long past -- with the deferred non-finite check the host may be a step ahead)
        st = getattr(self, '_mask_stage', None)
        if st is None or st[0].shape != mask_idx.shape:
            st = (torch.empty(mask_idx.shape, dtype=torch.int32).pin_memory(), torch.empty(mask_idx.shape, dtype=torch.int32, device=device),
                  torch.cuda.Event())
            self._mask_stage = st
        else:
            st[2].synchronize()
        st[0].copy_(mask_idx)
        st[1].copy_(st[0], non_blocking=True)
        st[2].record()
        return st[1]

    def _update(self, model, lo=0, hi=None):
        """the optimiser update over the whole flat buffers, or over their range [lo, hi) (the moments are then sized to it)"""
        gflat, pflat, wlow = model._gflat, model._pflat, model._wlow
        if hi is not None:
            gflat, pflat, wlow = gflat[lo:hi], pflat[lo:hi], None if wlow is None else wlow[lo:hi]
        if self.collectives:
            self._xchg.finish()
        st = hip.stream()
        spans = self._spans   # frozen parameters: the norm of the trainable gradients only
        _sumsq(gflat, spans, self.sumsq, self.ws)
        # The non-finite decision needs only the sum of squares (the optimiser kernel's test is isfinite(sqrt(sumsq) * |1/world|)): its
        # readback goes out HERE, ahead of the optimiser and the weight-shadow transposes, so that the same-step check below lets the host
        # go on ~0.8 ms before the device has finished the step -- the Python prelude of the next step then runs under those kernels instead
        # of after them (under rocprofv3 the device idled 0.8 ms per step at the step boundary; unprofiled the change is worth 0.2 ms:
        # 6601 -> 6616 records/s, four alternating pairs on one device)
        self.sumsq_host.copy_(self.sumsq, non_blocking=True)
        self._flag_event.record()
        self.step_count += 1
        lr = self.lr0 * self.mult(self.step_count - 1)  # lr in effect for this optimiser step
        wlow = hip.ptr(wlow)
        if spans is None:
            hip.run.ecgvit_adamw_step(
                pflat.data_ptr(), gflat.data_ptr(), self.m.data_ptr(), self.v.data_ptr(), wlow, gflat.numel(), self.sumsq.data_ptr(),
                1.0 / self.world, self.max_grad_norm, lr, 0.9, 0.999, 1e-8, self.wd, self.step_count, 1 if self.decoupled else 0,
                self.norm_out.data_ptr(), st)
        else:
            # frozen parameters: no update, no decay, no moment update; each span at its own step (the lr follows the global one)
            hip.run.ecgvit_adamw_step_spans(
                pflat.data_ptr(), gflat.data_ptr(), self.m.data_ptr(), self.v.data_ptr(), wlow, spans[0].data_ptr(), spans[1], spans[2],
                self.sumsq.data_ptr(), 1.0 / self.world, self.max_grad_norm, lr, 0.9, 0.999, 1e-8, self.wd, self.step_count,
                1 if self.decoupled else 0, self.norm_out.data_ptr(), st)
            for i, f in enumerate(self._flags):
                if not f:
                    self._lag[i] -= 1   # a frozen parameter's own step count stands still
        model.refresh_transposed_weights(only=self._trainable)   # the optimiser kernel rewrote the bf16 shadows (of the trainable weights)
        # non-blocking readback of (norm, finite flag) as the kernel computed them: only read if the early check fires (the message's norm)
        self.norm_host.copy_(self.norm_out, non_blocking=True)
        self._norm_event.record()
        self._flag_pending = True
        if self.sync_nonfinite:
            self._raise_if_flagged(wait=True)

    def step(self, sample_values, labels, lengths=None, micro_batch_size=None):
        """one fused training step; lengths: optional (B,) per-record sample counts (EcgVit.forward).
        micro_batch_size: None (the default given in args) or a positive int m; m < B accumulates the gradient of ceil(B/m) passes into one
        optimiser step (see the class docstring; with dropout each pass draws its own masks).  Returns (loss_mean, logits (B, K)) of the
        whole batch either way.
        sample_values may be a ragged (C, S) batch with its (B,) lengths (EcgVit.forward); micro-batches are then record ranges, each a
        ragged batch of its own.  The last block then runs in full (no CLS-only pruning).
        Under a per-record input transform (`FusedInputTransform(per_record=True)`) sample_values holds RAW records -- (B, C, W) or a ragged
        (C, S_raw) batch -- and lengths their raw sample counts; TimeOut spans are drawn per record in batch order, micro-batch by
        micro-batch, so the draws of a split step are those of the unsplit one."""
        model = self.model
        mb, eng, _ = self._begin(model, micro_batch_size)
        # the classifier reads the CLS rows only: the last block skips the other rows past its K / V (bf16 engine; the fp8 step keeps the
        # full block -- its 512-row products would fall below the 8-bit kernels' gates and change the delayed-scaling sites)
        cls_only = eng.dtype == torch.bfloat16 and not eng.fp8
        ragged = sample_values.dim() == 2
        if ragged:   # (C, S): validated once, before anything launches (the RaggedBatch travels on); B = the number of records
            sample_values = sample_values.contiguous().float()
            lengths = eng.check_ragged_input(sample_values, lengths, labels)
        elif eng.input_transform is not None and eng.input_transform.per_record:
            # RAW records (B, C, W): validated once (the RawPaddedBatch travels on, micro-batches keep the whole batch's pass width)
            lengths = eng.check_raw_input(sample_values, lengths)
        cuts = _cuts(labels.shape[0] if ragged else sample_values.shape[0], mb)
        return self._run(model, eng, _Supervised(self, model, eng, sample_values, labels, lengths, cuts, cls_only))

    def _begin(self, model, micro_batch_size, validate=None):
        """the prelude of every step: the host-only validation (micro_batch_size, then `validate()`) before anything touches the device, the
        eval-mode refusal, the frozen set, the optimiser state, the pending non-finite check -> (micro_batch_size, engine, validate())"""
        mb = self.micro_batch_size if micro_batch_size is None else check_micro_batch_size(micro_batch_size)
        checked = None if validate is None else validate()
        if not model.training:
            raise RuntimeError('train step on a model in eval mode')
        self._read_flags(model)
        self._state()
        self._apply_flags(model)
        self._raise_if_flagged()
        return mb, model._engine(), checked

    def _run(self, model, eng, obj):
        """THE pass loop: one optimiser step as the passes `obj.cuts` of the objective `obj`.  Per pass: a fresh dropout seed,
        `obj.forward(j, s, e, seed)` -> that pass's backward, `backward(tiles_per_workgroup)`.  Only the last pass is armed for the exchange.
        A split step sums the passes' gradients: acc = g (pass 0) or acc += g, and in the last pass g += acc -- over each bucket as the
        backward reports it final, right before its all-reduce goes out (overlapped exchange), else over every span after the pass.  The
        number of collectives per optimiser step does not change, and the one-pass step never touches the accumulator."""
        split, overlapped = len(obj.cuts) > 1, self.collectives and self.overlap
        for j, (s, e) in enumerate(obj.cuts):
            last = j == len(obj.cuts) - 1
            seed = self._dropout_seed(model)
            backward = obj.forward(j, s, e, seed)
            model._fwd_id += 1
            eng.on_grads_ready, tpw = None, 0
            if last:
                tpw = self._arm_overlap(model)
                if split and overlapped:
                    eng.on_grads_ready = self._fold_then_send(model)
            try:
                backward(tpw)
            finally:
                eng.on_grads_ready = None
            if split and not (last and overlapped):
                self._accumulate(model, hip.ACC_FOLD if last else hip.ACC_INIT if j == 0 else hip.ACC_ADD, self._acc_state(model)[0])
        loss, out = obj.result()
        self._update(model)
        self.last_loss = loss
        return loss, out

    def _const(self, device, key, values, dtype=torch.float32):
        """a small constant device tensor, made once per key"""
        cache = self.__dict__.setdefault('_consts', {})
        if (key, device) not in cache:
            cache[(key, device)] = torch.tensor(values, dtype=dtype, device=device)
        return cache[(key, device)]

    def _acc_state(self, model):
        """the accumulator and its span tables: the whole table (the trainable spans, or one whole-buffer span) and, with an overlapped
        exchange, one table per exchanged bucket (its range inside the trainable spans), rebuilt with the span table or the exchange"""
        g = model._gflat
        if self.gacc is None or self.gacc.numel() != g.numel() or self.gacc.device != g.device:
            self.gacc = torch.zeros_like(g)
        xchg = self._xchg if (self.collectives and self.overlap) else None
        t = self._acc_tables
        if t is None or t[0] is not self._spans or t[1] is not xchg or t[2] != g.numel():
            rows = [[0, g.numel(), 0]] if self._spans is None else self._spans[0].tolist()
            assert all(r[0] % 8 == 0 for r in rows), 'accumulator spans must start on 8-element boundaries'
            whole = (torch.tensor(rows, dtype=torch.int64, device=g.device), len(rows), sum(r[1] for r in rows))
            per = {}
            if xchg is not None:
                for tag, (lo, hi) in xchg.ranges.items():
                    br = [[max(o, lo), min(o + c, hi) - max(o, lo), 0] for o, c, _ in rows if max(o, lo) < min(o + c, hi)]
                    if br:
                        assert all(r[0] % 8 == 0 for r in br), 'bucket ranges must start on 8-element boundaries'
                        per[tag] = (torch.tensor(br, dtype=torch.int64, device=g.device), len(br), sum(r[1] for r in br))
                # the buckets are disjoint; every trainable parameter must lie in one of them, or part of its gradient would never be folded
                trainable = None if self._trainable is None else set(self._trainable)
                folded = [(lo, lo + c) for tab in per.values() for lo, c, _ in tab[0].tolist()]
                for n, (o, _, c) in model._layout.entries.items():
                    if trainable is None or n in trainable:
                        assert any(a <= o and o + c <= b for a, b in folded), f'{n} lies in no exchanged bucket'
            self._acc_tables = (self._spans, xchg, g.numel(), whole, per)
        return self._acc_tables[3], self._acc_tables[4]

    def _accumulate(self, model, mode, table):
        hip.run.ecgvit_grad_accumulate(self.gacc.data_ptr(), model._gflat.data_ptr(), table[0].data_ptr(), table[1], table[2], mode,
                                       1.0, hip.stream())

    def _fold_then_send(self, model):
        """the last pass's `on_grads_ready` under an overlapped exchange: g += acc over a bucket, then its all-reduce"""
        per, folded = self._acc_state(model)[1], set()

        def fold_then_send(tag):
            if tag in per and tag not in folded:
                folded.add(tag)
                self._accumulate(model, hip.ACC_FOLD, per[tag])
            self._xchg.bucket_ready(tag)
        return fold_then_send

    _flag_pending = False

    def _raise_if_flagged(self, wait=False):
        """`clip_grad_norm_(..., error_if_nonfinite=True)` semantics without a per-step host sync: the kernel skips the
        whole update when the norm is non-finite (state stays intact), and the sum of squares it tests is read from pinned memory as
        soon as its copy has landed (`wait=True` blocks for it -- for the copy, issued ahead of the optimiser kernel, not for the step)."""
        if self._flag_pending and (wait or self._flag_event.query()):
            if wait:
                self._flag_event.synchronize()
            self._flag_pending = False
            if not math.isfinite(float(self.sumsq_host[0])):
                self._norm_event.synchronize()
                norm, finite = self.norm_host.tolist()
                if finite == 0.0:
                    raise RuntimeError(f'The total norm for gradients is non-finite ({norm}), so it cannot be clipped.')

    def grad_norm(self):
        """pre-clip global gradient L2 norm of the last step (device sync)"""
        return float(self.norm_out[0].item())

    def finish(self):
        """drain the deferred non-finite check (call after the last step)"""
        self._raise_if_flagged(wait=True)


class HipProbeStep(HipTrainStep):
    """
    The linear probe on CACHED features: `step(features, labels)` is the step `HipTrainStep.step` takes with every parameter but
    `vit.mlp_head.*` frozen and dropout 0, started after the encoder instead of before it.  features: (B, hidden_size) f32 as
    `EcgVit.encode(..., norm=False)` / `HipEncoder(model, norm=False).encode` return them (the pooled residual-stream vector: the head's own
    LayerNorm is part of what is trained).

    One step: `ecgvit_head_fwd` over one row per record, BCE with the model's `loss_weight` and 'mean' reduction, `ecgvit_head_bwd`, the
    global clip at `max_grad_norm` with the non-finite error, AdamW (torch defaults) and the warm-up / cosine schedule of `args` -- the
    kernels, hyper-parameters and `get_last_lr()` / `grad_norm()` / `finish()` surface of `HipTrainStep`, over the head's range of the flat
    buffers only (its optimiser moments are the only state this class allocates).  The encoder parameters are neither read nor written and
    need not be frozen; no encoder activation is touched, so a step never invalidates a pending backward.  Single device; no micro-batches.
    """

    def __init__(self, model, args=None, max_grad_norm=1.0, sync_nonfinite=True):
        super().__init__(model, args, max_grad_norm=max_grad_norm, sync_nonfinite=sync_nonfinite)
        self.world, self.rank, self.collectives = 1, 0, False   # single device by definition
        self._buf = None

    def step_masked(self, *a, **kw):
        raise TypeError('HipProbeStep trains the classification head on cached features: it has no masked step')

    def _state(self):
        model = self.model
        model._engine()
        lo, hi = model._layout.span(lambda n: n.startswith('vit.mlp_head.'))
        self._alloc_state(hi - lo, model._pflat.device)
        if self._trainable is None:   # (`_update` refreshes the shadows of these only)
            self._trainable = [n for n in model._param_names if n.startswith('vit.mlp_head.')]
        return lo, hi

    def step(self, features, labels):
        """features (B, hidden_size) f32 on the device, labels (B, K).  Returns (loss_mean, logits (B, K)), fresh tensors."""
        model = self.model
        if not features.is_cuda:
            raise RuntimeError('HipProbeStep runs on the device (no CPU fallback exists): pass device tensors')
        d, K = model.config.hidden_size, model.num_class
        if features.dim() != 2 or features.shape[1] != d:
            raise ValueError(f'features must be (B, hidden_size={d}) as EcgVit.encode(..., norm=False) returns them, got {tuple(features.shape)}')
        if labels.dim() != 2 or tuple(labels.shape) != (features.shape[0], K):
            raise ValueError(f'labels must be (B={features.shape[0]}, {K}), got {tuple(labels.shape)}')
        lo, hi = self._state()
        self._raise_if_flagged()
        eng = model._engine()
        x = features.detach().contiguous().float()
        y = labels.contiguous().float()
        B = x.shape[0]
        w = _elem_weights(model, y)
        if self._buf is None or self._buf['xhat'].shape[0] != B or self._buf['xhat'].device != x.device:
            f32 = dict(device=x.device, dtype=torch.float32)
            self._buf = dict(xhat=torch.empty((B, d), **f32), hrstd=torch.empty(B, **f32), loss_elem=torch.empty((B, K), **f32),
                             dlogits=torch.empty((B, K), **f32), dx=torch.empty((B, d), **f32))
        a = self._buf
        logits = torch.empty((B, K), device=x.device, dtype=torch.float32)
        loss = torch.empty(1, device=x.device, dtype=torch.float32)
        st, ptr = hip.stream(), hip.ptr
        P, G, pre = eng.P32, eng.G32, 'vit.mlp_head.'
        hip.run.ecgvit_head_fwd(ptr(x), 1, ptr(P[pre + '0.weight']), ptr(P[pre + '0.bias']), ptr(P[pre + '1.weight']), ptr(P[pre + '1.bias']),
                                ptr(logits), ptr(a['xhat']), ptr(a['hrstd']), B, d, K, LN_EPS, hip.F32, st)
        hip.run.ecgvit_bce_fwd(ptr(logits), ptr(y), ptr(w), ptr(a['loss_elem']), ptr(loss), B * K, st)
        one = self._const(x.device, 'one', [1.0])
        hip.run.ecgvit_bce_bwd(ptr(logits), ptr(y), ptr(w), ptr(one), None, 1.0 / (B * K), ptr(a['dlogits']), B * K, st)
        hip.run.ecgvit_head_bwd(ptr(a['dlogits']), ptr(a['xhat']), ptr(a['hrstd']), ptr(P[pre + '0.weight']), ptr(P[pre + '0.bias']),
                                ptr(P[pre + '1.weight']), ptr(G[pre + '1.weight']), ptr(G[pre + '1.bias']), ptr(G[pre + '0.weight']),
                                ptr(G[pre + '0.bias']), ptr(a['dx']), 1, B, d, K, hip.F32, st)
        self._keep = (x, y, w)   # alive until the kernels that read them have run
        # (the alignment padding inside the head's range holds zeros and stays zero)
        self._update(model, lo, hi)
        self.last_loss = loss
        return loss, logits


def _elem_weights(model, y):
    """the BCE element weights of labels y under the model's `loss_weight` (None without one)"""
    if not model.loss_weight:
        return None
    return torch.tensor(model.loss_weight, device=y.device, dtype=torch.float32)[y.long()].contiguous()


def _sumsq(g, spans, out, ws):
    """out = the sum of squares of the flat gradient buffer g (or a range of it), or of its spans (device table, rows, elements) only"""
    st = hip.stream()
    if spans is None:
        hip.run.ecgvit_sumsq(g.data_ptr(), g.numel(), out.data_ptr(), ws.data_ptr(), st)
    else:
        hip.run.ecgvit_sumsq_spans(g.data_ptr(), spans[0].data_ptr(), spans[1], spans[2], out.data_ptr(), ws.data_ptr(), st)


def _cuts(B, mb):
    """the record ranges [s, e) of a step's passes: the whole batch, or consecutive slices of mb < B records (the last may be shorter)"""
    if mb is None or mb >= B:
        return [(0, B)]
    return [(s, min(s + mb, B)) for s in range(0, B, mb)]


class _Supervised:
    """`step` to the pass loop.  One pass keeps the loss fused in the forward and hands out copies of the engine's loss and logits.  A split
    step runs every pass's backward with the WHOLE batch's 1/(B*K), gathers the passes' logits and takes the loss in one BCE pass over all
    of them (equal logits -> the unsplit step's loss bit for bit); the labels, the `loss_weight` element weights and the lengths travel with
    their records."""

    def __init__(self, st, model, eng, x, y, lengths, cuts, cls_only):
        self.st, self.eng, self.lengths, self.cuts, self.cls_only, self.split = st, eng, lengths, cuts, cls_only, len(cuts) > 1
        self.x, self.y = x.contiguous().float(), y.contiguous().float()
        self.w = _elem_weights(model, self.y)
        self.B, self.K = self.y.shape[0], eng.K
        if self.split:
            if lengths is not None and eng.input_transform is None and self.x.dim() == 3:
                check_lengths(lengths, self.B, eng.P, self.x.shape[2])   # the whole batch's lengths are valid before the first pass
            self.logits = torch.empty((self.B, self.K), device=self.x.device, dtype=torch.float32)

    def forward(self, j, s, e, seed):
        x, y, w, ls = self.x, self.y, self.w, self.lengths
        if self.split:
            y, w = y[s:e], None if w is None else w[s:e]
            if x.dim() == 2:   # records s .. e - 1: a ragged batch of their own (host offsets, no device read)
                x, ls = ragged_slice(x, ls, s, e)
            elif isinstance(ls, RawPaddedBatch):
                x, ls = x[s:e], ls.records(s, e)
            else:
                x, ls = x[s:e], None if ls is None else ls[s:e]
        logits, _, loss = self.eng.forward(x, y, w, training=True, seed=seed, want_mean=not self.split, cls_only_last=self.cls_only, lengths=ls)
        if self.split:
            self.logits[s:e].copy_(logits)
        else:
            self.loss, self.logits = loss, logits
        one = self.st._const(self.x.device, 'one', [1.0])
        return lambda tpw: self.eng.backward(gscalar=one, gscale=1.0 / (self.B * self.K), tiles_per_workgroup=tpw, trainable=self.st._trainable)

    def result(self):
        if not self.split:
            return self.loss.clone(), self.logits.clone()   # the engine reuses its buffers next step: hand out copies
        st, y, (B, K) = self.st, self.y, self.logits.shape
        if getattr(st, '_bce_elem', None) is None or st._bce_elem.shape != (B, K) or st._bce_elem.device != y.device:
            st._bce_elem = torch.empty((B, K), device=y.device, dtype=torch.float32)
        loss = torch.empty(1, device=y.device, dtype=torch.float32)
        hip.run.ecgvit_bce_fwd(self.logits.data_ptr(), y.data_ptr(), hip.ptr(self.w), st._bce_elem.data_ptr(), loss.data_ptr(), B * K,
                               hip.stream())
        return loss, self.logits


class _Masked:
    """`step_masked` to the pass loop, rectangular (geo None: (B, m) mask indices, staged once and sliced on the device) or over records of
    unequal length (geo: a MaskedVarlenBatch, cut by `records` -- the counts' prefix sums, host offsets only).  One pass hands out copies of
    the engine's loss and reconstruction.  In a split step pass j's L1 mean enters the loss and the upstream gradient with weight B_j / B
    (rectangular) or (its masked patches) / (the batch's), so the sum is the whole batch's mean."""

    def __init__(self, st, wrapper, eng, x, mask_idx, geo, cuts):
        self.st, self.eng, self.geo, self.cuts, self.split = st, eng, geo, cuts, len(cuts) > 1
        self.x = x = x.contiguous().float()
        if geo is None:
            wrapper.check_mask_indices(mask_idx, x.shape[0])
            self.idx = st._device_mask_idx(mask_idx, x.device)
        if self.split:
            self.loss = torch.empty(1, device=x.device, dtype=torch.float32)
            self.one_span = st._const(x.device, 'one span', [[0, 1, 0]], torch.int64)   # the loss: a one-element span
            self.pred, self.k0 = None, 0
            if geo is not None:
                self.parts = [geo.records(s, e) for s, e in cuts]
                self.weights = [g.m / geo.m for _, g in self.parts]
                # the upstream gradients, one copy
                self.up = torch.tensor(self.weights, dtype=torch.float32).pin_memory().to(x.device, non_blocking=True)

    def forward(self, j, s, e, seed):
        st, eng, x, geo = self.st, self.eng, self.x, self.geo
        if geo is None:
            xs, idx = (x[s:e], self.idx[s:e]) if self.split else (x, self.idx)
            pred, mloss = eng.forward_masked(xs, idx, training=True, seed=seed)
        else:
            xs, g = x, geo
            if self.split:
                (s0, s1), g = self.parts[j]
                xs = x[:, s0:s1].contiguous() if x.dim() == 2 else x[s:s + g.B]
            pred, mloss = eng.forward_masked_varlen(xs, g, training=True, seed=seed)
        if not self.split:
            self.loss, self.pred = mloss, pred
            return lambda tpw: eng.backward_masked(tiles_per_workgroup=tpw, trainable=st._trainable)
        if geo is None:
            m, wj = self.idx.shape[1], (e - s) / x.shape[0]
            rows, total, gs = (e - s) * m, x.shape[0] * m, st._const(x.device, ('upstream', wj), [wj])
        else:
            rows, total, wj, gs = g.m, geo.m, self.weights[j], self.up[j:j + 1]
        if self.pred is None:
            self.pred = torch.empty((total,) + tuple(pred.shape[1:]), device=x.device, dtype=pred.dtype)
        self.pred[self.k0:self.k0 + rows].copy_(pred)
        self.k0 += rows
        hip.run.ecgvit_grad_accumulate(self.loss.data_ptr(), mloss.data_ptr(), self.one_span.data_ptr(), 1, 1,
                                       hip.ACC_INIT if j == 0 else hip.ACC_ADD, wj, hip.stream())
        return lambda tpw: eng.backward_masked(gscalar=gs, tiles_per_workgroup=tpw, trainable=st._trainable)

    def result(self):
        if not self.split:
            return self.loss.clone(), self.pred.clone()   # the engine reuses its buffers next step: hand out copies
        return self.loss, self.pred


def span_table(layout, names, flags, lag):
    """rows {element offset, count, step offset} of the flat buffers that a fused step with frozen parameters counts and updates: runs of
    consecutive trainable parameters (in the flat layout's order: embedding, blocks 0..L-1, head, pre-train head) with equal step offsets
    merge into one span (the 64-B alignment padding between them holds zeros and stays zero).  None when every parameter is trainable at
    the global step (the whole-buffer kernels then run, exactly as without frozen parameters)."""
    if all(flags) and not any(lag):
        return None
    lag_of = {n: (f, g) for n, f, g in zip(names, flags, lag)}
    rows, joined = [], False   # joined: the previous parameter in the layout is trainable (its span may grow)
    for n, (off, _, cnt) in layout.entries.items():
        f, g = lag_of[n]
        if f and joined and rows[-1][2] == g:
            rows[-1][1] = off + cnt - rows[-1][0]
        elif f:
            rows.append([off, cnt, g])
        joined = f
    if not rows:
        raise ValueError('no trainable parameter: every parameter has requires_grad=False')
    return rows


def trainable_ranges(layout, buckets, trainable):
    """the gradient exchange's buckets with frozen parameters: per bucket, the element range from its first to its last trainable parameter;
    buckets without one are dropped (never reported by the backward, never exchanged)"""
    trainable = set(trainable)
    out = []
    for tag, (lo, hi) in buckets:
        sel = [(o, o + c) for n, (o, _, c) in layout.entries.items() if n in trainable and lo <= o < hi]
        if sel:
            out.append((tag, (min(a for a, _ in sel), min(hi, (max(b for _, b in sel) + 15) // 16 * 16))))
    return out


def clip_grad_norm_(model, max_norm=1.0, error_if_nonfinite=True):
    """`nn.utils.clip_grad_norm_` for the torch-optimizer interop path, on the model's flat gradient buffer (one
    sum-of-squares pass + one scale pass instead of ~150 per-parameter launches). Requires `p.grad` to be the
    engine's gradient views (true after `loss.backward()` when `zero_grad(set_to_none=True)` preceded it)."""
    l = hip.lib()
    g = model._gflat
    for n, p in zip(model._param_names, model._param_list):  # grads that autograd cloned are copied back into the flat buffer
        if p.grad is not None and p.grad.data_ptr() != g.data_ptr() + 4 * model._layout.entries[n][0]:
            model._layout.view(g, n).copy_(p.grad)
            p.grad = model._layout.view(g, n)
    ws = torch.empty(l.ecgvit_sumsq_workspace(g.numel()), device=g.device, dtype=torch.uint8)
    sumsq = torch.empty(1, device=g.device, dtype=torch.float32)
    out = torch.empty(2, device=g.device, dtype=torch.float32)
    has = [p.grad is not None for p in model._param_list]
    spans = None
    if not all(has):   # as torch: parameters without a gradient (frozen ones) are not counted; their part of the buffer is not a gradient
        rows = span_table(model._layout, model._param_names, has, [0] * len(has))
        spans = (torch.tensor(rows, dtype=torch.int64, device=g.device), len(rows), sum(r[1] for r in rows))
    _sumsq(g, spans, sumsq, ws)
    hip.run.ecgvit_clip_scale(g.data_ptr(), g.numel(), sumsq.data_ptr(), float(max_norm), out.data_ptr(), hip.stream())
    norm, finite = out.tolist()
    if error_if_nonfinite and finite == 0.0:
        raise RuntimeError('The total norm for gradients is non-finite, so it cannot be clipped.')
    return out[0]
