"""
Host-side schedule of the ECG-ViT step over the C-ABI kernels (`include/ecgvit_hip.h`).

This file holds NO arithmetic: it owns the HBM layout (flat f32 parameter / gradient / optimiser buffers,
a bf16 shadow of the weights, per-layer activation slabs kept resident for the backward pass -- 288 GB of
HBM3E makes recomputation pointless at these sizes) and issues the kernels in order on the current HIP
stream.  What each launch replaces in the reference is cited at the call site
(vit-pytorch 0.33.2 `ViT.forward` reached from `ecg_transformer/models/ecg_vit.py:141`).
"""
import math
from collections import OrderedDict

import os

import torch

from . import hip
from .hip import lib, run, ptr, stream, GEMM_NT, GEMM_NN, GEMM_TN
from .hip import EPI_BIAS, EPI_GELU, EPI_GELU_BWD, EPI_RESIDUAL, EPI_DROPOUT, EPI_COLSUM, EPI_GELU_GRAD_AUX, EPI_MUL_AUX

LN_EPS = 1e-5  # nn.LayerNorm default, used by vit_pytorch PreNorm / mlp_head


def _align(n, a=8):
    return (n + a - 1) // a * a


def _numel(shape):
    n = 1
    for v in shape:
        n *= v
    return n


class ParamLayout:
    """name -> (offset, shape) inside one flat f32 buffer; every tensor starts on a 64-B boundary so the same
    offsets address the bf16 shadow on 32-B and the 8-bit shadows on 16-B boundaries (vector loads everywhere)."""

    def __init__(self, named_shapes):
        self.entries = OrderedDict()
        off = 0
        for name, shape in named_shapes:
            n = _numel(shape)
            self.entries[name] = (off, tuple(shape), n)
            off = _align(off + n, 16)
        self.total = off

    def view(self, flat, name):
        off, shape, n = self.entries[name]
        return flat[off:off + n].view(shape)

    def span(self, pred):
        """[lo, hi) element range of the flat buffer covered by the parameters whose name satisfies `pred` (must be contiguous)"""
        sel = [(o, o + c) for n, (o, _, c) in self.entries.items() if pred(n)]
        if not sel:
            return None
        lo, hi = min(a for a, _ in sel), max(b for _, b in sel)
        inside = [n for n, (o, _, c) in self.entries.items() if lo <= o < hi]
        assert all(pred(n) for n in inside), 'bucket is not contiguous in the flat layout'
        return lo, _align(hi, 16)

    def buckets_in_ready_order(self, n_layers):
        """gradient buckets in the order the backward pass completes them: head, layers L-1..0, then embedding (+ extras)"""
        out = [('head', self.span(lambda n: n.startswith('vit.mlp_head.')))]
        for i in reversed(range(n_layers)):
            out.append((f'layer{i}', self.span(lambda n, i=i: n.startswith(f'vit.transformer.layers.{i}.'))))
        out.append(('embed', self.span(lambda n: n in ('vit.pos_embedding', 'vit.cls_token') or n.startswith('vit.to_patch_embedding.'))))
        ex = self.span(lambda n: n.startswith('pretrain.'))
        if ex:
            out.append(('pretrain', ex))
        return [(k, v) for k, v in out if v]


class BackwardPlan:
    """Which parts of a backward pass run when only some parameters are trainable (frozen: `requires_grad=False`).

    The backward is a chain of input-gradient stages: 0 = the objective's head (classification head backward | reconstruction product and
    row scatter), then per block i from the top, at base = 1 + 7 (Ly-1-i): +0 FFN-down input gradient, +1 FFN-up input gradient, +2 LayerNorm-2
    backward, +3 out-projection input gradient, +4 attention backward, +5 QKV input gradient, +6 LayerNorm-1 backward; last, 1 + 7 Ly = the
    embedding backward.  A parameter's gradient needs every stage up to `need(name)`; the pass runs stages 0..`depth` (the deepest need of a
    trainable parameter) and stops there.
      wgrad  -- the Linear weights whose weight-gradient product runs (the trainable ones)
      live   -- the gradient buckets (`ParamLayout.buckets_in_ready_order` tags) holding a trainable parameter: the only ones reported ready
    A plan with `depth` = the embedding stage and every Linear weight trainable is the full pass."""

    def __init__(self, names, n_layers, trainable, masked=False):
        trainable = set(trainable)
        unknown = trainable - set(names)
        if unknown:
            raise ValueError(f'unknown parameter names: {sorted(unknown)}')
        if not trainable:
            raise ValueError('no trainable parameter: every parameter has requires_grad=False')
        self.n_layers, self.masked = n_layers, masked
        self.trainable = frozenset(trainable)
        self.embed_stage = 1 + 7 * n_layers
        self.depth = max(self.need(n) for n in trainable)
        self.wgrad = frozenset(n for n in trainable if n.endswith('.weight') and self._is_linear(n))
        self.live = frozenset(self.bucket(n) for n in trainable)

    @staticmethod
    def _is_linear(name):
        return name.startswith('vit.transformer.layers.') and '.fn.' in name or name in (
            'vit.to_patch_embedding.1.weight', 'pretrain.to_pixels.weight')

    @staticmethod
    def bucket(name):
        if name.startswith('vit.mlp_head.'):
            return 'head'
        if name.startswith('vit.transformer.layers.'):
            return 'layer' + name.split('.')[3]
        if name.startswith('pretrain.'):
            return 'pretrain'
        return 'embed'

    def need(self, name):
        """the last stage the gradient of `name` depends on (-1: none -- written before stage 0, or zero for this objective)"""
        if name.startswith('vit.mlp_head.'):
            return -1 if self.masked else 0
        if name == 'vit.cls_token':
            return -1 if self.masked else self.embed_stage
        if name.startswith('pretrain.'):
            return self.embed_stage if (self.masked and name == 'pretrain.mask_token') else -1
        if not name.startswith('vit.transformer.layers.'):
            return self.embed_stage   # position embedding, patch embedding
        parts = name.split('.')
        base = 1 + 7 * (self.n_layers - 1 - int(parts[3]))
        rest = '.'.join(parts[4:])
        return base + {'1.fn.net.3.weight': -1, '1.fn.net.3.bias': -1, '1.fn.net.0.weight': 0, '1.fn.net.0.bias': 0, '1.norm.weight': 2,
                       '1.norm.bias': 2, '0.fn.to_out.0.bias': 2, '0.fn.to_out.0.weight': 2, '0.fn.to_qkv.weight': 4, '0.norm.weight': 6,
                       '0.norm.bias': 6}[rest]

    def reach(self, stage):
        return stage <= self.depth


def _stage(t, device):
    """a small host tensor -> `device` through pinned memory (a pageable copy would block the host until the stream has drained)"""
    if torch.device(device).type != 'cuda':
        return t
    return t.pin_memory().to(device, non_blocking=True)


def _host_ints(t, what, shape_note):
    if not isinstance(t, torch.Tensor):
        raise ValueError(f'{what} must be {shape_note}, got {type(t).__name__}')
    if t.dtype.is_floating_point or t.dtype.is_complex or t.dtype == torch.bool:
        raise ValueError(f'{what} must be an integer tensor, got {t.dtype}')
    return t.detach().to('cpu', torch.int64)   # (a blocking read for a device tensor)


def _check_lengths(lengths, *, needed=False, B=None, allow_empty=False, width=None, max_len=None, pad=None, P=None, S=None):
    """The one validator of per-record sample counts (`check_lengths`, `check_ragged`, `check_masked_lengths`, `check_raw_lengths`) -> their
    int64 host copy (the one blocking read of a device tensor); anything else raises ValueError.  One fixed order, each check on when its
    keyword is given: present (needed), a tensor, integer dtype, 1-D with B >= 1 entries (B: exactly B; allow_empty: B = 0 passes), positive,
    <= width, <= max_len (pad = k: RAW counts, held to max_len after TimeEndPad to the next multiple of k), multiples of P, summing to S."""
    if needed and lengths is None:
        raise ValueError('a ragged (C, S) batch needs lengths: the (B,) per-record sample counts')
    t = _host_ints(lengths, 'lengths', 'a (B,) integer tensor')
    if t.dim() != 1 or (B is not None and t.shape[0] != B) or (t.shape[0] < 1 and not allow_empty):
        raise ValueError(f'lengths must have shape (batch={"B" if B is None else B},){"" if allow_empty else " with B >= 1"}, got {tuple(lengths.shape)}')
    if t.shape[0] == 0:
        return t
    lo, hi = int(t.min()), int(t.max())
    if lo <= 0:
        raise ValueError(f'lengths must be positive (got {lo})')
    if width is not None and hi > width:
        raise ValueError(f'lengths must not exceed the batch width {width} (got {hi})')
    if max_len is not None and pad is None and hi > max_len:
        raise ValueError(f'lengths must not exceed max_signal_length={max_len} (got {hi})')
    if max_len is not None and pad is not None and hi + (pad - hi % pad) > max_len:
        raise ValueError(f'padded record lengths must not exceed max_signal_length={max_len}: a raw record of {hi} samples pads to '
                         f'{hi + (pad - hi % pad)} (TimeEndPad adds a full patch to a multiple of patch_size={pad})')
    if P is not None and bool((t % P != 0).any()):
        raise ValueError(f'lengths must be multiples of patch_size={P}')
    if S is not None and int(t.sum()) != S:
        raise ValueError(f'lengths must sum to the ragged batch width S={S} (got {int(t.sum())})')
    return t


def check_lengths(lengths, B, P, width):
    """Per-record sample counts of a (B, C, width) batch -> int32 token counts n_tok = lengths / P + 1 on the lengths' own device, or None when
    every record fills the width (the uniform kernels then run).  Each entry must be a positive multiple of P and at most `width`, else
    ValueError.  The values are checked on the host (one blocking read for a device tensor)."""
    t = _check_lengths(lengths, B=B, allow_empty=True, width=width, P=P)
    if B == 0 or int(t.min()) == width:
        return None
    return _stage((t // P + 1).to(torch.int32), lengths.device)


def check_raw_lengths(lengths, xf, max_len, B=None, width=None, S=None):
    """RAW per-record sample counts under a per-record input transform (`FusedInputTransform(per_record=True)`) -> (raw, padded) int64 host
    tensors, padded[b] = xf.padded_length(raw[b]) (a full extra patch when raw[b] is a multiple of the patch).  lengths: a (B,) integer
    tensor, every entry >= 1 (no multiple-of-P rule), at most `width` (a padded (B, C, width) batch) / summing to S (a ragged (C, S) batch),
    and every padded length at most max_len; anything else raises ValueError.  Host work only (one blocking read for a device tensor)."""
    t = _check_lengths(lengths, needed=True, B=B, width=width, max_len=max_len, pad=xf.k, S=S)
    return t, t + (xf.k - t % xf.k)   # FusedInputTransform.padded_length, elementwise


class RawSide:
    """The raw side of a batch under a per-record input transform: what `ecgvit_patch_gather_transform_varlen` reads.
      raw, padded -- int64 [B] on the host: raw sample counts l_b and padded lengths n_b P
      src_off (int64), raw_len, n_patch, row_off (int32) -- [B] on `device`, staged through pinned memory in one copy: first sample of
               record b's lead 0, l_b, n_b, first patch row of record b
      lead_stride -- samples between the leads of one record (W of a padded batch, S_raw of a ragged one)
      nrows -- patch rows per record of the padded row layout (rows past n_b are written as zeros), 0 = packed rows;  n_max = max n_b"""

    def __init__(self, raw, padded, P, src_off, row_off, lead_stride, nrows, device):
        B = raw.shape[0]
        n = padded // P
        pack = torch.cat([src_off.to(torch.int64).contiguous().view(torch.int32), raw.to(torch.int32), n.to(torch.int32), row_off.to(torch.int32)])
        pack = _stage(pack, device)
        self.raw, self.padded, self.B = raw, padded, B
        self.src_off = pack[:2 * B].view(torch.int64)
        self.raw_len, self.n_patch, self.row_off = pack[2 * B:3 * B], pack[3 * B:4 * B], pack[4 * B:5 * B]
        self.lead_stride, self.nrows, self.n_max = int(lead_stride), int(nrows), int(n.max())
        self.src_off_host, self.row_off_host = src_off, row_off


def _excl_cumsum(t):
    return torch.cumsum(t, 0) - t


class RaggedBatch:
    """Token geometry of a ragged batch: B records concatenated along time, (C, S) with S = sum(lengths) (`check_ragged`).
      n_tok   -- int32 [B]: tokens of record b, lengths[b] / P + 1 (its CLS row included)
      tok_off -- int32 [B]: first packed token row of record b, off_b / P + b (off_b = exclusive prefix sum of lengths): its CLS row
      M       -- packed token rows, S / P + B;  N -- the widest record's tokens;  S -- samples
      lengths -- the validated sample counts, int64 on the host: slicing by record range (`records`) reads nothing from the device
    Under a per-record input transform (`raw`: the raw sample counts, `check_raw_lengths`) lengths are the PADDED lengths, the batch itself
    is (C, S_raw) with S_raw = sum(raw), and `rawside` (`RawSide`) says where each record's samples lie; S_raw = S otherwise."""

    def __init__(self, lengths, P, device, raw=None):
        t = lengths
        n_tok = t // P + 1
        tok_off = _excl_cumsum(n_tok)   # = off_b / P + b
        pack = _stage(torch.stack([n_tok, tok_off]).to(torch.int32), device)
        self.lengths, self.P, self.device = t, P, device
        self.n_tok, self.tok_off = pack[0], pack[1]
        self.S = int(t.sum())
        self.M, self.N = self.S // P + t.shape[0], int(t.max()) // P + 1
        self.raw, self.rawside, self.S_raw = raw, None, self.S
        if raw is not None:
            self.S_raw = int(raw.sum())
            # patch rows carry no CLS row: record b's first is tok_off[b] - b = (padded offset of b) / P
            self.rawside = RawSide(raw, t, P, _excl_cumsum(raw), _excl_cumsum(n_tok - 1), self.S_raw, 0, device)

    @property
    def B(self):
        return self.lengths.shape[0]

    def records(self, b0, b1):
        """records b0 .. b1 - 1: (s0, s1) = their sample range in the (C, S) batch (RAW offsets under a per-record transform), and their
        RaggedBatch"""
        src = self.lengths if self.raw is None else self.raw
        s0, s1 = int(src[:b0].sum()), int(src[:b1].sum())
        return (s0, s1), RaggedBatch(self.lengths[b0:b1], self.P, self.device, None if self.raw is None else self.raw[b0:b1])


class RawPaddedBatch:
    """Geometry of a padded (B, C, W) batch of RAW records under a per-record input transform (`VitEngine.check_raw_input`): record b holds
    raw[b] <= W samples, counts n_b = padded[b] / P patches, and the pass runs at `width` = max padded length (N' = width / P + 1 tokens).
      ntok -- int32 [B] on `device`, n_b + 1, or None when every record fills the width (the uniform kernels then run, as `check_lengths`)
      rawside -- `RawSide`: src_off[b] = b C W, row_off[b] = b width / P, width / P patch rows per record (zeros past n_b)
    A slice by record range (`records`: micro-batches, the evaluator) keeps the whole batch's width."""

    def __init__(self, raw, padded, P, C, W, device, width=None):
        B = raw.shape[0]
        self.raw, self.padded, self.P, self.C, self.W, self.device = raw, padded, P, C, W, device
        self.width = int(padded.max()) if width is None else width
        n = self.width // P
        self.ntok = None if int(padded.min()) == self.width else _stage((padded // P + 1).to(torch.int32), device)
        ar = torch.arange(B, dtype=torch.int64)
        self.rawside = RawSide(raw, padded, P, ar * (C * W), ar * n, W, n, device)

    @property
    def B(self):
        return self.raw.shape[0]

    def records(self, b0, b1):
        """records b0 .. b1 - 1 (x[b0:b1] of the batch) at the same pass width"""
        return RawPaddedBatch(self.raw[b0:b1], self.padded[b0:b1], self.P, self.C, self.W, self.device, self.width)


def check_ragged(lengths, S, P, max_len, device=None):
    """Per-record sample counts of a ragged (C, S) batch -> RaggedBatch with n_tok / tok_off as int32 tensors on `device` (default: the
    lengths' own device).  lengths is required, a (B,) integer tensor whose entries are positive multiples of P, at most `max_len`, and sum to
    S; anything else raises ValueError.  The values are read on the host once (a blocking read for a device tensor, as `check_lengths`)."""
    t = _check_lengths(lengths, needed=True, max_len=max_len, P=P, S=S)
    return RaggedBatch(t, P, lengths.device if device is None else torch.device(device))


def ragged_slice(x, lengths, b0, b1):
    """records b0 .. b1 - 1 of a ragged (C, S) batch as a ragged batch of their own: (x[:, off_b0 : off_b1] contiguous, their lengths).
    How micro-batches and the evaluator cut a ragged batch by record range.  lengths: a validated RaggedBatch (nothing is read from the
    device; the slice is a RaggedBatch) or a (B,) tensor (one host read; the slice is lengths[b0:b1])."""
    if isinstance(lengths, RaggedBatch):
        (s0, s1), rg = lengths.records(b0, b1)
        return x[:, s0:s1].contiguous(), rg
    if not isinstance(lengths, torch.Tensor):
        raise ValueError('a ragged (C, S) batch needs lengths: the (B,) per-record sample counts')
    t = lengths.detach().to('cpu', torch.int64)
    s0, s1 = int(t[:b0].sum()), int(t[:b1].sum())
    return x[:, s0:s1].contiguous(), lengths[b0:b1]


class MaskedVarlenBatch:
    """Token geometry of a masked pass over B records of unequal length -- no CLS row: record b holds n_b = lengths[b] / P patch tokens.
      width None -- packed rows (a ragged (C, S) batch): tok_off = exclusive prefix sum of n_b, M = S / P
      width L'   -- padded rows (a (B, C, L') batch with lengths): tok_off[b] = b n_pad, n_pad = L' / P, M = B n_pad
      n_tok, tok_off, order, n_cls -- int32 [B] on `device`, staged through pinned memory in one copy: order = the records by falling n_b
               (ties by record index; `ecgvit_mask_embed_varlen_bwd`), n_cls = n_b + 1 (what `ecgvit_patch_gather_varlen` takes)
      N -- the widest record's patches;  S -- valid samples;  lengths -- the validated sample counts, int64 on the host
      counts, m -- the records' mask counts (int64, host) and their sum;  rows -- int32 [m] on `device`: the masked rows tok_off[b] + idx
    Everything is computed on the host from host data: a step fed host tensors reads nothing back from the device.
    Under a per-record input transform (`raw` = (raw sample counts, lead stride, record stride | None): `check_raw_lengths`) lengths are the
    PADDED lengths and `rawside` (`RawSide`) says where each record's raw samples lie: in a ragged (C, S_raw) batch at the raw offsets
    (record stride None), in a padded (B, C, W) batch at b C W (lead stride W, record stride C W; width = the widest padded length)."""

    def __init__(self, lengths, P, device, width=None, raw=None):
        t = lengths
        B = t.shape[0]
        n = t // P
        self.n_pad = 0 if width is None else width // P
        tok_off = _excl_cumsum(n) if width is None else torch.arange(B, dtype=torch.int64) * self.n_pad
        order = torch.sort(n, descending=True, stable=True).indices
        self.lengths, self.P, self.device, self.width = t, P, device, width
        self.n_host, self.off_host = n, tok_off
        self.S, self.N = int(t.sum()), int(n.max())
        self.M = int(n.sum()) if width is None else B * self.n_pad
        pack = _stage(torch.stack([n, tok_off, order, n + 1]).to(torch.int32), device)
        self.n_tok, self.tok_off, self.order, self.n_cls = pack[0], pack[1], pack[2], pack[3]
        self.counts, self.m, self.rows = None, 0, None
        self.raw, self.rawside = raw, None
        if raw is not None:
            r, lead, rec = raw
            src = _excl_cumsum(r) if rec is None else torch.arange(B, dtype=torch.int64) * rec
            self.rawside = RawSide(r, t, P, src, tok_off, lead, self.n_pad, device)

    @property
    def B(self):
        return self.lengths.shape[0]

    def set_mask(self, idx, counts):
        """idx: validated record-local indices (int64, host, flat), counts (B,) int64 host (`check_mask_varlen`) -> the masked rows"""
        self.counts, self.m = counts, int(idx.numel())
        self.idx_host = idx
        self.rows = _stage((torch.repeat_interleave(self.off_host, counts) + idx).to(torch.int32), self.device)
        return self

    def as_rectangular(self, max_len):
        """the mask as (B, m) int32 host indices when this batch is one the rectangular pass runs -- padded rows, every record max_len samples,
        one mask count -- else None"""
        if self.raw is not None:   # raw records: only the per-record gather reads them
            return None
        if self.width != max_len or int(self.lengths.min()) != max_len or int(self.counts.min()) != int(self.counts.max()):
            return None
        return self.idx_host.view(self.B, -1).to(torch.int32)

    def records(self, b0, b1):
        """records b0 .. b1 - 1 with their mask indices: ((s0, s1) = their sample range in a ragged batch -- RAW offsets under a per-record
        transform --, their MaskedVarlenBatch)"""
        src, raw = self.lengths, None
        if self.raw is not None:
            src = self.raw[0]
            b = int(src[b0:b1].sum())
            raw = (src[b0:b1], b if self.raw[2] is None else self.raw[1], self.raw[2])   # (a ragged slice: its own S_raw is the lead stride)
        s0, s1 = int(src[:b0].sum()), int(src[:b1].sum())
        g = MaskedVarlenBatch(self.lengths[b0:b1], self.P, self.device, self.width, raw)
        if self.counts is not None:
            k0, k1 = int(self.counts[:b0].sum()), int(self.counts[:b1].sum())
            g.set_mask(self.idx_host[k0:k1], self.counts[b0:b1])
        return (s0, s1), g


def check_masked_lengths(lengths, P, max_len, B=None, width=None, S=None):
    """per-record sample counts of a masked batch -> int64 host tensor: a (B,) integer tensor of positive multiples of P, at most `width` (the
    padded form) / max_len, summing to S (the ragged form); anything else raises ValueError"""
    return _check_lengths(lengths, needed=True, B=B, width=width, max_len=max_len, P=P, S=S)


def check_mask_varlen(mask_idx, mask_counts, n):
    """record-local mask indices of records with n[b] patches (n: int64 host tensor) -> (idx, counts) as int64 host tensors.  mask_idx: 1-D
    integer tensor, record 0's indices first; mask_counts: (B,) integer tensor with 1 <= m_b <= n_b summing to mask_idx.numel(); the indices
    of a record distinct and in [0, n_b).  Anything else raises ValueError before any launch (the gather / scatter kernels index unchecked).
    Host tensors are checked on the host; device tensors cost blocking reads."""
    B = n.shape[0]
    c = _host_ints(mask_counts, 'mask_counts', 'a (B,) integer tensor')
    if c.dim() != 1 or c.shape[0] != B:
        raise ValueError(f'mask_counts must have shape (batch={B},), got {tuple(mask_counts.shape)}')
    if not isinstance(mask_idx, torch.Tensor) or mask_idx.dim() != 1:
        raise ValueError('with lengths, mask_idx must be a 1-D integer tensor of record-local patch indices (record 0\'s first), not (B, m): '
                         f'got {tuple(getattr(mask_idx, "shape", ()))}')
    i = _host_ints(mask_idx, 'mask_idx', 'a 1-D integer tensor')
    if int(c.min()) < 1 or bool((c > n).any()):
        raise ValueError('mask_counts must satisfy 1 <= m_b <= n_b (the patches of record b)')
    if int(c.sum()) != i.numel():
        raise ValueError(f'mask_counts must sum to mask_idx.numel()={i.numel()} (got {int(c.sum())})')
    rec = torch.repeat_interleave(torch.arange(B, dtype=torch.int64), c)
    if int(i.min()) < 0 or bool((i >= n[rec]).any()):
        raise ValueError('mask_idx entries must lie in [0, n_b) of their record')
    key = torch.sort(rec * (int(n.max()) + 1) + i).values
    if bool((key[1:] == key[:-1]).any()):
        raise ValueError('mask_idx holds a duplicate patch index inside a record')
    return i, c


def check_masked_varlen_input(x, mask_idx, lengths, mask_counts, *, C, P, max_len, dtype, fp8, input_transform):
    """validate a masked batch of records of unequal length before anything launches -> MaskedVarlenBatch with its mask set, or None for
    the rectangular call ((B, C, L) without lengths / mask_counts: `forward_masked`).  Host work only: needs no device.  x: (B, C, L') with lengths (the padded form) or
    a ragged (C, S) batch (bf16 engine); mask_idx / mask_counts: `check_mask_varlen`.  lengths may already be the MaskedVarlenBatch."""
    if isinstance(lengths, MaskedVarlenBatch):
        return lengths
    ragged = isinstance(x, torch.Tensor) and x.dim() == 2
    if lengths is None and mask_counts is None and not ragged:
        return None
    what = 'ragged batches' if ragged else 'per-record lengths'
    per_record = input_transform is not None and input_transform.per_record
    if input_transform is not None and not per_record:
        raise ValueError(f'{what} are not supported with a fused input transform (its TimeEndPad pads every record) '
                         f'unless it is built with per_record=True')
    if fp8:
        raise ValueError(f'{what} are not supported with fp8_linear')
    if ragged and dtype != torch.bfloat16:
        raise ValueError('ragged batches need the bf16 engine (the f32 parity path materialises padded (B, h, N, N) scores)')
    if not isinstance(x, torch.Tensor) or x.dim() not in (2, 3) or x.shape[-2] != C:
        raise ValueError(f'a masked batch is (B, {C}, L) or a ragged ({C}, S) tensor, got {tuple(getattr(x, "shape", ()))}')
    if lengths is None:
        if ragged:
            raise ValueError('a ragged (C, S) batch needs lengths: the (B,) per-record sample counts')
        raise ValueError('mask_counts needs lengths: the masked objective takes (B, m) mask_idx alone, or lengths with flat mask_idx and mask_counts')
    if mask_counts is None:
        raise ValueError('lengths needs mask_counts: with per-record lengths mask_idx is flat (record-local indices, record 0\'s first) and '
                         'mask_counts (B,) says how many belong to each record')
    if per_record:   # lengths are RAW sample counts; the token geometry is that of the padded lengths
        if ragged:
            raw, t = check_raw_lengths(lengths, input_transform, max_len, S=x.shape[1])
            width, rawinfo = None, (raw, x.shape[1], None)
        else:
            raw, t = check_raw_lengths(lengths, input_transform, max_len, B=x.shape[0], width=x.shape[2])
            width, rawinfo = int(t.max()), (raw, x.shape[2], C * x.shape[2])
        idx, counts = check_mask_varlen(mask_idx, mask_counts, t // P)
        return MaskedVarlenBatch(t, P, x.device, width, rawinfo).set_mask(idx, counts)
    if ragged:
        t = check_masked_lengths(lengths, P, max_len, S=x.shape[1])
        width = None
    else:
        width = x.shape[2]
        if not 0 < width <= max_len or width % P:
            raise ValueError(f'a batch of {width} samples per record: must be a positive multiple of patch_size={P} '
                             f'and at most max_signal_length={max_len}')
        t = check_masked_lengths(lengths, P, max_len, B=x.shape[0], width=width)
    idx, counts = check_mask_varlen(mask_idx, mask_counts, t // P)
    return MaskedVarlenBatch(t, P, x.device, width).set_mask(idx, counts)


class VitEngine:
    """Forward / backward of EcgVit for one activation dtype (torch.float32 = parity path, torch.bfloat16 =
    throughput path). Caller provides the flat buffers; all activations are allocated here, once per batch size."""

    def __init__(self, *, C, L, P, d, h, f, Ly, K, p_hidden, p_emb, dtype, layout: ParamLayout, fp8_linear=False, saved_ffn_e4m3=None):
        assert L % P == 0, 'Image dimensions must be divisible by the patch size.'  # vit_pytorch's own assertion text
        self.C, self.L, self.P, self.d, self.h, self.f, self.Ly, self.K = C, L, P, d, h, f, Ly, K
        self.n = L // P
        self.N = self.n + 1
        # the configured record length is the maximum: a pass over a narrower batch (L' <= L, L' % P == 0) runs at N' = L'/P + 1 tokens
        # (`_set_width`); L / n / N below always describe the current pass
        self.L_max, self.n_max, self.N_max = self.L, self.n, self.N
        self.dh = d // h
        self.CP = C * P
        self.p_hidden, self.p_emb = float(p_hidden), float(p_emb)
        self.dtype = dtype
        self.layout = layout
        self.scale = self.dh ** -0.5
        if d % 8 or f % 8 or self.CP % 8 or self.dh % 8:
            raise ValueError(f'HIP path needs hidden_size, intermediate_size, head dim and C*P to be multiples of 8 '
                             f'(got d={d}, f={f}, dh={self.dh}, C*P={self.CP})')
        if d > hip.ROW_MAX_D:
            raise ValueError(f'HIP LayerNorm kernels cover hidden_size <= {hip.ROW_MAX_D}')
        if h == 1:
            raise NotImplementedError('heads == 1 (vit_pytorch drops to_out) is not covered by the HIP path')
        if dtype == torch.bfloat16:
            if self.dh not in (64, 128):
                raise ValueError(f'bf16 fused attention needs head dim 64 or 128 (got {self.dh}); use dtype=torch.float32')
            if self.N > hip.ATTN_MAX_N:
                raise ValueError(f'bf16 fused attention covers <= {hip.ATTN_MAX_N} tokens (got {self.N}); use dtype=torch.float32')
            for nm, pv in (('hidden_dropout_prob', self.p_hidden), ('attention_probs_dropout_prob (the embedding dropout: reference ecg_vit.py:113)', self.p_emb)):
                if 0.0 < pv < 1.0 / 512:
                    # every dropout site of the bf16 path draws 8 random bits per element: p is applied as round(256 p) / 256 (0.1 -> 0.1016)
                    raise ValueError(f'the bf16 path applies dropout in steps of 1/256: {nm}={pv} would round to no dropout; use 0, a value '
                                     f'>= 1/512, or compute_dtype=torch.float32 (exact p)')
        # fp8 Linear operands (BASELINE.json configs[4]): every product of the four block Linears takes 8-bit operands -- forward e4m3 x e4m3,
        # input gradients e5m2 gradients x e4m3 weights, weight gradients e5m2 gradients x e4m3 activations with f32 split-K accumulation
        # (per-tensor scales, delayed for activations and gradients); attention, LayerNorm and the optimiser stay bf16 / f32
        self.fp8 = bool(fp8_linear)
        if self.fp8:
            if dtype != torch.bfloat16:
                raise ValueError('fp8_linear needs the bf16 engine (compute_dtype=torch.bfloat16)')
            if d % 128 or f % 128:
                raise ValueError(f'fp8_linear needs hidden_size and intermediate_size to be multiples of 128 (got d={d}, f={f})')
        # fp8_linear, steady state: four bf16 tensors per layer have 8-bit readers ONLY once their producers emit the 8-bit copies -- the
        # LayerNorm outputs xn1 / xn2 (QKV / FFN-up product + their weight gradients), the FFN-up output hact (FFN-down product + weight
        # gradient), the FFN-down input gradient dh (FFN-up input + weight gradient) and the dropout-masked gradient dxm of the fused LayerNorm
        # backward.  They are then not written at all (ECGVIT_EPI_NO_OUT / NULL y / NULL dxm): ~2.9 GB of stores less per EcgVit-large layer at
        # 256 x 501 tokens.  Needs every reader on its 8-bit kernel: the weight-gradient kernel wants d, f % 256 == 0 and >= 4096 rows.
        # (False: keep writing them -- tests hold the two modes against each other bit for bit.)
        self.fp8_drop_dead_bf16 = self.fp8 and d % 256 == 0 and f % 256 == 0
        # the saved FFN tensor gelu'(pre) x dropout multiplier as e4m3 bytes (ECGVIT_EPI_AUX8; bf16 or 8-bit operands, large A.B^T kernel): private to the
        # FFN-up forward and the FFN-down input gradient, 790 MB per layer at base whose HBM stream costs each launch ~85 us.  False: bf16.
        # `saved_ffn_e4m3` (EcgVit(..., saved_ffn_e4m3=)): None = on for the bf16 engine; False = keep the tensor in bf16
        if saved_ffn_e4m3 and dtype != torch.bfloat16:
            raise ValueError('saved_ffn_e4m3 needs the bf16 engine (the f32 parity path keeps the f32 pre-activation)')
        self.aux8 = dtype == torch.bfloat16 if saved_ffn_e4m3 is None else bool(saved_ffn_e4m3)
        self.B = None
        self._alloc_key = None
        self._pool, self._pool_B = None, 0
        self.T = self.N
        self.act = None
        self.P32 = self.G32 = self.W = None
        self._ws = {}
        self.saved = None
        self.input_transform = None  # FusedInputTransform: forward() then takes RAW (B, C, L_raw) records
        self.on_grads_ready = None   # callback(tag): a gradient bucket ('head' | 'layer{i}' | 'embed' | 'pretrain') is final
        self._tpw = 0                # ecgvit_gemm_desc.tiles_per_workgroup of the launches in flight (set by backward(..., tiles_per_workgroup=))

    def _set_width(self, width):
        """token geometry of the next pass: `width` samples per record (<= the configured max_signal_length, a multiple of P)"""
        if width == self.L:
            return
        if not 0 < width <= self.L_max or width % self.P:
            raise ValueError(f'a batch of {width} samples per record: must be a positive multiple of patch_size={self.P} '
                             f'and at most max_signal_length={self.L_max}')
        self.L, self.n = width, width // self.P
        self.N = self.n + 1

    def _gemm(self, *a, **kw):
        """every product of this engine: `tiles_per_workgroup` is per-engine, per-pass state (never a process-wide setting)"""
        kw.setdefault('tiles_per_workgroup', self._tpw)
        hip.gemm(*a, **kw)

    # ---------------------------------------------------------------- buffers
    def bind(self, pflat, gflat, wlow=None, wlow_t=None):
        """pflat/gflat: flat f32 params / grads. wlow: flat bf16 shadow of pflat (bf16 engine only); wlow_t: same layout, the trunk's
        Linear weights stored TRANSPOSED (see `transposed_weight_table`), so their input-gradient products run as A . B^T."""
        lay = self.layout
        self.P32 = {k: lay.view(pflat, k) for k in lay.entries}
        self.G32 = {k: lay.view(gflat, k) for k in lay.entries}
        self.WT = {}
        if self.dtype == torch.bfloat16:
            assert wlow is not None and wlow.dtype == torch.bfloat16
            self.W = {k: lay.view(wlow, k) for k in lay.entries}
            if wlow_t is not None:
                for k in self.transposed_weight_names():
                    off, shape = lay.entries[k][0], lay.entries[k][1]
                    self.WT[k] = wlow_t[off:off + shape[0] * shape[1]].view(shape[1], shape[0])
        else:
            self.W = self.P32
        self.device = pflat.device
        if self.fp8:
            assert wlow_t is not None, 'fp8_linear runs the input gradients against the transposed weight shadows'
            names = self.transposed_weight_names()
            assert len(names) == 4 * self.Ly, 'fp8_linear: every block Linear must be large enough for the 256^2 kernel'
            self._wlow, self._wlow_t = wlow, wlow_t
            self.w8 = torch.zeros(lay.total, dtype=torch.uint8, device=self.device)
            self.w8t = torch.zeros(lay.total, dtype=torch.uint8, device=self.device)
            self.w8_index = {k: i for i, k in enumerate(names)}
            self.w8_table = torch.tensor([[lay.entries[k][0], lay.entries[k][2]] for k in names], dtype=torch.int64, device=self.device)
            self.w8_count = max(lay.entries[k][2] for k in names)
            self.w8_scale = torch.zeros(len(names), dtype=torch.float32, device=self.device)
            self.w8_amax = torch.zeros(len(names), dtype=torch.float32, device=self.device)
            self.W8, self.WT8 = {}, {}
            for k in names:
                off, (r, c), n = lay.entries[k]
                self.W8[k] = self.w8[off:off + n].view(r, c)
                self.WT8[k] = self.w8t[off:off + n].view(c, r)
            # activation / gradient sites, 8 per layer: e4m3 xn1, attn, xn2, hact ; e5m2 dY(ffn-down), dh, dY(out), dqkv
            ns = 8 * self.Ly
            self.f8_scale = torch.zeros(ns, dtype=torch.float32, device=self.device)
            self.f8_amax = torch.zeros(ns, dtype=torch.float32, device=self.device)
            self.f8_fmt = torch.tensor(([hip.FP8_E4M3] * 4 + [hip.BF8_E5M2] * 4) * self.Ly, dtype=torch.int32, device=self.device)
            self._f8_seen = set()
            self._f8_last_training, self._f8_scale_train = None, None

    # ---------------------------------------------------------------- fp8 operand path
    def refresh_fp8_weights(self, only=None):
        """e4m3 shadows of the block Linears' weights and of their transposes, one scale per matrix from its current amax: three
        launches over the flat bf16 shadows (call after the optimiser rewrote them).  only: the names that changed (None = all): the
        launches then cover each run of consecutive rows of the matrix table that holds only changed matrices"""
        st = stream()
        nm = len(self.w8_index)
        runs = [(0, nm)]
        if only is not None:
            runs, r0 = [], None
            for k, i in list(self.w8_index.items()) + [(None, nm)]:
                if k is not None and k in only:
                    r0 = i if r0 is None else r0
                elif r0 is not None:
                    runs.append((r0, i))
                    r0 = None
        for r0, r1 in runs:
            tab, sc, am = self.w8_table[r0:r1], self.w8_scale[r0:r1], self.w8_amax[r0:r1]
            run.ecgvit_fp8_amax(ptr(self._wlow), ptr(tab), r1 - r0, self.w8_count, ptr(am), st)
            run.ecgvit_fp8_scale_update(ptr(sc), ptr(am), r1 - r0, None, hip.FP8_E4M3, st)
            for src, dst in ((self._wlow, self.w8), (self._wlow_t, self.w8t)):
                run.ecgvit_fp8_quantize(ptr(src), ptr(dst), ptr(tab), r1 - r0, self.w8_count, hip.FP8_E4M3, ptr(sc), None, st)

    def fp8_begin_step(self, training=True):
        """delayed scaling: the scales of this pass come from the amax the previous pass's quantise kernels accumulated.
        One exception: a TRAINING pass that follows EVAL passes resumes from the scales the last training pass left (snapshotted when the first eval
        pass began; the eval passes' amax is discarded) -- eval activations carry no dropout, training tensors are rescaled by 1 / (1 - p) (the FFN
        hidden activation most of all), and scales are amax / format-max with no headroom: scales taken from an eval pass would saturate the
        first training step after every evaluation."""
        if self._f8_seen:
            if training and self._f8_last_training is False and self._f8_scale_train is not None:
                # (only where the snapshot holds a scale: a site first reached after it -- e.g. a gradient site of a block that was frozen
                # until then -- keeps its own instead of taking scale 0, which would quantise it to zeros)
                self.f8_scale.copy_(torch.where(self._f8_scale_train > 0, self._f8_scale_train, self.f8_scale))
                self.f8_amax.zero_()
            else:
                run.ecgvit_fp8_scale_update(ptr(self.f8_scale), ptr(self.f8_amax), self.f8_scale.numel(), ptr(self.f8_fmt), 0, stream())
                if not training and self._f8_last_training:
                    self._f8_scale_train = self.f8_scale.clone()   # train -> eval: what the last training pass's amax gave (8 floats per layer)
        self._f8_last_training = bool(training)

    def _quant(self, site, x, count, out=None):
        """x (bf16, `count` elements) -> `out` (a layer's persistent e4m3 copy: the weight-gradient product reads it again in the
        backward pass) or the shared 8-bit scratch, in the site's format; returns (8-bit view, scale pointer tensor)"""
        st = stream()
        sc, am = self.f8_scale[site:site + 1], self.f8_amax[site:site + 1]
        fmt = hip.FP8_E4M3 if site % 8 < 4 else hip.BF8_E5M2
        if site not in self._f8_seen:   # first use: no history yet -> scale from this tensor's own amax (one extra read)
            run.ecgvit_fp8_amax(ptr(x), None, 1, count, ptr(am), st)
            run.ecgvit_fp8_scale_update(ptr(sc), ptr(am), 1, None, fmt, st)
            self._f8_seen.add(site)
        q = out if out is not None else self.act['q8'][:count]
        run.ecgvit_fp8_quantize(ptr(x), ptr(q), None, 1, count, fmt, ptr(sc), ptr(am), st)
        return q, sc

    def _emit8(self, kw, site, ld, out=None, only8=False):
        """ask an 8-bit product's epilogue to also write the 8-bit copy of its output that the next product (site `site`) consumes --
        possible once that site has a scale (from the second pass on); `out`: where (default: the q8b scratch); only8: the bf16 output has
        no reader then (EPI_NO_OUT); returns True when armed"""
        if site not in self._f8_seen:
            return False
        kw['epilogue'] = kw.get('epilogue', 0) | hip.EPI_QUANT_OUT | (hip.EPI_NO_OUT if only8 else 0)
        kw.update(q8_out=out if out is not None else self.act['q8b'], ldq8=ld, q8_scale=self.f8_scale[site:site + 1], q8_amax=self.f8_amax[site:site + 1],
                  q8_format=hip.FP8_E4M3 if site % 8 < 4 else hip.BF8_E5M2)
        return True

    def _aux8(self, M):
        """the FFN-wide launches over M token rows take the large A.B^T kernel (the mirror of ecgvit_gemm_nt_applicable for [M, f] x K = d), so the
        saved tensor may be e4m3 bytes; the library rejects the flag loudly if this ever disagrees with its own dispatch"""
        return (self.aux8 and bool(self.WT) and M >= 2048 and self.f >= 128 and self.f % 8 == 0 and self.d % 64 == 0 and self.d >= 192
                and (M + 256) * self.f * 2 < 2 ** 31)   # (self.WT: the input gradient runs as A.B^T against the transposed shadow)

    def _only8(self, M):
        """the bf16 copies with 8-bit readers only may be left unwritten in a pass over M token rows (see `fp8_drop_dead_bf16`)"""
        return self.fp8 and self.fp8_drop_dead_bf16 and M >= 4096

    def _bf16_reader(self, M, what):
        """called by every bf16 fallback of a block product: when `_only8(M)` holds, the producers have left xn1 / xn2 / hact / dh / dxm
        UNWRITTEN on the promise that every reader takes its 8-bit kernel -- a reader that falls back to bf16 would consume stale
        buffers from an earlier step and return wrong gradients without any error.  The promise is written out in several places
        (`_only8`, `_wgrad`, `_dgrad`, the library's applicability checks); if they ever drift apart, fail here"""
        if self._only8(M):
            raise RuntimeError(f'fp8_linear: {what} fell back to its bf16 kernel over {M} rows while the bf16 operand copies are not '
                               f'written (fp8_drop_dead_bf16); the 8-bit applicability conditions have drifted apart')

    def _linear(self, site, A, name, C, M, N, K, a8=None, emit_site=None, emit_to=None, prequant=False, emit_only8=False, **kw):
        """C = epilogue(A . W^T) for block Linear `name`: bf16 operands, or (fp8_linear) A quantised to e4m3 against the e4m3 shadow.
        a8: this layer's persistent e4m3 copy of A (written here, or already by A's producer when `prequant`; the weight-gradient
        product of the backward pass reads it again); emit_site / emit_to: the site that consumes C next and its persistent copy
        (then written by this epilogue).  Returns True when the 8-bit copy of C was emitted."""
        if not self.fp8 or M < 2048:    # the 8-bit kernel covers the large products only: small batches run bf16
            self._bf16_reader(M, 'Linear ' + name)
            self._gemm(GEMM_NT, A, self.W[name], C, M, N, K, K, K, N, **kw)
            return False
        if prequant:   # the producer (LayerNorm forward, a GEMM epilogue) already wrote A's 8-bit copy into a8
            q, sc = a8, self.f8_scale[site:site + 1]
        else:
            q, sc = self._quant(site, A, M * K, out=a8)
        emitted = emit_site is not None and self._emit8(kw, emit_site, N, out=emit_to, only8=emit_only8)
        mi = self.w8_index[name]
        self._gemm(GEMM_NT, q, self.W8[name], None if kw.get('epilogue', 0) & hip.EPI_NO_OUT else C, M, N, K, K, K, N, fp8_format=hip.FP8_E4M3,
                   scale_a=sc, scale_b=self.w8_scale[mi:mi + 1], **kw)
        return emitted

    def transposed_weight_names(self):
        """Linear weights of the transformer blocks whose dgrad is large enough for the 256^2 forward kernel (K % 64 == 0, N >= 256)"""
        out = []
        for i in range(self.Ly):
            lp = f'vit.transformer.layers.{i}.'
            for k in ('0.fn.to_qkv.weight', '0.fn.to_out.0.weight', '1.fn.net.0.weight', '1.fn.net.3.weight'):
                rows, cols = self.layout.entries[lp + k][1]
                if rows % 64 == 0 and rows >= 192 and cols >= 256 and cols % 8 == 0:
                    out.append(lp + k)
        return out

    def transposed_weight_table(self, device, only=None):
        """(table tensor int64 [nmat, 4] on `device`, nmat, ntiles) for ecgvit_transpose_bf16_batched; only: a subset of the names"""
        rows_, t = [], 0
        for k in self.transposed_weight_names():
            if only is not None and k not in only:
                continue
            off, (r, c) = self.layout.entries[k][0], self.layout.entries[k][1]
            rows_.append([off, r, c, t])
            t += ((r + 63) // 64) * ((c + 63) // 64)
        if not rows_:
            return None, 0, 0
        return torch.tensor(rows_, dtype=torch.int64, device=device), len(rows_), t

    def _grad8(self, site, dY, count, prequant=False):
        """(e5m2 copy of the gradient dY entering site `site`, its scale) for the site's two backward products -- the input gradient
        dY . W and the weight gradient dY^T . X; prequant: its producer already wrote the copy ('q8': LayerNorm backward into the
        operand scratch, True: a GEMM epilogue into q8b).  None when the 8-bit path does not apply."""
        if prequant:
            return self.act['q8' if prequant == 'q8' else 'q8b'][:count], self.f8_scale[site:site + 1]
        # (not prequant: the producer did not emit the copy and therefore DID write its bf16 output -- `_emit8` / the q8 LayerNorm branch arm
        # "no bf16 output" and "8-bit copy emitted" together, and report it through the return value that became `prequant`)
        return self._quant(site, dY, count)

    def _dgrad(self, dY, name, dX, M, kin, nout, site=None, emit_site=None, pre=None, emit_only8=False, **kw):
        """dX[M, kin] = dY[M, nout] . W[nout, kin]: on the forward kernel against the transposed shadow when there is one.
        pre: (8-bit copy of dY, scale) from `_grad8` (fp8_linear).  Returns True when the 8-bit copy of dX was emitted for `emit_site`
        (emit_only8: and dX itself left unwritten)."""
        if self.fp8 and pre is not None and name in self.w8_index:
            q, sc = pre
            emitted = emit_site is not None and self._emit8(kw, emit_site, kin, only8=emit_only8)
            mi = self.w8_index[name]
            self._gemm(GEMM_NT, q, self.WT8[name], None if kw.get('epilogue', 0) & hip.EPI_NO_OUT else dX, M, kin, nout, nout, nout, kin,
                       fp8_format=hip.BF8_E5M2, scale_a=sc, scale_b=self.w8_scale[mi:mi + 1], **kw)
            return emitted
        if self.fp8:
            self._bf16_reader(M, 'input gradient of ' + name)
        wt = self.WT.get(name)
        if wt is not None and M >= 2048:
            self._gemm(GEMM_NT, dY, wt, dX, M, kin, nout, nout, nout, kin, **kw)
        else:
            self._gemm(GEMM_NN, dY, self.W[name], dX, M, kin, nout, nout, kin, kin, **kw)

    def _alloc(self, B, masked=False, m=0, rows=None, mrows=None):
        """Activation slabs for a pass over B records (rows: the packed token rows of a ragged batch; None = B x tokens per record; mrows: the
        masked rows of a masked pass over records of unequal length, B x m otherwise).  Every slab's leading dimension is proportional to B, so
        ONE pool serves every batch size through prefix views: a loop that alternates train (B = 512) and eval (B = 64) batches, or ends an epoch
        on a short batch, re-slices instead of freeing and re-requesting ~40 GB (base) from the allocator on each switch.  The pool grows PER SLAB
        and never shrinks; slabs are shared by name across objectives and row layouts, so a loop that alternates supervised, masked, padded and
        ragged passes re-slices too (the slabs only one of them names -- the pruned block's, the masked head's -- stay in the pool)."""
        key = (B, masked, m, self._aux8(rows if rows is not None else B * (self.n if masked else self.N)), self.N, rows, mrows)
        if self._alloc_key == key and self.act is not None:
            return
        self._alloc_key = key
        self.T = self.n if masked else self.N   # tokens per record: no CLS row in the masked-pretrain trunk
        spec = self._act_spec(B, masked, m, rows, mrows=mrows)
        # a ragged pass reserves what a padded pass of the same B at max_signal_length takes: steps of equal B and any S then re-slice the
        # same slabs (and never hold more than that padded pass would)
        reserve = self._act_spec(B, masked, m, N=self.n_max if masked else self.N_max, mrows=mrows) if rows is not None else {}
        pool = self._pool if self._pool is not None else {}
        self._pool = pool
        self._pool_B = max(B, self._pool_B)
        # Grow-only and PER SLAB inside a group: a slab is re-requested only when this pass needs more bytes of it than the pool holds (a
        # workspace size need not be monotone in B), and slabs the current spec does not name (the e4m3 operand copies of an fp8 model while a
        # short batch runs on the bf16 kernels) stay in the pool for the pass that wants them again.  A slab whose ELEMENT TYPE depends on the
        # pass -- `hpre`: e4m3 bytes over >= 2048 token rows, the activation type below that -- is pooled as bytes and viewed per pass, so a
        # batch that crosses the boundary (a short epoch remainder) re-slices like any other
        for k, (sh, dt) in spec.items():
            pdt = torch.uint8 if k.endswith('.hpre') else dt
            need = _numel(sh) * (dt.itemsize if pdt != dt else 1)
            if k in reserve:
                rsh, rdt = reserve[k]
                need = max(need, _numel(rsh) * (rdt.itemsize if pdt != rdt else 1))
            have = pool.get(k)
            if have is None or have.dtype != pdt or have.numel() < need:
                if self.act is not None:
                    self.act = None                # views of the slab being replaced die with it
                pool[k] = None                     # (drop the old slab before asking for the new one)
                pool[k] = torch.empty(need, device=self.device, dtype=pdt)
        a, layers = {}, [dict() for _ in range(self.Ly)]
        for k, (sh, dt) in spec.items():
            if pool[k].dtype != dt:                # byte slab viewed in this pass's element type
                v = pool[k][:_numel(sh) * dt.itemsize].view(dt).view(sh)
            else:
                v = pool[k][:_numel(sh)].view(sh)
            if k[0] == 'L' and '.' in k:
                i, kk = k[1:].split('.', 1)
                layers[int(i)][kk] = v
            else:
                a[k] = v
        a['layers'] = layers
        self.act, self.B = a, B

    def _act_spec(self, B, masked, m, rows=None, N=None, mrows=None):
        """name -> (shape, dtype) of every activation / scratch slab of a pass over B records (layer slabs as 'L{i}.{name}'); rows: the packed
        token rows of a ragged batch; N: tokens per record (default: the current pass's); mrows: the masked rows (default B x m)"""
        T = self.dtype
        f32, u8 = torch.float32, torch.uint8
        if N is None:
            N = self.n if masked else self.N
        M, Mp = B * N, B * (N if masked else N - 1)
        if rows is not None:
            M, Mp = rows, rows - (0 if masked else B)   # (no CLS rows in the masked trunk)
        d, f, h = self.d, self.f, self.h
        sp = OrderedDict()
        sp.update(patches=((Mp, self.CP), T), tok=((Mp, d), T), x0=((M, d), T))
        for i in range(self.Ly):
            l = dict(mean1=((M,), f32), rstd1=((M,), f32), xn1=((M, d), T), qkv=((M, 3 * d), T), attn=((M, d), T), x1=((M, d), T),
                     mean2=((M,), f32), rstd2=((M,), f32), xn2=((M, d), T), hpre=((M, f), u8 if self._aux8(M) else T), hact=((M, f), T), x2=((M, d), T))
            if T == torch.float32:
                l['probs'] = ((B * h * N * N,), T)
            else:
                l['lse'] = ((B * h * N,), f32)
            if self.fp8 and M >= 2048:
                # e4m3 copies of the four Linear inputs, kept for the backward pass: the 8-bit weight-gradient products read them again
                # (one byte per element next to the two of the bf16 tensors: +0.9 GB per layer for large at 256 x 501 tokens)
                l.update(xn1_8=((M * d,), u8), attn_8=((M * d,), u8), xn2_8=((M * d,), u8), hact_8=((M * f,), u8))
            for k, v in l.items():
                sp[f'L{i}.{k}'] = v
        sp.update(logits=((B, self.K), f32), xhat=((B, d), f32), hrstd=((B,), f32), loss_elem=((B, self.K), f32), loss_mean=((1,), f32),
                  dlogits=((B, self.K), f32))
        # backward scratch (shared by all layers)
        sp.update(dxa=((M, d), T), dxb=((M, d), T), dxn=((M, d), T), dqkv=((M, 3 * d), T), dattn=((M, d), T), dh=((M, f), T),
                  dtok=((Mp, d), T), dxm=((M, d), T))
        if T == torch.float32:
            sp.update(pd=((B * h * N * N,), T), dp=((B * h * N * N,), T))
        if T == torch.bfloat16 and not masked:
            # the pruned last block (forward(..., cls_only_last=True)): its activations and gradients past K / V, one row per record
            sp.update({f'cls_{k}': ((B, d), T) for k in ('attn', 'x1', 'xn2', 'x2', 'dx', 'dy', 'dxn', 'dx1', 'dxm', 'dattn', 'dq')})
            sp.update(cls_hpre=((B, f), T), cls_hact=((B, f), T), cls_dh=((B, f), T), cls_lse=((B * h,), f32), cls_mean2=((B,), f32),
                      cls_rstd2=((B,), f32))
        l = lib()
        ws = max(l.ecgvit_layernorm_bwd_workspace(M, d), l.ecgvit_colsum_workspace(M, max(f, 3 * d)), 8 * ((M + 255) // 256) * f, 4096)
        if T == torch.bfloat16:
            for (mm, nn) in ((d, f), (f, d), (d, d), (3 * d, d), (d, self.CP)):
                ws = max(ws, hip.gemm_workspace_bytes(GEMM_TN, T, mm, nn, M))
        if masked:
            Rm = B * m if mrows is None else mrows
            sp.update(flag=((Mp,), u8), rows=((Rm, d), T), pred=((Rm, self.CP), T), target=((Rm, self.CP), T),
                      dpred=((Rm, self.CP), T), drows=((Rm, d), T), dmasked=((Mp, d), T), mloss=((1,), f32), l1part=((1024,), f32))
        sp['ws'] = ((ws,), u8)
        if self.fp8:
            sp['q8'] = ((M * max(f, 3 * d),), u8)   # one quantised operand at a time
            sp['q8b'] = ((M * f,), u8)              # 8-bit copies written by a producing epilogue
        return sp

    # ---------------------------------------------------------------- small launch helpers
    @staticmethod
    def _ln_exact(d):
        """d has the exact lane mapping of csrc/rowops.hip (ln_fit): the widths whose bf16 LayerNorm can also emit the 8-bit copies"""
        return d % 256 == 0 and d // 64 in (4, 8, 12, 16, 24, 32)

    def _ln_fwd(self, x, g, b, y, mean, rstd, rows, q8_site=None, y8=None):
        """LayerNorm forward; q8_site (fp8_linear): also write the e4m3 copy of y into the operand scratch for the Linear that consumes
        it (returns True), once that site has a scale and when the exact lane mapping covers d"""
        d = self.d
        if self.fp8 and q8_site is not None and q8_site in self._f8_seen and rows >= 2048 and self._ln_exact(d):
            # (y has 8-bit readers only when it has a persistent 8-bit copy for the weight gradient: see fp8_drop_dead_bf16)
            run.ecgvit_layernorm_fwd_q8(ptr(x), ptr(g), ptr(b), None if (y8 is not None and self._only8(rows)) else ptr(y), ptr(mean), ptr(rstd), rows, d, LN_EPS,
                                        ptr(y8 if y8 is not None else self.act['q8']),
                                        ptr(self.f8_scale[q8_site:q8_site + 1]), ptr(self.f8_amax[q8_site:q8_site + 1]), stream())
            return True
        run.ecgvit_layernorm_fwd(ptr(x), ptr(g), ptr(b), ptr(y), ptr(mean), ptr(rstd), rows, d, LN_EPS,
                                 hip.code(self.dtype), stream())
        return False

    def _ln_bwd(self, dy, x, g, mean, rstd, dres, dx, dg, db, rows):
        run.ecgvit_layernorm_bwd(ptr(dy), ptr(x), ptr(g), ptr(mean), ptr(rstd), ptr(dres), ptr(dx), ptr(dg), ptr(db),
                                 ptr(self.act['ws']), rows, self.d, hip.code(self.dtype), stream())

    def _ln_bwd_fused(self, dy, x, g, mean, rstd, dres, dx, dg, db, rows, dxm, dcolsum, p, seed, q8_site=None):
        """LayerNorm backward that also emits, for the NEXT stage, the dropout-masked copy of dx and its column sums; q8_site
        (fp8_linear): also the e5m2 copy of that gradient into the operand scratch for the input-gradient product that consumes it
        (returns True), once the site has a scale and when the exact lane mapping covers d"""
        d = self.d
        if (self.fp8 and q8_site is not None and q8_site in self._f8_seen and rows >= 2048 and self._ln_exact(d)
                and rows * d < 2 ** 31):
            run.ecgvit_layernorm_bwd_fused_q8(ptr(dy), ptr(x), ptr(g), ptr(mean), ptr(rstd), ptr(dres), ptr(dx), ptr(dg), ptr(db),
                                              ptr(self.act['ws']), rows, d, None if self._only8(rows) else ptr(dxm), ptr(dcolsum), p, seed, ptr(self.act['q8']),
                                              ptr(self.f8_scale[q8_site:q8_site + 1]), ptr(self.f8_amax[q8_site:q8_site + 1]), stream())
            return True
        run.ecgvit_layernorm_bwd_fused(ptr(dy), ptr(x), ptr(g), ptr(mean), ptr(rstd), ptr(dres), ptr(dx), ptr(dg), ptr(db),
                                       ptr(self.act['ws']), rows, self.d, ptr(dxm), ptr(dcolsum), p, seed,
                                       hip.code(self.dtype), stream())
        return False

    def _colsum(self, x, ld, out, M, N):
        run.ecgvit_colsum(ptr(x), ld, ptr(out), ptr(self.act['ws']), M, N, hip.code(self.dtype), stream())

    def _drop_apply(self, src, dst, count, p, seed):
        run.ecgvit_dropout_apply(ptr(src), ptr(dst), count, p, seed, hip.code(self.dtype), stream())

    def _wgrad(self, dY, X, name, Mout, Nin, rows, pre=None, x8=None, xsite=None):
        """dW[Mout, Nin] = dY[rows, Mout]^T . X[rows, Nin]  -> f32 gradient view (overwritten).  fp8_linear: pre = (e5m2 copy of dY,
        scale) from `_grad8`, x8 / xsite = the layer's persistent e4m3 copy of X and its site (scale): the product then runs on the
        8-bit streaming kernel (both operands k-major, transposed 8-bit LDS reads).  Nothing runs for a frozen weight (backward plan)."""
        if not self._wants(name):
            return
        if pre is not None and x8 is not None and Mout % 256 == 0 and Nin % 256 == 0 and rows >= 4096:
            q, sc = pre
            self._gemm(GEMM_TN, q, x8, self.G32[name], Mout, Nin, rows, Mout, Nin, Nin, workspace=self.act['ws'], fp8_format=hip.BF8_E5M2,
                       scale_a=sc, scale_b=self.f8_scale[xsite:xsite + 1])
            return
        if self.fp8 and name.startswith('vit.transformer.'):
            self._bf16_reader(rows, 'weight gradient of ' + name)
        self._gemm(GEMM_TN, dY, X, self.G32[name], Mout, Nin, rows, Mout, Nin, Nin, workspace=self.act['ws'])

    # ---------------------------------------------------------------- forward
    def _patch_rows(self, x):
        """a4: patch Rearrange (integer gather) + Linear(C*P, d) over the patch rows of the current pass (`saved`), whatever its row layout
        [+ f2: Normalize / TimeEndPad / TimeOut fused into the load]"""
        a, sv, T = self.act, self.saved, hip.code(self.dtype)
        B, rg, geo, ntok = sv['B'], sv.get('ragged'), sv.get('geo'), sv.get('ntok')
        xf = self.input_transform
        if sv.get('raw') is not None:   # f2 per record: raw records of unequal length, either row layout
            self._gather_raw(x, sv['raw'], sv['training'])
        elif xf is not None:
            mean, inv_std = xf.device_stats(x.device)
            t0 = tl = None
            if xf.timeout and sv['training']:
                t0, tl = xf.draw_timeout(B, self.L, x.device)
            self._xf_keep = (mean, inv_std, t0, tl)   # keep the int32 spans alive until the kernel has run
            run.ecgvit_patch_gather_transform(ptr(x), ptr(a['patches']), B, self.C, x.shape[2], self.L, self.P, self.CP, ptr(mean),
                                              ptr(inv_std), ptr(t0), ptr(tl), T, stream())
        elif rg is not None:   # packed rows: the uniform gather over the concatenation (patch row off_b / P + j is patch j of record b)
            run.ecgvit_patch_gather(ptr(x), ptr(a['patches']), 1, self.C, rg.S, self.P, self.CP, T, stream())
        elif ntok is not None:   # zero patches past each record's length.  The kernel's count includes a CLS token: the masked padded
            # form, whose ntok = n_b counts patches only, passes n_cls = n_b + 1
            cnt = ntok if geo is None else geo.n_cls
            run.ecgvit_patch_gather_varlen(ptr(x), ptr(a['patches']), ptr(cnt), B, self.C, self.L, self.P, self.CP, T, stream())
        else:
            run.ecgvit_patch_gather(ptr(x), ptr(a['patches']), B, self.C, self.L, self.P, self.CP, T, stream())
        rows = self._pass_rows(B) - (0 if sv['masked'] else B)   # (no CLS rows among the patch rows)
        self._gemm(GEMM_NT, a['patches'], self.W['vit.to_patch_embedding.1.weight'], a['tok'], rows, self.d, self.CP, self.CP, self.CP, self.d,
                   epilogue=EPI_BIAS, bias=self.P32['vit.to_patch_embedding.1.bias'])

    def _gather_raw(self, x, rs, training):
        """f2 per record (`FusedInputTransform(per_record=True)`): Normalize / TimeEndPad / TimeOut of every record at its own raw length,
        fused into the patch gather (reference: one record at a time on the host, ptb_dataset.py:132-149) -> act['patches'], rows as `rs`
        (`RawSide`) lays them out.  TimeOut (training passes): the spans are drawn here, per record in batch order, so consecutive
        micro-batches consume the generator as the unsplit batch does; two int32 per record through pinned memory."""
        xf = self.input_transform
        mean, inv_std = xf.device_stats(x.device)
        t0 = tl = None
        if xf.timeout and training:
            span = _stage(xf.draw_timeout_records(rs.padded), x.device)
            t0, tl = span[0], span[1]
        self._xf_keep = (mean, inv_std, t0, tl, rs)   # keep the tables alive until the kernel has run
        run.ecgvit_patch_gather_transform_varlen(ptr(x), ptr(self.act['patches']), ptr(rs.src_off), rs.lead_stride, ptr(rs.raw_len),
                                                 ptr(rs.n_patch), ptr(rs.row_off), rs.nrows, rs.n_max, rs.B, self.C, self.P, self.CP,
                                                 ptr(mean), ptr(inv_std), ptr(t0), ptr(tl), hip.code(self.dtype), stream())

    def check_raw_input(self, x, lengths):
        """validate a padded (B, C, W) batch of RAW records for this engine's per-record input transform before anything launches ->
        RawPaddedBatch.  lengths: the (B,) raw sample counts (`check_raw_lengths`; None = every record holds W samples), or the
        RawPaddedBatch of x itself (validated once by the caller)."""
        if self.fp8:
            raise ValueError('per-record lengths are not supported with fp8_linear')
        if not isinstance(x, torch.Tensor) or x.dim() != 3 or x.shape[1] != self.C or x.shape[0] < 1:
            raise ValueError(f'a batch of raw records is (B, {self.C}, W), got {tuple(getattr(x, "shape", ()))}')
        if isinstance(lengths, RawPaddedBatch):
            if lengths.B != x.shape[0] or lengths.W != x.shape[2] or lengths.P != self.P or lengths.device != x.device:
                raise ValueError(f'the RawPaddedBatch describes {lengths.B} records of width {lengths.W} at patch_size={lengths.P} on '
                                 f'{lengths.device}, the batch is {tuple(x.shape)} on {x.device} at patch_size={self.P}')
            return lengths
        B, W = x.shape[0], x.shape[2]
        if lengths is None:
            lengths = torch.full((B,), W, dtype=torch.int64)
        raw, padded = check_raw_lengths(lengths, self.input_transform, self.L_max, B=B, width=W)
        return RawPaddedBatch(raw, padded, self.P, self.C, W, x.device)

    def _trunk_fwd(self, B, ph, seed, cls_only_last=False):
        """L x { x = Attn(LN(x)) + x ; x = FF(LN(x)) + x } on act['x0'] ([B*T, d]); returns the output slab (cls_only_last: the last
        block's CLS rows only, compact [B, d] -- see `_cls_block_fwd`)"""
        a = self.act
        d, f = self.d, self.f
        M = self._pass_rows(B)
        pre = 'vit.'
        X = a['x0']
        for i, L in enumerate(a['layers']):
            lp = f'{pre}transformer.layers.{i}.'
            s0 = seed + 100 * (i + 1)
            if cls_only_last and i == self.Ly - 1:
                return self._cls_block_fwd(L, X, B, ph, s0, lp)
            # a6/a7: PreNorm(Attention)
            q1 = self._ln_fwd(X, self.P32[lp + '0.norm.weight'], self.P32[lp + '0.norm.bias'], L['xn1'], L['mean1'], L['rstd1'], M, q8_site=8 * i,
                              y8=L.get('xn1_8'))
            self._linear(8 * i + 0, L['xn1'], lp + '0.fn.to_qkv.weight', L['qkv'], M, 3 * d, d, a8=L.get('xn1_8'), prequant=q1)
            qa = self._attention_fwd(L, i, B, ph, s0 + 1)
            epi = EPI_BIAS | EPI_RESIDUAL | (EPI_DROPOUT if ph > 0 else 0)
            self._linear(8 * i + 1, L['attn'], lp + '0.fn.to_out.0.weight', L['x1'], M, d, d, a8=L.get('attn_8'), prequant=qa, epilogue=epi,
                         bias=self.P32[lp + '0.fn.to_out.0.bias'], residual=X, ldr=d, dropout_p=ph, seed=s0 + 2)
            # a6/a8: PreNorm(FeedForward): Linear -> GELU(erf) -> Dropout -> Linear -> Dropout, + residual
            q2 = self._ln_fwd(L['x1'], self.P32[lp + '1.norm.weight'], self.P32[lp + '1.norm.bias'], L['xn2'], L['mean2'], L['rstd2'], M,
                              q8_site=8 * i + 2, y8=L.get('xn2_8'))
            # bf16 path: the saved tensor is gelu'(pre) * dropout multiplier (not the pre-activation): the backward of this site is then
            # one multiply in the input-gradient GEMM's epilogue -- no erf, no mask hash; the f32 parity path keeps the pre-activation
            epi = EPI_BIAS | EPI_GELU | (EPI_DROPOUT if ph > 0 else 0) | (EPI_GELU_GRAD_AUX if self.dtype == torch.bfloat16 else 0)
            if self._aux8(M):
                epi |= hip.EPI_AUX8
            hq = self._linear(8 * i + 2, L['xn2'], lp + '1.fn.net.0.weight', L['hact'], M, f, d, a8=L.get('xn2_8'), emit_site=8 * i + 3,
                              emit_to=L.get('hact_8'), prequant=q2, emit_only8=self._only8(M), epilogue=epi,
                              bias=self.P32[lp + '1.fn.net.0.bias'], aux=L['hpre'], ldaux=f, dropout_p=ph, seed=s0 + 3)
            epi = EPI_BIAS | EPI_RESIDUAL | (EPI_DROPOUT if ph > 0 else 0)
            self._linear(8 * i + 3, L['hact'], lp + '1.fn.net.3.weight', L['x2'], M, d, f, a8=L.get('hact_8'), prequant=hq, epilogue=epi,
                         bias=self.P32[lp + '1.fn.net.3.bias'], residual=L['x1'], ldr=d, dropout_p=ph, seed=s0 + 4)
            X = L['x2']
        return X

    def _attention_fwd(self, L, i, B, ph, seed):
        """a7: softmax(q k^T * scale) v of block i, qkv -> attn, on the kernel the current pass calls for.  Returns True when the kernel also
        wrote the e4m3 copy of its output (fp8_linear, once site 8 i + 1 has a scale)"""
        sv, st = self.saved, stream()
        h, dh, N = self.h, self.dh, self.T
        rg, ntok = sv.get('ragged'), sv.get('ntok')
        site = 8 * i + 1
        if rg is not None:
            run.ecgvit_attention_ragged_fwd(ptr(L['qkv']), ptr(L['attn']), ptr(L['lse']), ptr(rg.n_tok), ptr(rg.tok_off), B, N, h, dh, self.scale,
                                            ph, seed, st)
        elif self.dtype == torch.bfloat16 and ntok is not None:
            run.ecgvit_attention_varlen_fwd(ptr(L['qkv']), ptr(L['attn']), ptr(L['lse']), ptr(ntok), B, N, h, dh, self.scale, ph, seed, st)
        elif self.dtype == torch.bfloat16:
            if self.fp8 and self._pass_rows(B) >= 2048 and site in self._f8_seen and dh == 64:   # (dh = 128: no 8-bit emission, _linear quantises attn)
                run.ecgvit_attention_fwd_q8(ptr(L['qkv']), ptr(L['attn']), ptr(L['lse']), B, N, h, dh, self.scale, ph, seed, ptr(L['attn_8']),
                                            ptr(self.f8_scale[site:site + 1]), ptr(self.f8_amax[site:site + 1]), st)
                return True
            run.ecgvit_attention_fwd(ptr(L['qkv']), ptr(L['attn']), ptr(L['lse']), B, N, h, dh, self.scale, ph, seed, hip.BF16, st)
        else:
            self._attn_fwd_f32(L, B, ph, seed)
        return False

    def _attention_bwd(self, L, i, B, ph, seed):
        """backward of `_attention_fwd`: dattn -> dqkv.  Returns True when the kernel also wrote the e5m2 copy of dqkv (operand scratch)"""
        a, sv, st = self.act, self.saved, stream()
        d, h, dh, N = self.d, self.h, self.dh, self.T
        rg, ntok = sv.get('ragged'), sv.get('ntok')
        site = 8 * i + 7
        if rg is not None:
            run.ecgvit_attention_ragged_bwd(ptr(L['qkv']), ptr(L['attn']), ptr(a['dattn']), ptr(L['lse']), ptr(a['dqkv']), ptr(rg.n_tok),
                                            ptr(rg.tok_off), B, N, h, dh, self.scale, ph, seed, st)
        elif self.dtype == torch.bfloat16 and ntok is not None:
            run.ecgvit_attention_varlen_bwd(ptr(L['qkv']), ptr(L['attn']), ptr(a['dattn']), ptr(L['lse']), ptr(a['dqkv']), ptr(ntok), B, N, h,
                                            dh, self.scale, ph, seed, st)
        elif self.dtype == torch.bfloat16:
            if (self.fp8 and self._pass_rows(B) >= 2048 and site in self._f8_seen and dh == 64 and 128 < N <= 512
                    and N * 3 * d * 2 < 2 ** 31):   # (dh = 128: _grad8 quantises dqkv)
                run.ecgvit_attention_bwd_q8(ptr(L['qkv']), ptr(L['attn']), ptr(a['dattn']), ptr(L['lse']), ptr(a['dqkv']), B, N, h, dh, self.scale,
                                            ph, seed, ptr(a['q8']), ptr(self.f8_scale[site:site + 1]), ptr(self.f8_amax[site:site + 1]), st)
                return True
            run.ecgvit_attention_bwd(ptr(L['qkv']), ptr(L['attn']), ptr(a['dattn']), ptr(L['lse']), ptr(a['dqkv']), B, N, h, dh, self.scale, ph,
                                     seed, hip.BF16, st)
        else:
            self._attn_bwd_f32(L, B, ph, seed)
        return False

    def _attention_cls_fwd(self, L, B, ph, seed):
        """the CLS query of every record against all its keys (the pruned last block): qkv -> act['cls_attn'], act['cls_lse']"""
        a, st = self.act, stream()
        h, dh, N = self.h, self.dh, self.T
        ntok = self.saved.get('ntok')
        if ntok is not None:
            run.ecgvit_attention_varlen_cls_fwd(ptr(L['qkv']), ptr(a['cls_attn']), ptr(a['cls_lse']), ptr(ntok), B, N, h, dh, self.scale, ph, seed,
                                                st)
        else:
            run.ecgvit_attention_cls_fwd(ptr(L['qkv']), ptr(a['cls_attn']), ptr(a['cls_lse']), B, N, h, dh, self.scale, ph, seed,
                                         hip.code(self.dtype), st)

    def _attention_cls_bwd(self, L, B, ph, seed):
        """backward of `_attention_cls_fwd`: act['cls_dattn'] -> dK / dV of every row in act['dqkv'], the compact dQ in act['cls_dq']"""
        a, st = self.act, stream()
        h, dh, N = self.h, self.dh, self.T
        ntok = self.saved.get('ntok')
        if ntok is not None:
            run.ecgvit_attention_varlen_cls_bwd(ptr(L['qkv']), ptr(a['cls_attn']), ptr(a['cls_dattn']), ptr(a['cls_lse']), ptr(a['dqkv']),
                                                ptr(a['cls_dq']), ptr(ntok), B, N, h, dh, self.scale, ph, seed, st)
        else:
            run.ecgvit_attention_cls_bwd(ptr(L['qkv']), ptr(a['cls_attn']), ptr(a['cls_dattn']), ptr(a['cls_lse']), ptr(a['dqkv']), ptr(a['cls_dq']),
                                         B, N, h, dh, self.scale, ph, seed, hip.code(self.dtype), st)

    def _cls_block_fwd(self, L, X, B, ph, s0, lp):
        """the last block when only its CLS rows are consumed (the classifier reads x[:, 0]): LayerNorm 1 and the K / V columns of to_qkv
        over every row (the CLS query attends to all keys), everything after them over one row per record.  The compact launches draw the
        dropout bits of the rows they stand for (mask row pitch T), so the result is the full block's row 0.  Returns x2 of the CLS rows [B, d]"""
        a, W, P = self.act, self.W, self.P32
        d, f, N = self.d, self.f, self.T
        M = B * N
        self._ln_fwd(X, P[lp + '0.norm.weight'], P[lp + '0.norm.bias'], L['xn1'], L['mean1'], L['rstd1'], M)
        wqkv = W[lp + '0.fn.to_qkv.weight']   # [3d, d]: rows [q | k | v]
        self._gemm(GEMM_NT, L['xn1'], wqkv, L['qkv'], M, 2 * d, d, d, d, 3 * d, b_off=d * d, c_off=d)   # K, V of every row
        self._gemm(GEMM_NT, L['xn1'], wqkv, L['qkv'], B, d, d, N * d, d, N * 3 * d)                       # Q of the CLS rows, in place
        self._attention_cls_fwd(L, B, ph, s0 + 1)
        drop = EPI_DROPOUT if ph > 0 else 0
        self._gemm(GEMM_NT, a['cls_attn'], W[lp + '0.fn.to_out.0.weight'], a['cls_x1'], B, d, d, d, d, d, epilogue=EPI_BIAS | EPI_RESIDUAL | drop,
                   bias=P[lp + '0.fn.to_out.0.bias'], residual=X, ldr=N * d, dropout_p=ph, seed=s0 + 2, mask_row_pitch=N)
        self._ln_fwd(a['cls_x1'], P[lp + '1.norm.weight'], P[lp + '1.norm.bias'], a['cls_xn2'], a['cls_mean2'], a['cls_rstd2'], B)
        self._gemm(GEMM_NT, a['cls_xn2'], W[lp + '1.fn.net.0.weight'], a['cls_hact'], B, f, d, d, d, f,
                   epilogue=EPI_BIAS | EPI_GELU | EPI_GELU_GRAD_AUX | drop, bias=P[lp + '1.fn.net.0.bias'], aux=a['cls_hpre'], ldaux=f,
                   dropout_p=ph, seed=s0 + 3, mask_row_pitch=N)
        self._gemm(GEMM_NT, a['cls_hact'], W[lp + '1.fn.net.3.weight'], a['cls_x2'], B, d, f, f, f, d, epilogue=EPI_BIAS | EPI_RESIDUAL | drop,
                   bias=P[lp + '1.fn.net.3.bias'], residual=a['cls_x1'], ldr=d, dropout_p=ph, seed=s0 + 4, mask_row_pitch=N)
        return a['cls_x2']

    def forward(self, x, labels=None, weight=None, training=True, seed=0, want_mean=True, cls_only_last=False, lengths=None):
        """x: (B, C, L) f32 contiguous device tensor. Returns (logits (B,K) f32, loss_elem (B,K) f32 | None, loss_mean (1,) | None).
        cls_only_last: compute the last block for the CLS rows only (past its K / V), the rows the classifier reads -- same loss, logits and
        gradients, 1/12 of the base trunk less work.  bf16 engine without fp8_linear; the last block's other rows are then not computed
        (attention_probs of that layer is unavailable until the next full forward).
        x may be narrower than max_signal_length (a multiple of P): the pass then runs at L'/P + 1 tokens with position rows 0..L'/P.
        lengths: (B,) integer tensor (host or device) of per-record sample counts inside x (`check_lengths`); record b then gives what it
        would give alone at x[b:b+1, :, :lengths[b]] (dropout 0; up to summation order).  Not with fp8_linear or a fused input transform."""
        return self._head_loss(self._trunk_pass(x, labels, weight, training, seed, cls_only_last, lengths), want_mean)

    def _head_loss(self, X, want_mean):
        """the tail of a supervised forward: a10 x[:, 0] -> LayerNorm -> Linear(d, K), a11 BCEWithLogitsLoss.  The head reads one row per
        record at pitch saved['head_pitch']: N in the padded layout; 1 when X holds the CLS rows only (cls_only_last) or after gathering
        the CLS rows tok_off[b] of a ragged batch compact.  Returns (logits, loss_elem | None, loss_mean | None)"""
        a, sv, T = self.act, self.saved, hip.code(self.dtype)
        st = stream()
        B, d, rg, labels = sv['B'], self.d, sv['ragged'], sv['labels']
        pre = 'vit.'
        sv['head_pitch'] = 1 if (sv['cls_only_last'] or rg is not None) else self.N
        if rg is not None:
            run.ecgvit_gather_rows(ptr(X), ptr(rg.tok_off), ptr(a['cls_x2']), 1, rg.M, B, d, d, d, T, st)
            X = a['cls_x2']
        run.ecgvit_head_fwd(ptr(X), sv['head_pitch'], ptr(self.P32[pre + 'mlp_head.0.weight']), ptr(self.P32[pre + 'mlp_head.0.bias']),
                            ptr(self.P32[pre + 'mlp_head.1.weight']), ptr(self.P32[pre + 'mlp_head.1.bias']),
                            ptr(a['logits']), ptr(a['xhat']), ptr(a['hrstd']), B, d, self.K, LN_EPS, T, st)
        if labels is None:
            return a['logits'], None, None
        run.ecgvit_bce_fwd(ptr(a['logits']), ptr(labels), ptr(sv['weight']), ptr(a['loss_elem']),
                           ptr(a['loss_mean']) if want_mean else None, B * self.K, st)
        return a['logits'], a['loss_elem'], (a['loss_mean'] if want_mean else None)

    def _trunk_pass(self, x, labels, weight, training, seed, cls_only_last, lengths):
        """`forward` up to the trunk's output: validation, geometry, slabs, patch embedding, the L blocks.  Returns X = saved['xL'], the last
        block's output ([B * N, d], or the compact CLS rows [B, d] under cls_only_last).
        A ragged batch: x (C, S) = the records concatenated along time, lengths (B,) their sample counts.  Every row-wise kernel runs over the
        M = S / P + B packed token rows; attention per record on the packed rows; the classifier reads the CLS rows tok_off[b].  The last
        block always runs in full (no cls_only_last).  Hidden and embedding dropout draw their bits by packed element index, so a ragged
        step does not draw the masks of the padded step of the same records (attention dropout does, on the valid region).  X: [M, d]"""
        if x.dim() == 2:
            rg = self.check_ragged_input(x, lengths, labels)
            self._set_width((rg.N - 1) * self.P)
            return self._supervised_trunk(x, rg.B, labels, weight, training, seed, lengths=True, ragged=rg, raw=rg.rawside)
        B = x.shape[0]
        assert x.shape[1] == self.C and x.dtype == torch.float32 and x.is_contiguous()
        rp = None
        if self.input_transform is None:
            width = x.shape[2]
            if width != self.L_max and self.fp8:
                raise ValueError(f'fp8_linear runs full-width batches only (max_signal_length={self.L_max}, got {width} samples)')
        elif self.input_transform.per_record:   # RAW records: lengths are raw sample counts, the pass runs at the widest padded length
            rp = self.check_raw_input(x, lengths)
            width, lengths = rp.width, None
        else:
            if lengths is not None:
                raise ValueError('per-record lengths are not supported with a fused input transform (its TimeEndPad pads every record) '
                                 'unless it is built with per_record=True')
            assert self.input_transform.padded_length(x.shape[2]) == self.L_max, 'config.max_signal_length must be the padded length'
            width = self.L_max
        if lengths is not None and self.fp8:
            raise ValueError('per-record lengths are not supported with fp8_linear')
        cls_only_last = bool(cls_only_last)
        if cls_only_last and (self.dtype != torch.bfloat16 or self.fp8):
            raise ValueError('cls_only_last needs the bf16 engine without fp8_linear')
        self._set_width(width)
        ntok = None
        if lengths is not None:
            ntok = check_lengths(lengths, B, self.P, width)
            if ntok is not None and not ntok.is_cuda:
                ntok = _stage(ntok, x.device)
        if rp is not None:
            ntok = rp.ntok
        return self._supervised_trunk(x, B, labels, weight, training, seed, cls_only_last=cls_only_last, ntok=ntok,
                                      lengths=lengths is not None or ntok is not None, raw=None if rp is None else rp.rawside)

    def _supervised_trunk(self, x, B, labels, weight, training, seed, cls_only_last=False, ntok=None, lengths=False, ragged=None, raw=None):
        """a validated supervised batch at the width already set, from the slabs to the trunk's output X = saved['xL'].  ragged: the
        RaggedBatch of packed rows; ntok: per-record token counts of padded rows; raw: the `RawSide` of raw records"""
        self._alloc(B, rows=None if ragged is None else ragged.M)
        a, T = self.act, hip.code(self.dtype)
        st = stream()
        ph = self.p_hidden if training else 0.0
        pe = self.p_emb if training else 0.0
        self.saved = dict(B=B, ph=ph, pe=pe, seed=seed, labels=labels, weight=weight, masked=False, training=training, cls_only_last=cls_only_last,
                          ntok=ntok, lengths=lengths, ragged=ragged, raw=raw)
        if self.fp8:
            # EVERY forward, eval included, starts from the scales of the pass before it (delayed scaling with a history of one pass): an
            # inference-only model otherwise keeps its first batch's scales forever and clamps larger activations silently.  No backward can be
            # waiting for the old scales: a later forward overwrites the activations that backward reads (one live graph per model -- the
            # autograd node raises on a stale backward)
            self.fp8_begin_step(training)
        self._patch_rows(x)
        # a5: cat CLS, += pos_embedding[:, :n+1], emb dropout
        cls, pos = self.P32['vit.cls_token'], self.P32['vit.pos_embedding']
        if ragged is not None:
            run.ecgvit_embed_finish_ragged(ptr(a['tok']), ptr(cls), ptr(pos), ptr(a['x0']), ptr(ragged.n_tok), ptr(ragged.tok_off), B, self.N,
                                           self.d, pe, seed + 1, T, st)
        else:
            run.ecgvit_embed_finish(ptr(a['tok']), ptr(cls), ptr(pos), ptr(a['x0']), B, self.n, self.d, pe, seed + 1, T, st)
        X = self._trunk_fwd(B, ph, seed, cls_only_last)
        self.saved['xL'] = X
        return X

    def check_ragged_input(self, x, lengths, labels=None):
        """validate a ragged (C, S) batch for this engine before anything launches -> RaggedBatch (`check_ragged`).  lengths may already be
        the RaggedBatch of x (validated once by the caller: no second read of the lengths); labels, when given, must hold one row per record"""
        xf = self.input_transform
        per_record = xf is not None and xf.per_record
        if xf is not None and not per_record:
            raise ValueError('ragged batches are not supported with a fused input transform (its TimeEndPad pads every record) '
                             'unless it is built with per_record=True')
        if self.fp8:
            raise ValueError('ragged batches are not supported with fp8_linear')
        if self.dtype != torch.bfloat16:
            raise ValueError('ragged batches need the bf16 engine (the f32 parity path materialises padded (B, h, N, N) scores)')
        if not isinstance(x, torch.Tensor) or x.dim() != 2 or x.shape[0] != self.C:
            raise ValueError(f'a ragged batch is a ({self.C}, S) tensor, got {tuple(getattr(x, "shape", ()))}')
        if x.dtype != torch.float32 or not x.is_contiguous():
            raise ValueError('a ragged batch must be a contiguous float32 tensor')
        if isinstance(lengths, RaggedBatch):
            if lengths.S_raw != x.shape[1] or lengths.P != self.P or lengths.device != x.device or (lengths.raw is not None) != per_record:
                raise ValueError(f'the RaggedBatch describes S={lengths.S_raw} samples at patch_size={lengths.P} on {lengths.device}'
                                 f'{" (raw records)" if lengths.raw is not None else ""}, '
                                 f'the batch is ({x.shape[0]}, {x.shape[1]}) on {x.device} at patch_size={self.P}')
            rg = lengths
        elif per_record:   # (C, S_raw): lengths are RAW sample counts, the packed token rows those of the padded lengths
            raw, padded = check_raw_lengths(lengths, xf, self.L_max, S=x.shape[1])
            rg = RaggedBatch(padded, self.P, x.device, raw)
        else:
            rg = check_ragged(lengths, x.shape[1], self.P, self.L_max, device=x.device)
        if labels is not None and labels.shape[0] != rg.B:
            raise ValueError(f'labels must hold one row per record: {rg.B} records, got {labels.shape[0]} label rows')
        return rg

    # ---------------------------------------------------------------- pooled representations (EcgVit.encode)
    POOL_MODES = {'cls': hip.POOL_CLS, 'mean': hip.POOL_MEAN}

    def encode(self, x, lengths=None, pool='cls', norm=True):
        """One vector per record, (B, d) f32 in a fresh tensor: an EVAL pass (no dropout, no TimeOut) of `forward` up to the trunk's output,
        then one `ecgvit_pool_records` launch.  x / lengths: every batch form `forward` takes, with its validation and refusals.
        pool 'cls': the record's CLS row (bf16 engine without fp8_linear, padded batches: the last block runs for the CLS rows only);
        'mean': the mean over the record's own tokens, CLS row included (the full last block).  norm: through vit.mlp_head.0 (LayerNorm).
        Overwrites the activations like any forward."""
        if pool not in self.POOL_MODES:
            raise ValueError(f"pool must be 'cls' or 'mean', got {pool!r}")
        prune = pool == 'cls' and x.dim() == 3 and self.dtype == torch.bfloat16 and not self.fp8
        self._trunk_pass(x, None, None, False, 0, prune, lengths)
        return self.pool_saved(pool, norm)

    def pool_saved(self, pool='cls', norm=True):
        """pool the trunk output of the LAST supervised forward (saved['xL']) on its own row base: the padded rows with the per-record token
        counts, the packed rows of a ragged batch, or the compact CLS rows of a pruned last block (which hold no other row: pool='mean' then
        raises ValueError)"""
        if pool not in self.POOL_MODES:
            raise ValueError(f"pool must be 'cls' or 'mean', got {pool!r}")
        sv = self.saved
        if sv is None or sv.get('masked') or sv.get('xL') is None:
            raise RuntimeError('pool_saved needs the trunk output of a supervised forward')
        n_tok, tok_off, N = *self._row_tables(sv), self.N
        if sv.get('cls_only_last'):
            if pool != 'cls':
                raise ValueError("pool='mean' needs every token row: the last forward computed the last block's CLS rows only (cls_only_last)")
            n_tok, tok_off, N = None, None, 1
        B, pre = sv['B'], 'vit.'
        out = torch.empty((B, self.d), dtype=torch.float32, device=sv['xL'].device)
        g, b = (self.P32[pre + 'mlp_head.0.weight'], self.P32[pre + 'mlp_head.0.bias']) if norm else (None, None)
        run.ecgvit_pool_records(ptr(sv['xL']), ptr(out), ptr(n_tok), ptr(tok_off), B, N, self.d, self.POOL_MODES[pool], ptr(g), ptr(b),
                                LN_EPS, hip.code(self.dtype), stream())
        return out

    @staticmethod
    def _row_tables(sv):
        """(n_tok, tok_off) of the pass `sv` describes: the packed rows of a ragged batch, per-record token counts of padded rows, or neither"""
        rg = sv.get('ragged')
        return (rg.n_tok, rg.tok_off) if rg is not None else (sv.get('ntok'), None)

    def _pass_rows(self, B):
        """token rows of the current pass: B x tokens per record, or the packed rows of a ragged batch"""
        rg = self.saved.get('ragged') if self.saved is not None else None
        return rg.M if rg is not None else B * self.T

    # ---------------------------------------------------------------- masked pre-train objective
    def forward_masked(self, x, idx, training=True, seed=0):
        """SimMIM-style step (build's own definition; absent from the reference): tokens = Linear(patches); masked tokens <-
        mask_token; + pos[1:n+1]; trunk on n tokens (no CLS); masked rows -> Linear(d, C*P); L1 vs the raw masked patches.
        x (B,C,L) f32; idx (B,m) int32 distinct patch indices per record. Returns (pred (B*m, C*P), loss (1,) f32)."""
        B, m = idx.shape
        self._set_width(self.L_max)   # (B, m) indices: full-width records; records of unequal length go through forward_masked_varlen
        assert idx.dtype == torch.int32 and idx.is_contiguous() and 0 < m <= self.n
        self._alloc(B, masked=True, m=m)
        a, n, d = self.act, self.n, self.d
        ph, pe = (self.p_hidden, self.p_emb) if training else (0.0, 0.0)
        self.saved = dict(B=B, ph=ph, pe=pe, seed=seed, masked=True, idx=idx, m=m, mrows=(B, n, m), training=training)
        if self.fp8:
            self.fp8_begin_step(training)
        self._patch_rows(x)
        run.ecgvit_mask_embed_finish(ptr(a['tok']), ptr(self.P32['pretrain.mask_token']), ptr(self.P32['vit.pos_embedding']),
                                     ptr(idx), ptr(a['x0']), ptr(a['flag']), B, n, m, d, hip.code(self.dtype), stream())
        return self._masked_trunk_and_loss()

    def _masked_trunk_and_loss(self):
        """a masked pass from act['x0'] on: embedding dropout, the L blocks, masked rows -> Linear(d, C*P), L1 against the same rows of the
        raw patches.  saved['mrows'] = (batches, rows per batch, indices per batch) is how saved['idx'] addresses the masked rows: (B, n, m)
        for (B, m) record-local indices, (1, M, sum m_b) for row numbers of the whole pass.  Returns (pred, loss (1,))"""
        a, sv, T = self.act, self.saved, hip.code(self.dtype)
        st = stream()
        B, pe, seed, idx, d, CP = sv['B'], sv['pe'], sv['seed'], sv['idx'], self.d, self.CP
        nb, nrow, m = sv['mrows']
        if pe > 0:
            self._drop_apply(a['x0'], a['x0'], self._pass_rows(B) * d, pe, seed + 1)
        X = self._trunk_fwd(B, sv['ph'], seed)
        sv['xL'] = X
        run.ecgvit_gather_rows(ptr(X), ptr(idx), ptr(a['rows']), nb, nrow, m, d, d, d, T, st)
        self._gemm(GEMM_NT, a['rows'], self.W['pretrain.to_pixels.weight'], a['pred'], nb * m, CP, d, d, d, CP, epilogue=EPI_BIAS,
                   bias=self.P32['pretrain.to_pixels.bias'])
        run.ecgvit_gather_rows(ptr(a['patches']), ptr(idx), ptr(a['target']), nb, nrow, m, CP, CP, CP, T, st)
        # L1 loss and d(loss)/d(pred) in one pass (upstream gradient 1; backward_masked re-runs it for any other upstream)
        run.ecgvit_l1_loss_fwd_bwd(ptr(a['pred']), ptr(a['target']), ptr(a['mloss']), ptr(a['dpred']), None, ptr(a['l1part']), nb * m, CP, CP, T, st)
        return a['pred'], a['mloss']

    def check_masked_varlen_input(self, x, mask_idx, lengths, mask_counts):
        """`check_masked_varlen_input` for this engine"""
        return check_masked_varlen_input(x, mask_idx, lengths, mask_counts, C=self.C, P=self.P, max_len=self.L_max, dtype=self.dtype, fp8=self.fp8,
                                         input_transform=self.input_transform)

    def forward_masked_varlen(self, x, geo, training=True, seed=0):
        """`forward_masked` over records of unequal length (`MaskedVarlenBatch`, from `check_masked_varlen_input`): record b gives what it
        gives alone at its own length (dropout 0); the loss is the mean over every masked element of the batch.  x: the ragged (C, S) batch
        (packed rows: every row-wise kernel runs over the M = S / P rows, attention per record on the packed rows) or (B, C, L') (padded rows:
        the rows past a record's length are exact zeros, its keys there never attended to, its samples there never read).
        Returns (pred (sum m_b, C*P), loss (1,) f32)."""
        B, M, mt, packed = geo.B, geo.M, geo.m, geo.n_pad == 0
        assert x.dtype == torch.float32 and x.is_contiguous() and geo.rows is not None
        self._set_width((geo.N if packed else geo.n_pad) * self.P)
        self._alloc(B, masked=True, rows=M if packed else None, mrows=mt)
        a = self.act
        ph, pe = (self.p_hidden, self.p_emb) if training else (0.0, 0.0)
        self.saved = dict(B=B, ph=ph, pe=pe, seed=seed, masked=True, idx=geo.rows, m=mt, mrows=(1, M, mt), training=training, geo=geo, lengths=True,
                          ntok=None if packed else geo.n_tok, ragged=geo if packed else None, raw=geo.rawside)
        self._patch_rows(x)
        run.ecgvit_mask_embed_varlen_fwd(ptr(a['tok']), ptr(self.P32['pretrain.mask_token']), ptr(self.P32['vit.pos_embedding']), ptr(geo.rows),
                                         ptr(a['x0']), ptr(a['flag']), ptr(geo.n_tok), ptr(geo.tok_off), B, geo.N, geo.n_pad, M, mt, self.d,
                                         hip.code(self.dtype), stream())
        return self._masked_trunk_and_loss()

    def backward_masked(self, gscalar=None, tiles_per_workgroup=0, trainable=None):
        """loss + every gradient of the masked objective (the L1 kernel produces loss and dpred in one pass).
        tiles_per_workgroup, trainable: as `backward`"""
        self._tpw = int(tiles_per_workgroup)
        self._begin_plan(trainable, masked=True)
        try:
            self._backward_masked(gscalar)
            self._ready_rest()
        finally:
            self._tpw = 0
            self._plan = None

    def _backward_masked(self, gscalar):
        a, W, T = self.act, self.W, hip.code(self.dtype)
        st = stream()
        sv = self.saved
        B, idx, pe, seed = sv['B'], sv['idx'], sv['pe'], sv['seed']
        d, n = self.d, self.n
        G = self.G32
        M = self._pass_rows(B)
        nb, nrow, m = sv['mrows']   # how idx addresses the masked rows (`_masked_trunk_and_loss`)
        Rm = nb * m
        if gscalar is not None:
            run.ecgvit_l1_loss_fwd_bwd(ptr(a['pred']), ptr(a['target']), ptr(a['mloss']), ptr(a['dpred']), ptr(gscalar), ptr(a['l1part']), Rm,
                                       self.CP, self.CP, T, st)
        # the classification head does not take part: its gradients are zero for this objective -- known at once, so its bucket is
        # released FIRST and its exchange overlaps the whole backward pass (buckets complete in the order head, layers L-1..0, embed,
        # pretrain, as in the supervised pass)
        for k in ('vit.mlp_head.0.weight', 'vit.mlp_head.0.bias', 'vit.mlp_head.1.weight', 'vit.mlp_head.1.bias', 'vit.cls_token'):
            G[k].zero_()
        self._ready('head')
        self._colsum(a['dpred'], self.CP, G['pretrain.to_pixels.bias'], Rm, self.CP)
        self._wgrad(a['dpred'], a['rows'], 'pretrain.to_pixels.weight', self.CP, d, Rm)
        if not self._reach(0):
            return
        self._gemm(GEMM_NN, a['dpred'], W['pretrain.to_pixels.weight'], a['drows'], Rm, d, self.CP, self.CP, d, d)
        dX = a['dxa']
        dX.zero_()
        run.ecgvit_scatter_rows(ptr(a['drows']), ptr(idx), ptr(dX), nb, nrow, m, d, d, d, T, st)
        dX = self._trunk_bwd(dX, a['dxb'])
        if dX is None or not self._reach(self._stage(-1, 0)):
            return
        if pe > 0:
            self._drop_apply(dX, dX, M * d, pe, seed + 1)
        geo = sv.get('geo')   # records of unequal length
        if geo is not None:
            run.ecgvit_mask_embed_varlen_bwd(ptr(dX), ptr(a['flag']), ptr(a['dtok']), ptr(a['dmasked']), ptr(G['vit.pos_embedding']),
                                             ptr(geo.n_tok), ptr(geo.tok_off), ptr(geo.order), B, geo.N, geo.n_pad, d, T, st)
            if n < self.n_max:   # the kernel wrote position rows 0 .. n (n = the pass's patches per record); the rest take no part
                G['vit.pos_embedding'].view(-1, d)[1 + n:].zero_()
        else:
            run.ecgvit_mask_embed_bwd(ptr(dX), ptr(a['flag']), ptr(a['dtok']), ptr(a['dmasked']), ptr(G['vit.pos_embedding']), B, n, d,
                                      T, st)
        self._colsum(a['dmasked'], d, G['pretrain.mask_token'], M, d)
        self._colsum(a['dtok'], d, G['vit.to_patch_embedding.1.bias'], M, d)
        self._wgrad(a['dtok'], a['patches'], 'vit.to_patch_embedding.1.weight', d, self.CP, M)
        self._ready('embed')
        self._ready('pretrain')

    def _attn_fwd_f32(self, L, B, ph, seed):
        """f32 parity path of Attention.forward: dots = q k^T * scale (batched exact-f32 MFMA GEMM), softmax, attn v."""
        d, h, dh, N = self.d, self.h, self.dh, self.T
        qkv, S = L['qkv'], L['probs']
        sq = (N * 3 * d, dh)
        self._gemm(GEMM_NT, qkv, qkv, S, N, N, dh, 3 * d, 3 * d, N, alpha=self.scale, batch=(B, h), strideA=sq, strideB=sq,
                 strideC=(h * N * N, N * N), b_off=d)
        ntok = self.saved.get('ntok')
        if ntok is not None:   # keys past each record's length get probability 0, its padded query rows all zeros
            run.ecgvit_softmax_rows_varlen(ptr(S), ptr(ntok), B, h, N, N, stream())
        else:
            run.ecgvit_softmax_rows(ptr(S), B * h * N, N, N, stream())
        Pd = S
        if ph > 0:
            Pd = self.act['pd']
            self._drop_apply_f32(S, Pd, B * h * N * N, ph, seed)
        self._gemm(GEMM_NN, Pd, qkv, L['attn'], N, dh, N, N, 3 * d, d, batch=(B, h), strideA=(h * N * N, N * N), strideB=sq,
                 strideC=(N * d, dh), b_off=2 * d)

    def _drop_apply_f32(self, src, dst, count, p, seed):
        # f32 parity path: the 16-bit pair hash of `ecgvit_dropout_apply` over element index ((b*h + head)*N + q)*N + key, exact p.
        # NOT the fused bf16 kernels' mask (one 8-bit hash per four keys, p rounded to 1/256, pitch ceil(N/4)): the two paths drop
        # different units, each consistently between its own forward and backward
        cnt8 = count // 8 * 8
        run.ecgvit_dropout_apply(ptr(src), ptr(dst), cnt8, p, seed, hip.F32, stream())
        if cnt8 != count:
            raise ValueError('f32 attention dropout needs B*h*N*N to be a multiple of 8')

    # ---------------------------------------------------------------- backward
    def backward(self, gscalar=None, gelem=None, gscale=1.0, glogits=None, tiles_per_workgroup=0, trainable=None):
        """Overwrites every gradient view in gflat. Upstream: `gscalar` (1,) for the mean loss, or `gelem` (B,K) for
        reduction='none'; gscale folds the 1/(B*K) of the mean. `glogits` (B,K): extra upstream gradient on the logits.
        tiles_per_workgroup > 0: this pass's large A.B^T launches run as dispatcher-balanced chunks of about that many tiles (the
        caller overlaps RCCL collectives with the pass, whose kernels hold CUs); the setting ends with the pass, exception or not.
        trainable: the names of the trainable parameters (None = all: the full pass).  Otherwise (`BackwardPlan`) only the gradients of
        those parameters are guaranteed: no weight-gradient product runs for a frozen Linear weight, and the pass stops after the last
        stage a trainable parameter needs (nothing below it is launched; only buckets holding a trainable parameter are reported to
        `on_grads_ready`).  The fused by-products of stages that do run are still written, frozen or not: the bias gradients reduced in GEMM
        epilogues and colsum passes (FFN-up / FFN-down / out-projection / patch-embedding biases), the LayerNorm gamma / beta of the fused
        LayerNorm backward, the classification head's four gradients, and the zeroed gradients of parameters outside the objective.  The
        gradients of frozen parameters are otherwise left as they were."""
        self._tpw = int(tiles_per_workgroup)
        self._begin_plan(trainable, masked=False)
        try:
            self._backward(gscalar, gelem, gscale, glogits)
            self._ready_rest()
        finally:
            self._tpw = 0
            self._plan = None

    _plan = None

    def _begin_plan(self, trainable, masked):
        """the backward plan of this pass: None (full pass) when `trainable` is None or names every parameter"""
        self._reported = set()
        if trainable is None:
            self._plan = None
            return
        key = (frozenset(trainable), masked)
        if len(key[0]) == len(self.layout.entries) and key[0] == set(self.layout.entries):
            self._plan = None
            return
        if getattr(self, '_plan_key', None) != key:
            self._plan_cached = BackwardPlan(list(self.layout.entries), self.Ly, key[0], masked=masked)
            self._plan_key = key
        self._plan = self._plan_cached

    def _stage(self, i, k):
        """BackwardPlan stage index of step k of block i (i = -1: the embedding backward)"""
        return 1 + 7 * self.Ly if i < 0 else 1 + 7 * (self.Ly - 1 - i) + k

    def _reach(self, stage):
        return self._plan is None or stage <= self._plan.depth

    def _wants(self, name):
        """does the weight-gradient product of Linear weight `name` run in this pass"""
        return self._plan is None or name in self._plan.wgrad

    def _ready_rest(self):
        """a pass that a plan stopped early: every live bucket not reported yet is final (nothing more will write it)"""
        if self._plan is not None:
            for tag, _ in self.layout.buckets_in_ready_order(self.Ly):
                self._ready(tag)

    def _backward(self, gscalar, gelem, gscale, glogits):
        a, T = self.act, hip.code(self.dtype)
        st = stream()
        sv = self.saved
        B, pe, seed = sv['B'], sv['pe'], sv['seed']
        d, N, n = self.d, self.N, self.n
        rg = sv.get('ragged')
        M = self._pass_rows(B)
        Mp = M - B
        pre = 'vit.'
        G = self.G32
        if sv['labels'] is not None and (gscalar is not None or gelem is not None):
            run.ecgvit_bce_bwd(ptr(a['logits']), ptr(sv['labels']), ptr(sv['weight']), ptr(gscalar), ptr(gelem), gscale,
                               ptr(a['dlogits']), B * self.K, st)
            dlog = a['dlogits']
            if glogits is not None:
                raise NotImplementedError('simultaneous loss and logits upstream gradients')
        elif glogits is not None:
            dlog = glogits
        else:
            raise ValueError('backward needs an upstream gradient')
        cls, pitch = sv.get('cls_only_last', False), sv.get('head_pitch')   # (pitch 1: the head read compact CLS rows -- `_head_loss`)
        if pitch is None:
            raise RuntimeError('backward needs a supervised forward: the last pass (encode, or a hand-made `saved`) did not run the head')
        dX = a['cls_dx'] if cls else a['dxa']   # (cls_only_last: the gradient of the CLS rows only, compact)
        if not self._reach(0):   # frozen parameters: nothing trainable takes part in this objective's backward
            self._zero_pretrain_grads()
            return
        run.ecgvit_head_bwd(ptr(dlog), ptr(a['xhat']), ptr(a['hrstd']), ptr(self.P32[pre + 'mlp_head.0.weight']),
                            ptr(self.P32[pre + 'mlp_head.0.bias']), ptr(self.P32[pre + 'mlp_head.1.weight']),
                            ptr(G[pre + 'mlp_head.1.weight']), ptr(G[pre + 'mlp_head.1.bias']),
                            ptr(G[pre + 'mlp_head.0.weight']), ptr(G[pre + 'mlp_head.0.bias']),
                            ptr(a['cls_dx'] if pitch == 1 else dX), pitch, B, d, self.K, T, st)
        if rg is not None:   # the CLS rows' gradient, compact -> rows tok_off[b]; every other row 0
            dX[:M].zero_()
            run.ecgvit_scatter_rows(ptr(a['cls_dx']), ptr(rg.tok_off), ptr(dX), 1, M, B, d, d, d, T, st)
        self._ready('head')
        dX = self._trunk_bwd(dX, a['dxb'], cls_only_last=cls)
        self._zero_pretrain_grads()
        if dX is None or not self._reach(self._stage(-1, 0)):
            return
        # ---- embedding backward
        if rg is not None:
            run.ecgvit_embed_bwd_ragged(ptr(dX), ptr(a['dtok']), ptr(G[pre + 'cls_token']), ptr(G[pre + 'pos_embedding']), ptr(rg.n_tok),
                                        ptr(rg.tok_off), B, N, d, pe, seed + 1, T, st)
        else:
            run.ecgvit_embed_bwd(ptr(dX), ptr(a['dtok']), ptr(G[pre + 'cls_token']), ptr(G[pre + 'pos_embedding']), B, n, d, pe,
                                 seed + 1, T, st)
        if N < self.N_max:   # a narrower pass: embed_bwd wrote position rows < N only, the rest take no part
            G[pre + 'pos_embedding'].view(-1, d)[N:].zero_()
        self._colsum(a['dtok'], d, G[pre + 'to_patch_embedding.1.bias'], Mp, d)
        self._wgrad(a['dtok'], a['patches'], pre + 'to_patch_embedding.1.weight', d, self.CP, Mp)
        self._ready('embed')

    def _zero_pretrain_grads(self):
        for k in self.G32:
            if k.startswith('pretrain.'):
                self.G32[k].zero_()   # the masked-objective head takes no part in the supervised step
        self._ready('pretrain')

    def _ready(self, tag):
        if self._plan is not None:   # frozen parameters: buckets without a trainable parameter are never reported, the others once
            if tag not in self._plan.live or tag in self._reported:
                return
            self._reported.add(tag)
        if self.on_grads_ready is not None:
            self.on_grads_ready(tag)

    def _trunk_bwd(self, dX, other, cls_only_last=False):
        """backward of _trunk_fwd: consumes dX = d(loss)/d(x_L) ([B*T, d]; cls_only_last: [B, d], the CLS rows), fills every layer's
        parameter gradients, returns d(x_0) -- or None when a backward plan (frozen parameters) stopped the pass inside the trunk"""
        a, sv = self.act, self.saved
        B, ph, seed = sv['B'], sv['ph'], sv['seed']
        d, f = self.d, self.f
        M = self._pass_rows(B)
        pre = 'vit.'
        G = self.G32
        # dY = gradient entering the current `dropout(Linear + bias) + residual` site (masked copy of dX when dropout is on);
        # after the first site, the fused LayerNorm backward of the previous stage has already produced it AND its bias gradient
        have = False
        dY = dX
        pq4 = pq6 = False   # fp8_linear: the LayerNorm backward before a site already wrote its e5m2 operand copy
        top = self.Ly
        if cls_only_last:
            top -= 1
            dX, other = self._cls_block_bwd(dX, a['dxa'], other, B, ph, seed)
            if dX is None:
                return None
            have, dY = True, (a['dxm'] if ph > 0 else dX)
        for i in reversed(range(top)):
            L = a['layers'][i]
            lp = f'{pre}transformer.layers.{i}.'
            s0 = seed + 100 * (i + 1)
            Xin = a['x0'] if i == 0 else a['layers'][i - 1]['x2']
            # ---- FeedForward backward: x2 = drop(hact W2^T + b2) + x1
            if not have:
                dY = dX
                if ph > 0:
                    self._drop_apply(dX, a['dxm'], M * d, ph, s0 + 4)
                    dY = a['dxm']
                self._colsum(dY, d, G[lp + '1.fn.net.3.bias'], M, d)
            f8 = self.fp8 and M >= 2048
            b = self._stage(i, 0)   # frozen parameters: the pass stops before the first input-gradient stage nothing trainable needs
            g4 = self._grad8(8 * i + 4, dY, M * d, prequant='q8' if pq4 else False) if f8 and (self._wants(lp + '1.fn.net.3.weight') or self._reach(b)) else None
            self._wgrad(dY, L['hact'], lp + '1.fn.net.3.weight', d, f, M, pre=g4, x8=L.get('hact_8'), xsite=8 * i + 3)
            # dgrad with GELU' (+ dropout mask) epilogue; the epilogue also reduces the columns = gradient of the FFN-up bias
            if self.dtype == torch.bfloat16:
                epi, pdrop = EPI_MUL_AUX | EPI_COLSUM | (hip.EPI_AUX8 if self._aux8(M) else 0), 0.0
            else:
                epi, pdrop = EPI_GELU_BWD | EPI_COLSUM | (EPI_DROPOUT if ph > 0 else 0), ph
            if not self._reach(b):
                return None
            dq = self._dgrad(dY, lp + '1.fn.net.3.weight', a['dh'], M, f, d, site=8 * i + 4, emit_site=8 * i + 5, pre=g4, emit_only8=self._only8(M),
                             epilogue=epi, aux=L['hpre'],
                             ldaux=f, dropout_p=pdrop, seed=s0 + 3, workspace=a['ws'], colsum_out=G[lp + '1.fn.net.0.bias'])
            g5 = self._grad8(8 * i + 5, a['dh'], M * f, prequant=bool(dq)) if f8 and (self._wants(lp + '1.fn.net.0.weight') or self._reach(b + 1)) else None
            self._wgrad(a['dh'], L['xn2'], lp + '1.fn.net.0.weight', f, d, M, pre=g5, x8=L.get('xn2_8'), xsite=8 * i + 2)
            if not self._reach(b + 1):
                return None
            self._dgrad(a['dh'], lp + '1.fn.net.0.weight', a['dxn'], M, d, f, site=8 * i + 5, pre=g5)
            # LN2 backward; its output feeds the attention out-projection site (mask seed s0+2, bias to_out.0.bias)
            if not self._reach(b + 2):
                return None
            pq6 = self._ln_bwd_fused(a['dxn'], L['x1'], self.P32[lp + '1.norm.weight'], L['mean2'], L['rstd2'], dX, other,
                                     G[lp + '1.norm.weight'], G[lp + '1.norm.bias'], M, a['dxm'], G[lp + '0.fn.to_out.0.bias'], ph, s0 + 2,
                                     q8_site=8 * i + 6)
            dX, other = other, dX  # dX = d(x1)
            dY = a['dxm'] if ph > 0 else dX
            # ---- Attention backward: x1 = drop(attn Wo^T + bo) + x
            g6 = self._grad8(8 * i + 6, dY, M * d, prequant='q8' if pq6 else False) if f8 and (self._wants(lp + '0.fn.to_out.0.weight') or self._reach(b + 3)) else None
            self._wgrad(dY, L['attn'], lp + '0.fn.to_out.0.weight', d, d, M, pre=g6, x8=L.get('attn_8'), xsite=8 * i + 1)
            if not self._reach(b + 3):
                return None
            self._dgrad(dY, lp + '0.fn.to_out.0.weight', a['dattn'], M, d, d, site=8 * i + 6, pre=g6)
            if not self._reach(b + 4):
                return None
            pq7 = self._attention_bwd(L, i, B, ph, s0 + 1)   # fp8_linear: True = it wrote the e5m2 copy of dqkv itself (operand scratch)
            g7 = self._grad8(8 * i + 7, a['dqkv'], M * 3 * d, prequant='q8' if pq7 else False) if f8 and (self._wants(lp + '0.fn.to_qkv.weight') or self._reach(b + 5)) else None
            self._wgrad(a['dqkv'], L['xn1'], lp + '0.fn.to_qkv.weight', 3 * d, d, M, pre=g7, x8=L.get('xn1_8'), xsite=8 * i)
            if not self._reach(b + 5):
                return None
            self._dgrad(a['dqkv'], lp + '0.fn.to_qkv.weight', a['dxn'], M, d, 3 * d, site=8 * i + 7, pre=g7)
            if not self._reach(b + 6):
                return None
            if i > 0:
                # LN1 backward; its output feeds layer i-1's FFN-down site (mask seed of layer i-1, bias net.3.bias)
                lq = f'{pre}transformer.layers.{i - 1}.'
                pq4 = self._ln_bwd_fused(a['dxn'], Xin, self.P32[lp + '0.norm.weight'], L['mean1'], L['rstd1'], dX, other,
                                         G[lp + '0.norm.weight'], G[lp + '0.norm.bias'], M, a['dxm'], G[lq + '1.fn.net.3.bias'], ph,
                                         seed + 100 * i + 4, q8_site=8 * (i - 1) + 4)
                have = True
            else:
                self._ln_bwd(a['dxn'], Xin, self.P32[lp + '0.norm.weight'], L['mean1'], L['rstd1'], dX, other,
                             G[lp + '0.norm.weight'], G[lp + '0.norm.bias'], M)
            dX, other = other, dX
            dY = a['dxm'] if ph > 0 else dX
            # every gradient of layer i is final here (its net.3.bias came from the fused LN1 backward of layer i+1, earlier)
            self._ready(f'layer{i}')
        return dX

    def _cls_block_bwd(self, dXc, dres, out, B, ph, seed):
        """backward of `_cls_block_fwd`: dXc = d(loss)/d(x2) of the CLS rows [B, d].  The FFN, the out-projection and LayerNorm 2 run over B
        rows; the CLS attention backward writes dK / dV of every row and the compact dQ; the K / V products over every row, the Q products
        over the CLS rows.  LayerNorm 1's backward runs over every row as in `_trunk_bwd`, its residual gradient d(x1) being non-zero on
        the CLS rows only (scattered into the zeroed `dres`).  Fills the layer's gradients and releases its bucket; returns (d(x_in) = out,
        the free full slab = dres), or (None, None) when a backward plan (frozen parameters) stopped the pass inside the block"""
        a, W, P, G = self.act, self.W, self.P32, self.G32
        st = stream()
        d, f, N = self.d, self.f, self.T
        M, T, ws = B * N, hip.code(self.dtype), a['ws']
        i = self.Ly - 1
        L = a['layers'][i]
        lp = f'vit.transformer.layers.{i}.'
        s0 = seed + 100 * (i + 1)
        Xin = a['x0'] if i == 0 else a['layers'][i - 1]['x2']
        # ---- FeedForward: x2 = drop(hact W2^T + b2) + x1, the CLS rows
        dY = dXc
        if ph > 0:
            run.ecgvit_dropout_apply_rows(ptr(dXc), ptr(a['cls_dy']), B, d, N, ph, s0 + 4, T, st)
            dY = a['cls_dy']
        self._colsum(dY, d, G[lp + '1.fn.net.3.bias'], B, d)
        if self._wants(lp + '1.fn.net.3.weight'):
            self._gemm(GEMM_TN, dY, a['cls_hact'], G[lp + '1.fn.net.3.weight'], d, f, B, d, f, f, workspace=ws)
        b = self._stage(i, 0)   # frozen parameters: the pass stops before the first input-gradient stage nothing trainable needs
        if not self._reach(b):
            return None, None
        self._gemm(GEMM_NN, dY, W[lp + '1.fn.net.3.weight'], a['cls_dh'], B, f, d, d, f, f, epilogue=EPI_MUL_AUX | EPI_COLSUM, aux=a['cls_hpre'],
                   ldaux=f, workspace=ws, colsum_out=G[lp + '1.fn.net.0.bias'])
        if self._wants(lp + '1.fn.net.0.weight'):
            self._gemm(GEMM_TN, a['cls_dh'], a['cls_xn2'], G[lp + '1.fn.net.0.weight'], f, d, B, f, d, d, workspace=ws)
        if not self._reach(b + 1):
            return None, None
        self._gemm(GEMM_NN, a['cls_dh'], W[lp + '1.fn.net.0.weight'], a['cls_dxn'], B, d, f, f, d, d)
        if not self._reach(b + 2):
            return None, None
        run.ecgvit_layernorm_bwd_fused_rowpitch(ptr(a['cls_dxn']), ptr(a['cls_x1']), ptr(P[lp + '1.norm.weight']), ptr(a['cls_mean2']),
                                                ptr(a['cls_rstd2']), ptr(dXc), ptr(a['cls_dx1']), ptr(G[lp + '1.norm.weight']),
                                                ptr(G[lp + '1.norm.bias']), ptr(ws), B, d, ptr(a['cls_dxm']), ptr(G[lp + '0.fn.to_out.0.bias']),
                                                ph, s0 + 2, N, T, st)
        # ---- Attention: x1 = drop(attn Wo^T + bo) + x, the CLS rows
        dY = a['cls_dxm'] if ph > 0 else a['cls_dx1']
        if self._wants(lp + '0.fn.to_out.0.weight'):
            self._gemm(GEMM_TN, dY, a['cls_attn'], G[lp + '0.fn.to_out.0.weight'], d, d, B, d, d, d, workspace=ws)
        if not self._reach(b + 3):
            return None, None
        self._gemm(GEMM_NN, dY, W[lp + '0.fn.to_out.0.weight'], a['cls_dattn'], B, d, d, d, d, d)
        if not self._reach(b + 4):
            return None, None
        self._attention_cls_bwd(L, B, ph, s0 + 1)
        # to_qkv: dW[K|V] = dKV^T . xn1 over every row, dW[Q] = dQ^T . xn1 over the CLS rows; d(xn1) = dKV . W[K|V] (+ dQ . W[Q] on the CLS rows)
        name = lp + '0.fn.to_qkv.weight'
        if self._wants(name):
            self._gemm(GEMM_TN, a['dqkv'], L['xn1'], G[name], 2 * d, d, M, 3 * d, d, d, workspace=ws, a_off=d, c_off=d * d)
            self._gemm(GEMM_TN, a['cls_dq'], L['xn1'], G[name], d, d, B, d, N * d, d, workspace=ws)
        if not self._reach(b + 5):
            return None, None
        wt = self.WT.get(name)
        if wt is not None and M >= 2048:
            self._gemm(GEMM_NT, a['dqkv'], wt, a['dxn'], M, d, 2 * d, 3 * d, 3 * d, d, a_off=d, b_off=d)
        else:
            self._gemm(GEMM_NN, a['dqkv'], W[name], a['dxn'], M, d, 2 * d, 3 * d, d, d, a_off=d, b_off=d * d)
        self._gemm(GEMM_NN, a['cls_dq'], W[name], a['dxn'], B, d, d, d, d, N * d, epilogue=hip.EPI_ACCUM)
        if not self._reach(b + 6):
            return None, None
        dres.zero_()
        run.ecgvit_scatter_rows(ptr(a['cls_dx1']), ptr(self._cls_rows(B)), ptr(dres), B, N, 1, d, d, d, T, st)
        if i > 0:
            lq = f'vit.transformer.layers.{i - 1}.'
            self._ln_bwd_fused(a['dxn'], Xin, P[lp + '0.norm.weight'], L['mean1'], L['rstd1'], dres, out, G[lp + '0.norm.weight'],
                               G[lp + '0.norm.bias'], M, a['dxm'], G[lq + '1.fn.net.3.bias'], ph, seed + 100 * i + 4)
        else:
            self._ln_bwd(a['dxn'], Xin, P[lp + '0.norm.weight'], L['mean1'], L['rstd1'], dres, out, G[lp + '0.norm.weight'], G[lp + '0.norm.bias'], M)
        self._ready(f'layer{i}')
        return out, dres

    def _cls_rows(self, B):
        """int32 [B, 1] zeros: row 0 of every record (ecgvit_scatter_rows index)"""
        t = getattr(self, '_cls_idx', None)
        if t is None or t.numel() < B or t.device != self.device:
            t = self._cls_idx = torch.zeros(max(B, 1), dtype=torch.int32, device=self.device)
        return t[:B]

    def _attn_bwd_f32(self, L, B, ph, seed):
        d, h, dh, N = self.d, self.h, self.dh, self.T
        a = self.act
        qkv, P, dqkv, dO, dP = L['qkv'], L['probs'], a['dqkv'], a['dattn'], a['dp']
        sq, so, sp = (N * 3 * d, dh), (N * d, dh), (h * N * N, N * N)
        Pd = P
        if ph > 0:
            Pd = a['pd']
            self._drop_apply_f32(P, Pd, B * h * N * N, ph, seed)
        # dV = Pd^T dO
        self._gemm(GEMM_TN, Pd, dO, dqkv, N, dh, N, N, d, 3 * d, batch=(B, h), strideA=sp, strideB=so, strideC=sq, c_off=2 * d)
        # dPd = dO V^T
        self._gemm(GEMM_NT, dO, qkv, dP, N, N, dh, d, 3 * d, N, batch=(B, h), strideA=so, strideB=sq, strideC=sp, b_off=2 * d)
        if ph > 0:
            self._drop_apply_f32(dP, dP, B * h * N * N, ph, seed)
        # dS = P * (dP - rowsum(P dP)) * scale
        run.ecgvit_softmax_bwd_rows(ptr(P), ptr(dP), B * h * N, N, N, self.scale, stream())
        # dQ = dS K ; dK = dS^T Q
        self._gemm(GEMM_NN, dP, qkv, dqkv, N, dh, N, N, 3 * d, 3 * d, batch=(B, h), strideA=sp, strideB=sq, strideC=sq, b_off=d)
        self._gemm(GEMM_TN, dP, qkv, dqkv, N, dh, N, N, 3 * d, 3 * d, batch=(B, h), strideA=sp, strideB=sq, strideC=sq, c_off=d)

    # ---------------------------------------------------------------- attention rollout of a whole batch (f3)
    def attention_rollout_saved(self):
        """The reference visualiser's CLS-to-patch attention map (ecg_vit.py:164-194) of EVERY record of the last supervised forward, from the
        activations it left behind: one `ecgvit_rollout_cls` per layer, one `ecgvit_rollout_colsum` per layer pair (i, i - 1), one
        `ecgvit_rollout_finish`.  No (N, N) matrix is built on the bf16 engine (P is rebuilt tile by tile from qkv / lse); the f32 engine reads
        the probabilities it keeps.  The row layout is the forward's own: packed rows of a ragged batch, per-record token counts, or neither.
        Returns (maps (B, Ly, N_pass - 1) f32 in a fresh tensor, exact zeros past each record's patches and each record scaled to a maximum of
        1, patch counts (B,) int64 on the host)."""
        sv = self.saved
        if sv is None:
            raise RuntimeError('attention rollout needs the activations of a supervised forward')
        if sv.get('masked'):
            raise RuntimeError('the last forward ran the masked objective: its attention rollout is not available')
        if sv.get('cls_only_last'):
            raise RuntimeError('the last forward ran with cls_only_last: its last block computed the CLS query only')
        rg = sv.get('ragged')
        n_tok, tok_off = self._row_tables(sv)
        B, N, h, dh, Ly = sv['B'], self.T, self.h, self.dh, self.Ly
        layers = self.act['layers']
        dev = layers[0]['qkv'].device
        bf16 = self.dtype == torch.bfloat16
        T = hip.code(self.dtype)
        l, st = lib(), stream()
        f32 = torch.float32
        maps = torch.empty(B, Ly, N - 1, dtype=f32, device=dev)
        c, r = torch.empty(B, N, dtype=f32, device=dev), torch.empty(B, N, dtype=f32, device=dev)
        ws = torch.empty(l.ecgvit_rollout_workspace(B, N, h), dtype=torch.uint8, device=dev)

        def src(L):   # (qkv, lse, probs) of a layer as the entry points take them
            return (ptr(L['qkv']), ptr(L['lse']), None) if bf16 else (None, None, ptr(L['probs']))
        for i in range(Ly):
            run.ecgvit_rollout_cls(*src(layers[i]), ptr(c), ptr(n_tok), ptr(tok_off), B, N, h, dh, self.scale, T, st)
            row = c
            if i > 0:
                run.ecgvit_rollout_colsum(*src(layers[i - 1]), ptr(c), ptr(r), ptr(ws), ptr(n_tok), ptr(tok_off), B, N, h, dh, self.scale, T, st)
                row = r
            maps[:, i].copy_(row[:, 1:])   # (a strided device copy: layer i of every record is row[1:])
        run.ecgvit_rollout_finish(ptr(maps), ptr(n_tok), B, Ly, N, st)
        P = self.P
        if rg is not None:
            counts = rg.lengths // P
        elif sv.get('raw') is not None:
            counts = sv['raw'].padded // P
        elif n_tok is not None:
            counts = n_tok.to('cpu', torch.int64) - 1
        else:
            counts = torch.full((B,), N - 1, dtype=torch.int64)
        return maps, counts.to(torch.int64).clone()

    # ---------------------------------------------------------------- per-layer attention probabilities (f3)
    def attention_probs(self, layer):
        """Post-softmax attention of `layer` for the last forward, (B, h, N, N) f32 -- what vit_pytorch's Recorder hooks
        (reference ecg_vit.py:176-194). The f32 path keeps them; the fused bf16 path rebuilds them from its saved qkv + log-sum-exp."""
        if self.saved.get('ragged') is not None:
            raise RuntimeError('the last forward ran on a ragged batch: its attention probabilities are not available')
        if self.saved.get('lengths'):
            raise RuntimeError('the last forward ran with per-record lengths: its attention probabilities are not available')
        B, L = self.saved['B'], self.act['layers'][layer]
        if self.saved.get('cls_only_last') and layer % self.Ly == self.Ly - 1:
            raise RuntimeError('the last forward ran with cls_only_last: its last block computed the CLS query only')
        if self.dtype == torch.float32:
            return L['probs'].view(B, self.h, self.T, self.T)
        out = torch.empty(B, self.h, self.T, self.T, dtype=torch.float32, device=L['qkv'].device)
        run.ecgvit_attention_probs(ptr(L['qkv']), ptr(L['lse']), ptr(out), B, self.T, self.h, self.dh, self.scale, hip.BF16, stream())
        return out
