"""
Input transforms of the reference data pipeline, FUSED into the patch-embed load.

Reference: `ecg_transformer/preprocess/transform.py` -- `Normalize` (:18-35), `TimeEndPad` (:140-154), `TimeOut` (:175-185) --
composed per record on the host in `get_ptbxl_dataset` (`preprocess/ptb_dataset.py:132-149`: Normalize, TimeEndPad(patch_size),
and TimeOut for the training split only).  Here the raw `(B, 12, L_raw)` batch goes to the device as is and the three
transforms are applied inside `ecgvit_patch_gather_transform` while the samples stream through LDS: no extra read+write of
the input tensor, no per-record numpy work on the host.  Only the TimeOut span is drawn on the host (two int32 per record), with
the same torch RNG calls the reference makes, so a seeded run masks the same spans.

`per_record=True`: the records need not share a raw length.  `lengths[b]` is then record b's RAW sample count l_b (any integer >= 1), in a
padded `(B, 12, W)` batch (W >= max l_b; samples at or past l_b are never read) or a ragged `(12, S_raw)` one (the raw records
concatenated).  Record b is transformed as the reference transforms it alone -- normalised, zero-padded in normalised space to
`padded_length(l_b)`, TimeOut drawn on that padded length (`draw_timeout_records`) -- inside `ecgvit_patch_gather_transform_varlen`, and
counts `padded_length(l_b) / patch_size` patches from there on.  Without `per_record` (the default) per-record lengths and ragged batches
are refused as before: the rectangular kernel pads every record to one length.
"""
import math

import numpy as np
import torch

from . import hip
from .hip import run, ptr, stream
from .records import DeviceTables, check_device_store, chunk_step, host_chunks, select_records


class FusedInputTransform:
    def __init__(self, mean, std, patch_size, timeout=False, timeout_scale=(0.0, 0.5), per_record=False):
        mean = torch.as_tensor(mean, dtype=torch.float32)
        std = torch.as_tensor(std, dtype=torch.float32)
        assert mean.numel() == 12 and std.numel() == 12   # transform.py:26
        self.mean, self.inv_std = mean.contiguous(), (1.0 / std).contiguous()
        self.k = int(patch_size)
        self.timeout = bool(timeout)
        self.per_record = bool(per_record)
        self.sampler = torch.distributions.Uniform(low=timeout_scale[0], high=timeout_scale[1])   # transform.py:178
        self._dev = None

    def padded_length(self, l_raw: int) -> int:
        """TimeEndPad: n_pad = k - (l % k)  -- a FULL extra patch when l is already a multiple of k (transform.py:150)"""
        return l_raw + (self.k - (l_raw % self.k))

    def draw_timeout(self, batch: int, l_pad: int, device):
        """per record: r ~ U(lo, hi); l_crop = round(r * L); start = randint(L - l_crop)  (transform.py:180-183), as int32 tensors"""
        starts, lens = [], []
        for _ in range(batch):
            r = self.sampler.sample().item()
            l_crop = round(r * l_pad)
            start = torch.randint(high=l_pad - l_crop, size=(1,)).item()
            starts.append(start)
            lens.append(l_crop)
        return (torch.tensor(starts, dtype=torch.int32, device=device), torch.tensor(lens, dtype=torch.int32, device=device))

    def draw_timeout_records(self, padded_lengths):
        """`draw_timeout` for records of unequal length: per record, in batch order, the reference's two RNG calls on that record's own padded
        length (transform.py:180-183) -> (2, B) int32 HOST tensor [starts; lengths] (the engine stages it through pinned memory).  Drawing a
        batch range by range, in order, consumes the generator exactly as drawing it whole."""
        out = torch.empty(2, len(padded_lengths), dtype=torch.int32)
        for b, l_pad in enumerate(int(v) for v in padded_lengths):
            r = self.sampler.sample().item()
            l_crop = round(r * l_pad)
            out[0, b] = torch.randint(high=l_pad - l_crop, size=(1,)).item()
            out[1, b] = l_crop
        return out

    def device_stats(self, device):
        if self._dev is None or self._dev[0].device != device:
            self._dev = (self.mean.to(device), self.inv_std.to(device))
        return self._dev


# ------------------------------------------------------------------------------------------------------------------------------------
# Fitting the statistics: the reference's DynamicNormalize (preprocess/transform.py:38-137), on the device
# ------------------------------------------------------------------------------------------------------------------------------------
SCHEMES = ('global', 'std', 'norm', 'none')
MAX_TARGETS = hip.FIT_TARGETS   # order statistics per lead of one fit


def parse_normalize(normalize):
    """The reference's `NormArg` -> [(scheme, arg or None), ...], by the reference's own rules (transform.py:119-124, :53-65): a scheme name, a
    (scheme, arg) TUPLE, or a sequence whose first element is a tuple, of tuples and names.  arg defaults to 1 for 'std' and 2 for 'norm' and
    is dropped for 'global' / 'none'.  ValueError where the reference asserts (unknown scheme, non-numeric arg, a pair of the wrong length)
    and, beyond it, for an arg <= 0 or non-finite: the divisor of every stage must be positive."""
    if isinstance(normalize, str) or (isinstance(normalize, (tuple, list)) and len(normalize) > 0 and not isinstance(normalize[0], tuple)):
        norm_args = [normalize]
    else:
        norm_args = normalize
    if not isinstance(norm_args, (tuple, list)) or len(norm_args) == 0:
        raise ValueError(f'normalize: a scheme name, a (scheme, arg) tuple or a sequence of them is expected, got {normalize!r}')
    out = []
    for pr in norm_args:
        pr = pr if isinstance(pr, tuple) else (pr,)
        if len(pr) not in (1, 2):
            raise ValueError(f'normalize: {pr!r} is not (scheme,) or (scheme, arg)')
        scheme, arg = pr[0], (pr[1] if len(pr) == 2 else None)
        if not isinstance(scheme, str) or scheme not in SCHEMES:
            raise ValueError(f'normalize: unknown scheme {scheme!r} (one of {SCHEMES})')
        if scheme in ('std', 'norm'):
            if arg is None:
                arg = 1 if scheme == 'std' else 2
            elif not isinstance(arg, (float, int)):
                raise ValueError(f'normalize: the arg of {scheme!r} must be a number, got {arg!r}')
            if not (math.isfinite(arg) and arg > 0):
                raise ValueError(f'normalize: the arg of {scheme!r} must be positive and finite, got {arg!r}')
        else:
            arg = None
        out.append((scheme, arg))
    return out


def norm_percentile(arg):
    """p = 100 Phi(arg) in f64 (the reference: scipy.stats.norm().cdf(arg) * 100, transform.py:79)"""
    return 100.0 * (0.5 * (1.0 + math.erf(float(arg) / math.sqrt(2.0))))


def percentile_targets(q, n):
    """np.nanpercentile's default ('linear') for percentile q over n valid samples: the two neighbouring 0-based ranks of the virtual index
    (n - 1) q / 100 and the interpolation weight, in f64 as numpy computes them -> (lo, hi, gamma)"""
    vi = (n - 1) * (q / 100.0)
    lo = int(math.floor(vi))
    lo = min(max(lo, 0), n - 1)
    hi = min(lo + 1, n - 1)
    return lo, hi, vi - lo


def lerp(a, b, t):
    """numpy's _lerp (lib/_function_base_impl.py) on f64 scalars"""
    d = b - a
    return b - d * (1.0 - t) if t >= 0.5 else a + d * t


class RawStats:
    """What one sweep of the data gives, per lead (f64 / exact): count, nan_count, mean, std (ddof 0; None unless a 'std' stage asked for them),
    and `order`: {rank-spec: (12,) f64} with rank-specs 'min', 'max' and ('q', percentile) -- the already interpolated percentile.
    `ranks` / `values`: the (12, T) 0-based ranks selected on the device and the (12, T) f32 order statistics found there."""

    def __init__(self, count, nan_count, mean=None, std=None, order=None, ranks=None, values=None):
        self.count, self.nan_count, self.mean, self.std = count, nan_count, mean, std
        self.order, self.ranks, self.values = order or {}, ranks, values


class NormStage:
    def __init__(self, scheme, arg, norm_meta):
        self.scheme, self.arg, self.norm_meta = scheme, arg, norm_meta   # norm_meta: two (12,) f32 arrays, None for 'none'

    def __repr__(self):
        return f'<NormStage {self.scheme} arg={self.arg}>'


def plan_order_stats(stages):
    """the raw order statistics the stages need, in table order: 'min', 'max' if any stage is 'global', then ('q', 100 - p), ('q', p) per
    distinct 'norm' arg"""
    specs = []
    if any(s == 'global' for s, _ in stages):
        specs += ['min', 'max']
    for s, a in stages:
        if s == 'norm':
            p = norm_percentile(a)
            for spec in (('q', 100.0 - p), ('q', p)):
                if spec not in specs:
                    specs.append(spec)
    return specs


def compose_stages(stages, raw, lead_names=None):
    """The stage-composition algebra, on the host in f64.  Stage j of the reference is fitted on the output of stages < j, each a per-lead
    affine map x -> (x - sub) / div with div > 0 taken from that stage's F32-ROUNDED norm_meta (transform.py:86-100).  Under such a map the
    mean, minimum, maximum and every percentile follow the map and the standard deviation is divided by div, so stage j's statistics are
    those of the raw samples (`raw`: RawStats) pushed through the composite (A, D) of the earlier stages: x_j = (x - A) / D, and after a stage
    with (sub, div): A += sub D, D *= div.  -> ([NormStage], mean (12,) f32, std (12,) f32) with (x - mean) / std the whole chain.
    ValueError, naming the lead, where a divisor is not positive and finite (the reference hands back inf / NaN there)."""
    C = len(raw.count)
    A, D = np.zeros(C, np.float64), np.ones(C, np.float64)
    out = []
    for scheme, arg in stages:
        if scheme == 'none':
            out.append(NormStage(scheme, None, None))
            continue
        if scheme == 'global':
            a, b = (raw.order['min'] - A) / D, (raw.order['max'] - A) / D
        elif scheme == 'norm':
            p = norm_percentile(arg)
            a, b = (raw.order[('q', 100.0 - p)] - A) / D, (raw.order[('q', p)] - A) / D
        else:
            a, b = (raw.mean - A) / D, raw.std / D * arg
        a, b = a.astype(np.float32), b.astype(np.float32)                   # transform.py:85-86
        with np.errstate(invalid='ignore', over='ignore'):
            sub, div = (a, b) if scheme == 'std' else (a, b - a)            # f32 - f32 = f32, as the reference's `ma - mi`
        bad = ~(np.isfinite(div) & (div > 0) & np.isfinite(sub))
        if bad.any():
            c = int(np.flatnonzero(bad)[0])
            name = lead_names[c] if lead_names is not None else c
            raise ValueError(f'lead {name} has no finite spread under {scheme!r} (sub {sub[c]!r}, div {div[c]!r}): the reference would normalise it to inf / NaN')
        out.append(NormStage(scheme, arg, (a, b)))
        A = A + sub.astype(np.float64) * D
        D = D * div.astype(np.float64)
    return out, A.astype(np.float32), D.astype(np.float32)


class DynamicNormalizeFit:
    """Result of `fit_dynamic_normalize`: `.stages` (per stage scheme, arg and the reference's `norm_meta` as two (12,) f32 arrays), `.mean` /
    `.std` ((12,) f32: the composite affine, (x - mean) / std is the whole chain), `.count` / `.nan_count` per lead, `.raw` (RawStats)."""

    def __init__(self, stages, mean, std, raw):
        self.stages, self.mean, self.std, self.raw = stages, mean, std, raw
        self.count, self.nan_count = raw.count, raw.nan_count

    def to_transform(self, patch_size, timeout=False, per_record=False):
        return FusedInputTransform(self.mean, self.std, patch_size, timeout=timeout, per_record=per_record)

    def __repr__(self):
        return f'<DynamicNormalizeFit stages={self.stages}>'


def _key_to_f32(keys):
    keys = np.asarray(keys, dtype=np.uint32)
    bits = np.where(keys & np.uint32(0x80000000), keys ^ np.uint32(0x80000000), ~keys)
    return bits.astype(np.uint32).view(np.float32)


class _DeviceSweep:
    """the launches of one pass over the selected records: in place on a device store, or chunk by chunk through a staging buffer for a host one"""

    def __init__(self, records, s, chunk_records, device):
        if isinstance(records, torch.Tensor) and records.is_cuda:
            check_device_store(records, 'a device store')
            tab, R = DeviceTables.of(records, s), s.R
            self.chunks = lambda: [tab]
        else:
            host = records.numpy() if isinstance(records, torch.Tensor) else records
            R = min(chunk_step(s, chunk_records), s.R)
            self.chunks = lambda: (DeviceTables(torch.from_numpy(buf).to(device), off, lens, stride)
                                   for buf, off, lens, stride, _ in host_chunks(host, s, chunk_records))
        self.ws = torch.empty(max(8, hip.lib().ecgvit_fit_workspace(R, s.C) // 8), dtype=torch.float64, device=device)

    def run(self, *launches):
        """every launch of `launches` (callables of a chunk's DeviceTables) over every chunk, the chunks uploaded once per call"""
        for tab in self.chunks():
            for fn in launches:
                fn(tab)


def device_raw_stats(records, specs, want_std, offsets=None, idxs=None, chunk_records=None, device=None):
    """One sweep of the per-lead raw statistics on the device -> RawStats.  specs: `plan_order_stats` rank-specs; want_std: the second moments
    pass.  Passes: counts + sum together with the top-digit histogram; the squared deviations together with the second digit; the last two
    digits -- a host store is uploaded four times (twice without order statistics), a device store is read in place."""
    s = select_records(records, offsets, idxs)
    C = s.C
    if len(specs) and 2 * len(specs) > MAX_TARGETS + (2 if 'min' in specs else 0):
        raise ValueError(f'{len(specs)} order statistics per lead need more than {MAX_TARGETS} ranks: fit fewer distinct percentiles at once')
    if isinstance(records, torch.Tensor) and records.is_cuda:
        device = records.device
    else:
        device = torch.device(device if device is not None else 'cuda')
        if device.type != 'cuda' or not torch.cuda.is_available():
            raise RuntimeError('fit_dynamic_normalize runs on the device (no CPU fallback exists)')
    with torch.cuda.device(device):
        sweep = _DeviceSweep(records, s, chunk_records, device)
        state = torch.zeros(C, 4, dtype=torch.int64, device=device)
        hist = torch.zeros(4, C, hip.FIT_TARGETS, hip.FIT_BINS, dtype=torch.int64, device=device)
        selt = torch.zeros(C, hip.FIT_TARGETS, 4, dtype=torch.int64, device=device)
        ws = sweep.ws

        def moments(mean):
            return lambda t: run.ecgvit_fit_moments(ptr(t.x), ptr(t.src_off), t.stride, ptr(t.raw_len), t.R, C, ptr(mean), ptr(ws), ptr(state), stream())

        def histogram(p, T):
            return lambda t: run.ecgvit_fit_histogram(ptr(t.x), ptr(t.src_off), t.stride, ptr(t.raw_len), t.R, C, ptr(selt), T, p, ptr(hist[p]), stream())

        sweep.run(moments(None), *([histogram(0, 0)] if specs else []))
        st = state.cpu().numpy()
        count, nan_count = st[:, 0].copy(), st[:, 1].copy()
        if (count == 0).any():
            c = int(np.flatnonzero(count == 0)[0])
            raise ValueError(f'lead {c} has no finite spread: every selected sample is NaN')
        mean = st[:, 2].copy().view(np.float64) / count
        raw = RawStats(count, nan_count, mean=mean)
        # the rank table: per spec the two neighbouring ranks ('min' / 'max': one each)
        ranks, plan = [], []
        for spec in specs:
            if spec == 'min':
                plan.append((len(ranks), None)); ranks.append(np.zeros(C, np.int64))
            elif spec == 'max':
                plan.append((len(ranks), None)); ranks.append(count - 1)
            else:
                tg = [percentile_targets(spec[1], int(k)) for k in count]
                plan.append((len(ranks), np.array([t[2] for t in tg])))
                ranks += [np.array([t[0] for t in tg], np.int64), np.array([t[1] for t in tg], np.int64)]
        T = len(ranks)
        mean_dev = torch.from_numpy(mean).to(device) if want_std else None
        if T:
            host_sel = np.zeros((C, hip.FIT_TARGETS, 4), np.int64)
            host_sel[:, :T, 0] = np.stack(ranks, 1)
            selt.copy_(torch.from_numpy(host_sel))
            run.ecgvit_fit_select(ptr(hist[0]), ptr(selt), C, T, 0, stream())
            for p in (1, 2, 3):
                sweep.run(histogram(p, T), *([moments(mean_dev)] if (want_std and p == 1) else []))
                run.ecgvit_fit_select(ptr(hist[p]), ptr(selt), C, T, p, stream())
            out = selt.cpu().numpy()
            if (out[:, :T, 3] == 0).any():
                raise RuntimeError('radix select: a rank lies past the count of its lead')
            vals = _key_to_f32(out[:, :T, 1].astype(np.uint64).astype(np.uint32))
            raw.ranks, raw.values = np.stack(ranks, 1), vals
            v64 = vals.astype(np.float64)
            for spec, (j, gamma) in zip(specs, plan):
                raw.order[spec] = v64[:, j] if gamma is None else np.array([lerp(v64[c, j], v64[c, j + 1], gamma[c]) for c in range(C)])
        elif want_std:
            sweep.run(moments(mean_dev))
        if want_std:
            raw.std = np.sqrt(state.cpu().numpy()[:, 3].copy().view(np.float64) / count)
    return raw


def fit_dynamic_normalize(records, normalize=(('norm', 3), ('std', 1)), offsets=None, idxs=None, chunk_records=None):
    """The reference's `DynamicNormalize(sig, normalize)` (preprocess/transform.py:108-137; fitted on the training split at util/config.py:296-308)
    with the sweeps over the data done by HIP kernels on the device: per lead the count, the NaN count, the two-pass f64 mean / standard
    deviation and EXACT order statistics by radix select, NaN samples left out as np.nanmean / nanstd / nanmin / nanmax / nanpercentile leave
    them out -> `DynamicNormalizeFit`; `.to_transform(patch_size, ...)` is the `FusedInputTransform` of the whole chain.

    records: (n, 12, L), or a ragged (12, S_total) store with `offsets` (the (n + 1,) table `RaggedDeviceFeeder` takes).  A float32 device
    tensor is read in place -- `idxs` (record indices, e.g. the training fold) only builds an address table, nothing is copied.  A host
    array / memmap / tensor of any float type is moved to the device `chunk_records` records at a time (rounded to float32 as the feeders round),
    once per pass.  A ragged corpus has no rectangle: its statistics are those of the records padded to the longest with NaN.
    normalize: what the reference's `NormArg` accepts (`parse_normalize`).  A sequence of stages costs ONE sweep: every stage is a per-lead
    affine map, so its statistics follow from the raw ones (`compose_stages`).
    A lead with no finite spread -- all NaN, constant under 'std', max == min or equal percentiles -- raises ValueError naming the lead; the
    reference hands back a transform that maps it to inf / NaN."""
    stages = parse_normalize(normalize)
    specs = plan_order_stats(stages)
    raw = device_raw_stats(records, specs, any(s == 'std' for s, _ in stages), offsets=offsets, idxs=idxs, chunk_records=chunk_records)
    st, mean, std = compose_stages(stages, raw)
    return DynamicNormalizeFit(st, mean, std, raw)
