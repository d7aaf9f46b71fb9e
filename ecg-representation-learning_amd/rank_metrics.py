"""
Rank-based AUROC and bootstrap confidence intervals on the device (`include/ecgvit_hip_rank.h` states the contract, `csrc/rank_metrics.hip`
holds the kernels).

`metrics.eval_counts` gets a class's AUROC from all (positive, negative) pairs, O(n^2 K).  Here every class column is sorted once (a stable
radix sort of (key, record index)); a weighted prefix sum over the sorted order then gives the very integer the all-pairs kernel leaves in its
pair slot, and, with a replicate's multiplicities as the weights, the integer behind `roc_auc_score(sample_weight=multiplicities)` -- which is
the reference's `get_accuracy(preds[idx], labels[idx])` on the resample `idx`.  The device returns (R, K) triples (num2, wp, wn) of exact
integers; the divisions and the percentiles are host f64, as in `DeviceCounts.result`.

A replicate holding only one label value of a class is invalid for that class (the reference's own `msk_2_class` rule, util/train.py:29, applied
to the resample): NaN in `per_class_auc`, left out of the replicate's macro average.  No class is redrawn and nothing is stratified.
"""
import collections
import warnings

import numpy as np
import torch

from . import rank_abi
from .hip import ptr, stream
from .metrics import DeviceCounts
from . import hip

__all__ = ['RankedScores', 'BootstrapResult', 'rank_scores', 'auroc_counts', 'bootstrap_auc', 'draws', 'multiplicities']

_M64 = (1 << 64) - 1
_GAMMA = 0x9E3779B97F4A7C15
DEFAULT_WORKSPACE_BYTES = 256 << 20   # multiplicities of one chunk of replicates


def _check_pair(scores, labels):
    """every refusal of a (scores, labels) pair, the device asked for last -> (n, K)"""
    for t, name in ((scores, 'scores'), (labels, 'labels')):
        if not isinstance(t, torch.Tensor):
            raise ValueError(f'{name} must be a torch tensor, got {type(t).__name__}')
        if t.dtype != torch.float32:
            raise ValueError(f'{name} must be float32, got {t.dtype}')
        if t.dim() != 2:
            raise ValueError(f'{name} must be (n, K), got {tuple(t.shape)}')
    if scores.shape != labels.shape:
        raise ValueError(f'labels must be {tuple(scores.shape)} as scores, got {tuple(labels.shape)}')
    n, K = scores.shape
    if n < 1 or K < 1:
        raise ValueError(f'scores must hold at least one record and one class, got {tuple(scores.shape)}')
    for t, name in ((scores, 'scores'), (labels, 'labels')):
        if t.stride(1) != 1 and K > 1 or (n > 1 and t.stride(0) < K):
            raise ValueError(f'{name} must have contiguous rows')
    if n > rank_abi.MAX_ROWS:
        raise ValueError(f'scores: n = {n} exceeds {rank_abi.MAX_ROWS}')
    if K > rank_abi.MAX_CLASSES:
        raise ValueError(f'scores: K = {K} exceeds {rank_abi.MAX_CLASSES}')
    for t, name in ((scores, 'scores'), (labels, 'labels')):
        if not t.is_cuda:
            raise ValueError(f'{name} must be a device tensor (rank metrics run on the device: no CPU fallback exists)')
    return n, K


def _pitch(t):
    return t.stride(0) if t.shape[0] > 1 else t.shape[1]


def pad4(replicates):
    """the pitch of the record-major multiplicities: a wave of the walks takes four replicates of a record in one load"""
    return (replicates + 3) // 4 * 4


class RankedScores:
    """The sorted order of every class column: `packed` (K, n) int32 words (record index | label bit << 30 | last-of-tie-group bit << 31) and
    `first_nan` (K,) int32, on the device."""

    def __init__(self, packed, first_nan, scores, labels, from_logits):
        self.packed, self.first_nan, self.from_logits = packed, first_nan, bool(from_logits)
        self.K, self.n = packed.shape
        self.scores, self.labels = scores, labels

    def order(self, c):
        """record indices of class c under (key ascending, record index ascending): (n,) int64 on the device"""
        return self.records(self.packed[c])

    @staticmethod
    def records(words):
        """packed words -> the record indices they hold (int64)"""
        return (words & 0x3FFFFFFF).long()

    def _walk(self, mult, R, out, pairs=None):
        rank_abi.run.ecgvit_rank_walk(ptr(self.packed), ptr(self.first_nan), self.n, self.K, ptr(mult), R, ptr(out), ptr(pairs), stream())


def rank_scores(scores, labels, from_logits=False) -> RankedScores:
    """Sort every class column once (asynchronous).  scores / labels: (n, K) f32 device tensors with contiguous rows."""
    n, K = _check_pair(scores, labels)
    nbytes = rank_abi.lib().ecgvit_rank_workspace(n, K, 0)
    if nbytes <= 0:
        raise ValueError(f'scores: unsupported shape {(n, K)}')
    ws = torch.empty(nbytes, dtype=torch.uint8, device=scores.device)
    packed = torch.empty(K, n, dtype=torch.int32, device=scores.device)
    first_nan = torch.empty(K, dtype=torch.int32, device=scores.device)
    rank_abi.run.ecgvit_rank_sort(ptr(scores), _pitch(scores), ptr(labels), _pitch(labels), n, K, int(bool(from_logits)), ptr(packed), ptr(first_nan),
                                  ptr(ws), stream())
    return RankedScores(packed, first_nan, scores, labels, from_logits)


def _counts(ranked, id2code):
    """the 4 + 2K layout of `eval_counts`: the confusion slots from `ecgvit_eval_counts` without its all-pairs kernel, the pair slots from the walk"""
    s, y, n, K = ranked.scores, ranked.labels, ranked.n, ranked.K
    counts = torch.empty(4 + 2 * K, dtype=torch.int64, device=s.device)
    hip.run.ecgvit_eval_counts(ptr(s), _pitch(s), ptr(y), _pitch(y), n, K, int(ranked.from_logits), 0, ptr(counts), stream())
    triples = torch.empty(1, K, 3, dtype=torch.int64, device=s.device)
    ranked._walk(None, 1, triples, counts[4 + K:])
    h = DeviceCounts(counts, n, K, True, id2code)
    h._keep = (s, y, ranked, triples)
    return h


def auroc_counts(scores, labels, from_logits=False, id2code=None) -> DeviceCounts:
    """`eval_counts(..., return_auc=True)` by the rank route: the same 4 + 2K integers, so `.result()` is the same dict."""
    return _counts(rank_scores(scores, labels, from_logits), id2code)


# ---- the generator, restated on the host (include/ecgvit_hip_rank.h) ---------------------------------------------------------------------
def _mix(z):
    z = np.asarray(z, dtype=np.uint64)
    z = z ^ (z >> np.uint64(30))
    z = z * np.uint64(0xBF58476D1CE4E5B9)
    z = z ^ (z >> np.uint64(27))
    z = z * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def draws(seed, replicate, n):
    """the n draws of replicate `replicate` under `seed`, as the device makes them: (n,) int64 in [0, n)"""
    with np.errstate(over='ignore'):
        key = _mix(np.uint64((int(seed) + _GAMMA * (int(replicate) + 1)) & _M64))
        u = _mix(key + np.uint64(_GAMMA) * np.arange(1, n + 1, dtype=np.uint64))
        hi, lo = u >> np.uint64(32), u & np.uint64(0xFFFFFFFF)
        return ((hi * np.uint64(n) + ((lo * np.uint64(n)) >> np.uint64(32))) >> np.uint64(32)).astype(np.int64)   # (u n) >> 64 for n < 2^32


def multiplicities(seed, replicate, n):
    return np.bincount(draws(seed, replicate, n), minlength=n).astype(np.int64)


# ---- replicates ---------------------------------------------------------------------------------------------------------------------------
def valid_classes(counts):
    """(..., K, slots) int64 of either walk, slots 1 and 2 holding wp and wn -> (..., K) bool: the class holds a positive and a negative of
    non-zero weight"""
    return (counts[..., 1] > 0) & (counts[..., 2] > 0)


class ReplicateResult:
    """What the results of every walk share.  `point`: the dict of the whole set.  `n_valid` (K,) replicates in which the class is valid.
    `n`, `n_boot`, `seed` (None under indices), `source` (`draw_source`) and `chunk`: the draws' record, which the bootstrap driver fills.
    A subclass sets `per_class_<metric>` (R, K) f64, NaN where invalid, and `macro_<metric>` (R,) = `_macro` of it, for each of its metrics."""

    def __init__(self, point, counts, id2code=None):
        self.point, self.id2code = point, id2code
        self.n = self.n_boot = self.seed = self.source = self.chunk = None
        self.valid = valid_classes(counts)
        self.n_valid = self.valid.sum(axis=0)

    def _macro(self, per):
        """the mean over each replicate's valid classes (NaN: none)"""
        cnt = self.valid.sum(axis=-1)
        with np.errstate(divide='ignore', invalid='ignore'):
            return np.where(cnt > 0, np.where(self.valid, per, 0.0).sum(axis=-1) / cnt, np.nan)

    def _drawn(self, n, R, chunk, seed, indices):
        self.chunk, self.n, self.n_boot, self.seed, self.source = chunk, n, R, (seed if indices is None else None), draw_source(seed, indices)
        return self

    @staticmethod
    def _alpha(alpha):
        if isinstance(alpha, bool) or not isinstance(alpha, (int, float)) or not 0 < alpha < 1:
            raise ValueError(f'alpha must be in (0, 1), got {alpha!r}')
        return [100.0 * alpha / 2, 100.0 * (1 - alpha / 2)]

    @staticmethod
    def percentiles(values, alpha, axis=None):
        """the alpha / 2 and 1 - alpha / 2 percentiles of the values that are not NaN (NaN, without a warning, where none is)"""
        q = ReplicateResult._alpha(alpha)
        with warnings.catch_warnings():
            warnings.simplefilter('ignore', RuntimeWarning)
            return np.nanpercentile(values, q, axis=axis)

    def _ci(self, metric, alpha):
        lo, hi = self.percentiles(getattr(self, 'macro_' + metric), alpha)
        return float(lo), float(hi)

    def _class_ci(self, metric, alpha):
        return self.percentiles(getattr(self, 'per_class_' + metric), alpha, axis=0).T.copy()


class BootstrapResult(ReplicateResult):
    """`point`: the `get_accuracy` dict of the whole set.  `triples`: (R, K, 3) int64 (num2, wp, wn) as the device left them.
    `per_class_auc` (R, K) f64, NaN where the replicate holds one label value only; `macro_auc` (R,) the mean over the replicate's valid classes
    (NaN: none); `n_valid` (K,) replicates in which the class is valid."""

    def __init__(self, point, triples, id2code=None):
        super().__init__(point, triples, id2code)
        self.triples = triples
        num2, wp, wn = (triples[..., i].astype(np.float64) for i in range(3))
        with np.errstate(divide='ignore', invalid='ignore'):
            self.per_class_auc = np.where(self.valid, num2 / (2.0 * wp * wn), np.nan)
        self.macro_auc = self._macro(self.per_class_auc)

    def ci(self, alpha=0.05):
        """(lo, hi) of the macro AUROC: the alpha / 2 and 1 - alpha / 2 percentiles of the replicates that have a valid class"""
        return self._ci('auc', alpha)

    def class_ci(self, alpha=0.05):
        """(K, 2) per-class (lo, hi) over the replicates in which the class is valid; NaN for a class that never is"""
        return self._class_ci('auc', alpha)


def intervals(res, metric='auc', alpha=0.05):
    """(macro (lo, hi), {class key of the point estimate: (lo, hi)} or None) of one metric of a result, for the evaluators' dicts"""
    per = res.point[f'per_class_{metric}']
    if per is None:
        return res._ci(metric, alpha), None
    cc = res._class_ci(metric, alpha)
    cols = [k for k in range(cc.shape[0]) if (res.id2code[k] if res.id2code is not None else k) in per]
    return res._ci(metric, alpha), {key: (float(cc[k, 0]), float(cc[k, 1])) for key, k in zip(per, cols)}


def _check_indices(indices, n):
    """(R, n) integer draws, a torch tensor (host or device) or a numpy array -> the tensor; out-of-range draws are met here for a host array"""
    if isinstance(indices, np.ndarray):
        indices = torch.from_numpy(np.ascontiguousarray(indices))
    if not isinstance(indices, torch.Tensor) or indices.dtype not in (torch.int64, torch.int32):
        raise ValueError('indices must be an (R, n) int64 or int32 tensor or array')
    if indices.dim() != 2 or indices.shape[1] != n or indices.shape[0] < 1:
        raise ValueError(f'indices must be (R, {n}) with R >= 1, got {tuple(indices.shape)}')
    if not indices.is_cuda and indices.device.type == 'cpu' and (int(indices.min()) < 0 or int(indices.max()) >= n):
        raise ValueError(f'indices must lie in [0, {n}), got {int(indices.min())} .. {int(indices.max())}')
    return indices


def _plan(scores, labels, n_boot, seed, indices, workspace_bytes):
    """every refusal of a bootstrap call, the device asked for last -> (n, K, R, replicates per chunk, indices as a tensor or None)"""
    if isinstance(n_boot, bool) or not isinstance(n_boot, int) or n_boot < 1:
        raise ValueError(f'n_boot must be an integer >= 1, got {n_boot!r}')
    if isinstance(seed, bool) or not isinstance(seed, int) or not 0 <= seed <= _M64:
        raise ValueError(f'seed must be an integer in [0, 2^64), got {seed!r}')
    if indices is not None and seed != 0:
        raise ValueError('seed and indices are both given: the draws come from one or the other')
    if workspace_bytes is not None and (isinstance(workspace_bytes, bool) or not isinstance(workspace_bytes, int) or workspace_bytes < 1):
        raise ValueError(f'workspace_bytes must be a positive integer, got {workspace_bytes!r}')
    if isinstance(scores, torch.Tensor) and scores.dim() == 2 and indices is not None:
        indices = _check_indices(indices, scores.shape[0])
    R = n_boot if indices is None or not isinstance(indices, torch.Tensor) else indices.shape[0]
    if R > rank_abi.MAX_REPLICATES:
        raise ValueError(f'n_boot = {R} exceeds {rank_abi.MAX_REPLICATES}')
    n, K = _check_pair(scores, labels)
    quad = rank_abi.lib().ecgvit_rank_workspace(n, K, 4)   # the multiplicities are held four replicates wide
    chunk = max(1, min(R, (DEFAULT_WORKSPACE_BYTES if workspace_bytes is None else workspace_bytes) // quad * 4))
    return n, K, R, chunk, indices


def draw_source(seed, indices):
    """what the replicates of a result were drawn from: ('seed', seed), or ('indices', R, a wrapping int64 checksum of the draws) -- two results
    compare replicate by replicate only when these are equal"""
    if indices is None:
        return ('seed', int(seed))
    flat = indices.to(torch.int64).reshape(-1)
    return ('indices', int(indices.shape[0]), int((flat * torch.arange(1, flat.numel() + 1, dtype=torch.int64, device=flat.device)).sum()))


# A quantity on the sorted order, as the bootstrap driver and the evaluators' key assembly take it.  counts(ranked, id2code): the handle of the
# point estimate; walk(ranked, mult, R, out): one launch over R replicates; slots: integers per (replicate, class); result: the ReplicateResult;
# metrics: its `macro_` / `per_class_` names; key: the result's name under an evaluator's predictions; max_rows: n at which the route refuses.
Route = collections.namedtuple('Route', 'counts walk slots result metrics key max_rows')
AUC = Route(_counts, RankedScores._walk, 3, BootstrapResult, ('auc',), 'bootstrap', None)


def _bootstrap(routes, scores, labels, n_boot=1000, seed=0, indices=None, from_logits=False, id2code=None, workspace_bytes=None):
    """The bootstrap of every route of `routes` on one sort and one set of draws: a point estimate per route, then one multiplicity fill per chunk
    of replicates and each route's walk over it -> [the route's result]"""
    n, K, R, chunk, indices = _plan(scores, labels, n_boot, seed, indices, workspace_bytes)
    for route in routes:
        if route.max_rows is not None and n >= route.max_rows:
            raise ValueError(f'scores: n = {n}, the weights of a replicate must sum to less than {route.max_rows}')
    ranked, dev = rank_scores(scores, labels, from_logits), scores.device
    points = [route.counts(ranked, id2code) for route in routes]
    outs = [torch.empty(R, K, route.slots, dtype=torch.int64, device=dev) for route in routes]
    mult = torch.empty(n, pad4(chunk), dtype=torch.int32, device=dev)   # record-major; a shorter last chunk uses its head
    for r0 in range(0, R, chunk):
        rows = min(chunk, R - r0)
        if indices is None:
            rank_abi.run.ecgvit_rank_multiplicities_seeded(seed, r0, rows, n, ptr(mult), stream())
        else:
            idx = indices[r0:r0 + rows].to(device=dev, dtype=torch.int64).contiguous()
            rank_abi.run.ecgvit_rank_multiplicities(ptr(idx), n, rows, n, ptr(mult), stream())
        for route, out in zip(routes, outs):
            route.walk(ranked, mult, rows, out[r0:r0 + rows])
    return [route.result(point.result(), out.cpu().numpy(), id2code)._drawn(n, R, chunk, seed, indices) for route, point, out in zip(routes, points, outs)]


def bootstrap_auc(scores, labels, n_boot=1000, seed=0, indices=None, from_logits=False, id2code=None, workspace_bytes=None) -> BootstrapResult:
    """The point estimate and `n_boot` bootstrap replicates of the per-class and macro AUROC.
    seed: the replicates' draws come from the device's counter-based generator (`draws` restates it); the same seed resamples two score sets
    identically, whatever the chunking.  indices: (R, n) draws with replacement instead (host or device; R replaces n_boot): replicate b is then
    `get_accuracy(preds[indices[b]], labels[indices[b]])`.  A seed other than 0 beside indices is refused.
    workspace_bytes: bound on the multiplicity rows held at once (default 256 MiB); the replicates run in chunks of that many rows.
    The result records `n`, `n_boot`, `seed` (None under indices) and `source` (`draw_source`), which `pr_metrics.paired_diff_ci` compares."""
    return _bootstrap((AUC,), scores, labels, n_boot, seed, indices, from_logits, id2code, workspace_bytes)[0]


def bootstrap_keywords(bootstrap):
    """`bootstrap` of `HipEvaluator.evaluate` / `HipKnnProbe`: an int (n_boot) or a dict of `bootstrap_auc`'s keywords -> the dict"""
    if isinstance(bootstrap, bool) or not isinstance(bootstrap, (int, dict)):
        raise ValueError(f'bootstrap must be None, an integer or a dict of bootstrap_auc keywords, got {bootstrap!r}')
    kw = dict(bootstrap) if isinstance(bootstrap, dict) else dict(n_boot=bootstrap)
    bad = set(kw) - {'n_boot', 'seed', 'indices', 'workspace_bytes'}
    if bad:
        raise ValueError(f'bootstrap: unknown keywords {sorted(bad)}')
    return kw
