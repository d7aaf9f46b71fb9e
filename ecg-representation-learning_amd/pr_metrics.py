"""
Average precision and class-wise F-max on the device, with bootstrap confidence intervals (`include/ecgvit_hip_pr.h` states the contract,
`csrc/pr_metrics.hip` holds the kernel).

The rank route (`rank_metrics`) sorts every class column once.  A second walk over the same packed order, from the highest score down, leaves six
exact integers per (replicate, class): (ap_q, wp, wn, f_tp, f_fp, f_pos).  AP = ap_q / (2^32 wp) is scikit-learn's step-wise
`average_precision_score(y, s, sample_weight=w)` to within 2^-32; F-max = 2 f_tp / (f_tp + f_fp + wp) is the maximum of F1 over all thresholds
"score >= t", and the threshold is the score of the record at sorted position f_pos (ties in F go to the highest threshold).  With a replicate's
multiplicities as the weights these are the values on the resample.  The divisions and the percentiles are host f64.

The replicates are those of `bootstrap_auc`: the same generator, the same `indices` rule, the same chunking.  With one seed the AUROC, AP and F-max
replicates are the same resamples, and `paired_diff_ci` compares two score sets replicate by replicate.

A class is valid in a replicate when it holds a positive and a negative of non-zero weight (`BootstrapResult`'s rule): NaN otherwise, left out of the
replicate's macro average.  The PTB-XL benchmark's sample-centric Fmax (per-record precision and recall over a threshold grid) is another quantity
and is not built here.
"""
import numpy as np
import torch

from . import pr_abi, rank_abi, rank_metrics
from .hip import ptr, stream
from .rank_metrics import RankedScores, BootstrapResult, ReplicateResult, Route

__all__ = ['PrCounts', 'PrBootstrapResult', 'pr_walk', 'pr_counts', 'bootstrap_pr', 'paired_diff_ci']

_Q = float(1 << 32)
METRICS = ('ap', 'fmax')


def pr_walk(ranked, mult=None, replicates=1):
    """One launch of `ecgvit_pr_walk` (asynchronous) -> (R, K, 6) int64 on the device: (ap_q, wp, wn, f_tp, f_fp, f_pos).
    ranked: a `RankedScores`.  mult: None (unit weights; replicates must be 1), or the record-major multiplicities of `replicates` replicates as
    `ecgvit_rank_multiplicities*` leave them: an int32 device tensor of at least n * R4 elements, R4 = replicates rounded up to a multiple of 4.
    The caller guarantees that a replicate's weights sum to less than 2^30."""
    if not isinstance(ranked, RankedScores):
        raise ValueError(f'ranked must be a RankedScores (rank_scores makes one), got {type(ranked).__name__}')
    if isinstance(replicates, bool) or not isinstance(replicates, int) or not 1 <= replicates <= rank_abi.MAX_REPLICATES:
        raise ValueError(f'replicates must be an integer in [1, {rank_abi.MAX_REPLICATES}], got {replicates!r}')
    if ranked.n >= pr_abi.MAX_WEIGHT:
        raise ValueError(f'ranked: n = {ranked.n}, the weights of a replicate must sum to less than {pr_abi.MAX_WEIGHT}')
    if mult is None:
        if replicates != 1:
            raise ValueError(f'replicates must be 1 without mult (unit weights are one replicate), got {replicates}')
    else:
        r4 = rank_metrics.pad4(replicates)
        if not isinstance(mult, torch.Tensor) or mult.dtype != torch.int32:
            raise ValueError('mult must be an int32 tensor of record-major multiplicities')
        if not mult.is_contiguous() or mult.numel() < ranked.n * r4:
            raise ValueError(f'mult must be contiguous and hold at least n * R4 = {ranked.n} * {r4} elements, got {tuple(mult.shape)}')
        if mult.device != ranked.packed.device:
            raise ValueError(f'mult must be on {ranked.packed.device} as ranked, got {mult.device}')
        if mult.data_ptr() % 16:
            raise ValueError('mult must be 16-byte aligned')
    out = torch.empty(replicates, ranked.K, pr_abi.SLOTS, dtype=torch.int64, device=ranked.packed.device)
    _walk(ranked, mult, replicates, out)
    return out


def _walk(ranked, mult, R, out):
    pr_abi.run.ecgvit_pr_walk(ptr(ranked.packed), ptr(ranked.first_nan), ranked.n, ranked.K, ptr(mult), R, ptr(out), stream())


def _values(sixes):
    """(..., K, 6) int64 -> valid (..., K) bool, AP and F-max (..., K) f64 with NaN where invalid"""
    ap_q, wp, wn, tp, fp = (sixes[..., i].astype(np.float64) for i in range(5))
    valid = rank_metrics.valid_classes(sixes)
    with np.errstate(divide='ignore', invalid='ignore'):
        ap = np.where(valid, ap_q / (_Q * wp), np.nan)
        fmax = np.where(valid, 2.0 * tp / (tp + fp + wp), np.nan)
    return valid, ap, fmax


class PrCounts:
    """Handle on the six integers per class of one unit-weight walk; `.result()` syncs and returns the dict.  `sixes`: (1, K, 6) int64 on the device."""

    def __init__(self, ranked, sixes, id2code=None):
        self.ranked, self.sixes, self.id2code = ranked, sixes, id2code

    def result(self):
        """macro_ap, per_class_ap, macro_fmax, per_class_fmax, per_class_threshold: keyed as `get_accuracy` keys `per_class_auc` (class index, or
        `id2code`'s name), invalid classes left out; None when no class is valid.  The threshold is the f32 score itself (the logit under
        from_logits) of the lowest record of the winning tie group: predicting `score >= threshold` gives F-max.  A valid class whose positives
        all score NaN has F-max 0 and threshold +inf (predict nothing)."""
        r, K = self.ranked, self.ranked.K
        pos = self.sixes[0, :, 5]
        rec = r.records(r.packed.gather(1, pos.clamp(min=0)[:, None])[:, 0])
        thr = r.scores[rec, torch.arange(K, device=rec.device)].cpu().numpy()
        six = self.sixes.cpu().numpy()[0]
        valid, ap, fmax = _values(six)
        ks = [k for k in range(K) if valid[k]]
        if not ks:
            return dict(macro_ap=None, per_class_ap=None, macro_fmax=None, per_class_fmax=None, per_class_threshold=None)
        key = (lambda k: self.id2code[k]) if self.id2code is not None else (lambda k: k)
        per_ap, per_f = {key(k): float(ap[k]) for k in ks}, {key(k): float(fmax[k]) for k in ks}
        per_t = {key(k): float(thr[k]) if six[k, 5] >= 0 else float('inf') for k in ks}
        return dict(macro_ap=sum(per_ap.values()) / len(ks), per_class_ap=per_ap, macro_fmax=sum(per_f.values()) / len(ks), per_class_fmax=per_f,
                    per_class_threshold=per_t)


def _counts(ranked, id2code):
    return PrCounts(ranked, pr_walk(ranked), id2code)


def pr_counts(scores, labels, from_logits=False, id2code=None) -> PrCounts:
    """Sort every class column, then one unit-weight walk (asynchronous).  scores / labels: (n, K) f32 device tensors with contiguous rows, as
    `rank_scores` takes them.  `.result()` is the dict of average precision, F-max and its threshold per class and their macro averages."""
    return _counts(rank_metrics.rank_scores(scores, labels, from_logits), id2code)


class PrBootstrapResult(ReplicateResult):
    """`point`: the `pr_counts` dict of the whole set.  `sixes`: (R, K, 6) int64 as the device left them.  `per_class_ap`, `per_class_fmax` (R, K)
    f64, NaN where the replicate holds one label value only; `macro_ap`, `macro_fmax` (R,) the means over the replicate's valid classes (NaN:
    none); `n_valid` (K,) replicates in which the class is valid.  `n`, `n_boot`, `seed`, `source`: the draws' record, as on `BootstrapResult`."""

    def __init__(self, point, sixes, id2code=None):
        super().__init__(point, sixes, id2code)
        self.sixes = sixes
        _, self.per_class_ap, self.per_class_fmax = _values(sixes)
        self.macro_ap, self.macro_fmax = self._macro(self.per_class_ap), self._macro(self.per_class_fmax)

    @staticmethod
    def _metric(metric):
        if metric not in METRICS:
            raise ValueError(f'metric must be one of {METRICS}, got {metric!r}')
        return metric

    def ci(self, metric='ap', alpha=0.05):
        """(lo, hi) of the macro value: the alpha / 2 and 1 - alpha / 2 percentiles of the replicates that have a valid class"""
        return self._ci(self._metric(metric), alpha)

    def class_ci(self, metric='ap', alpha=0.05):
        """(K, 2) per-class (lo, hi) over the replicates in which the class is valid; NaN for a class that never is"""
        return self._class_ci(self._metric(metric), alpha)


PR = Route(_counts, _walk, pr_abi.SLOTS, PrBootstrapResult, METRICS, 'bootstrap_pr', pr_abi.MAX_WEIGHT)


def bootstrap_pr(scores, labels, n_boot=1000, seed=0, indices=None, from_logits=False, id2code=None, workspace_bytes=None) -> PrBootstrapResult:
    """The point estimate and `n_boot` bootstrap replicates of per-class and macro average precision and F-max.  Every argument is
    `bootstrap_auc`'s, and so are the draws: under one seed (or the same indices) replicate b here and replicate b there are the same resample."""
    return rank_metrics._bootstrap((PR,), scores, labels, n_boot, seed, indices, from_logits, id2code, workspace_bytes)[0]


def paired_diff_ci(a, b, metric, alpha=0.05):
    """(lo, hi): the percentile interval of the replicate-wise differences a - b of two results' macro values.  metric: 'auc' for two
    `BootstrapResult`s, 'ap' or 'fmax' for two `PrBootstrapResult`s.  The two must have resampled identically: the same n, n_boot and draw source
    (one seed, or the same indices), else the differences pair nothing and the call is refused."""
    kind = BootstrapResult if metric == 'auc' else PrBootstrapResult if metric in METRICS else None
    if kind is None:
        raise ValueError(f"metric must be 'auc', 'ap' or 'fmax', got {metric!r}")
    for r, name in ((a, 'a'), (b, 'b')):
        if not isinstance(r, kind):
            raise ValueError(f'{name} must be a {kind.__name__} for metric {metric!r}, got {type(r).__name__}')
        if r.source is None:
            raise ValueError(f'{name} carries no record of its draws (bootstrap_auc / bootstrap_pr make results that do)')
    for field in ('n', 'n_boot', 'source'):
        if getattr(a, field) != getattr(b, field):
            raise ValueError(f'b was not resampled as a: {field} is {getattr(b, field)!r} against {getattr(a, field)!r}')
    lo, hi = ReplicateResult.percentiles(getattr(a, 'macro_' + metric) - getattr(b, 'macro_' + metric), alpha)
    return float(lo), float(hi)
