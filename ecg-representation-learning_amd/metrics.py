"""
Evaluation metrics computed on the device.

Mirror of the reference's `get_accuracy` (`ecg_transformer/util/train.py:12-56`) -- same name, arguments, keys and (quirky)
meanings -- and of `MyTrainer.evaluate` (`ecg_transformer/models/train.py:321-378`).  The reference calls `get_accuracy` on EVERY
train step (`models/train.py:289`): a D2H copy of (B, 71) logits, a host sync, and four sklearn passes.  Here one stream-ordered
`ecgvit_eval_counts` launch leaves 4 + 2*71 exact integers in device memory; they are read (146 x 8 bytes) only when somebody
looks at the numbers, so the train loop stays asynchronous.  The few divisions are done on the host in double precision.

Reference quirks kept, because a drop-in has to log the same numbers (see oracle/metrics_oracle.py for the derivation):
`binary_positive_recall` is tn / (tn + fn) and `binary_negative_recall` is tp / (tp + fp) -- the reference swaps y_true / y_pred in
`classification_report` and then swaps the two names (train.py:46-49).
`per_class_auc` keys: the reference maps class index -> PTB-XL code through its dataset config (`id2code`, train.py:21-22); the
dataset metadata is out of scope here, so pass `id2code` (a list of 71 names) or get integer class indices as keys.
"""
import torch

from . import hip
from .engine import ragged_slice, RawPaddedBatch
from .hip import run, ptr, stream


class DeviceCounts:
    """Handle on the integer statistics of one (scores, labels) pair; `.result()` syncs and returns the reference's dict."""

    def __init__(self, counts, B, K, return_auc, id2code):
        self.counts, self.B, self.K, self.return_auc, self.id2code = counts, B, K, return_auc, id2code

    def result(self):
        c = self.counts.cpu().tolist()   # the only D2H transfer (and sync) of the metric path
        B, K = self.B, self.K
        tp, tn, fp, fn = c[:4]
        recalls = [r for r in ((tn / (tn + fp)) if tn + fp else None, (tp / (tp + fn)) if tp + fn else None) if r is not None]
        macro, per_class = None, None
        if self.return_auc:
            pos, pairs = c[4:4 + K], c[4 + K:]
            valid = [k for k in range(K) if 0 < pos[k] < B]   # classes with both label values (train.py:29)
            if valid:
                per_class = {(self.id2code[k] if self.id2code is not None else k): pairs[k] / (2.0 * pos[k] * (B - pos[k])) for k in valid}
                vals = list(per_class.values())
                macro = sum(vals) / len(vals)
        return dict(
            binary_accuracy=(tp + tn) / (B * K),
            weighted_binary_accuracy=sum(recalls) / len(recalls),
            binary_negative_recall=tp / (tp + fp) if tp + fp else 0.0,
            binary_positive_recall=tn / (tn + fn) if tn + fn else 0.0,
            macro_auc=macro, per_class_auc=per_class)


def eval_counts(scores, labels, from_logits=False, return_auc=True, id2code=None) -> DeviceCounts:
    """Launch the counting kernels (asynchronous). scores / labels: (B, K) f32 device tensors."""
    if not (scores.is_cuda and labels.is_cuda):
        raise RuntimeError('metrics run on the device (no CPU fallback exists): pass device tensors')
    assert scores.dim() == 2 and scores.shape == labels.shape and scores.dtype == torch.float32 and labels.dtype == torch.float32
    assert scores.stride(1) == 1 and labels.stride(1) == 1
    B, K = scores.shape
    counts = torch.empty(4 + 2 * K, dtype=torch.int64, device=scores.device)
    run.ecgvit_eval_counts(ptr(scores), scores.stride(0), ptr(labels), labels.stride(0), B, K, int(from_logits), int(return_auc),
                           ptr(counts), stream())
    h = DeviceCounts(counts, B, K, return_auc, id2code)
    h._keep = (scores, labels)
    return h


def get_accuracy(preds, labels, return_auc=True, id2code=None):
    """Drop-in for the reference's `get_accuracy(preds, labels, return_auc)`: `preds` are per-class probabilities."""
    return eval_counts(preds, labels, from_logits=False, return_auc=return_auc, id2code=id2code).result()


class HipEvaluator:
    """`MyTrainer.evaluate` (models/train.py:321-378) with everything kept on the device: logits of the whole eval set are written
    into one (n_eval, K) buffer, the loss is the mean of the per-batch mean losses (train.py:357-358), and the metrics come from one
    `ecgvit_eval_counts` over the whole set. With torch.distributed initialised and `gather=True` each rank evaluates its shard of the
    records and the (logits, labels) shards are all-gathered (RCCL) before counting, so every rank reports whole-set AUROC."""

    def __init__(self, model, eval_batch_size=64, id2code=None, gather=False, process_group=None):
        self.model, self.bsz, self.id2code, self.gather, self.pg = model, int(eval_batch_size), id2code, gather, process_group

    def evaluate(self, sample_values, labels, return_predictions=False, lengths=None, bootstrap=None, pr=False):
        """bootstrap: None, or an int (replicates) or a dict of `rank_metrics.bootstrap_auc`'s keywords (n_boot, seed, indices, workspace_bytes):
        adds `eval/macro_auc_ci` and `eval/per_class_auc_ci`, the 95 % percentile intervals over the resampled whole set (every rank of a
        gathered evaluation holds the whole set and draws the same replicates from the same seed), and `bootstrap` under `predictions`.
        pr: True adds `eval/macro_ap`, `eval/per_class_ap`, `eval/macro_fmax`, `eval/per_class_fmax` and `eval/per_class_threshold`
        (`pr_metrics.pr_counts`: average precision, the class-wise maximum of F1 over all thresholds, and the logit that attains it), and with
        `bootstrap` their `_ci` keys over the same replicates (`bootstrap_pr` under `predictions`).  False: nothing is added or launched.
        sample_values: (n, C, L) f32 device tensor (this rank's shard), labels: (n, K) f32; lengths: optional (n,) per-record sample
        counts (EcgVit.forward), sliced with the batches.  A ragged (C, S) batch with its (n,) lengths is cut by record range: eval_batch_size
        records per call, each a ragged batch of its own.  Under a per-record input transform sample_values holds RAW records and lengths their
        raw sample counts (the ragged form is then cut at the raw offsets); evaluation draws no TimeOut."""
        model = self.model
        training = model.training
        model.eval()
        n, K = labels.shape
        if sample_values.dim() == 2:   # ragged: validated once, then cut by record range on the host offsets
            sample_values = sample_values.contiguous().float()
            lengths = model._engine().check_ragged_input(sample_values, lengths, labels)
        elif getattr(getattr(model, '_input_transform', None), 'per_record', False):
            # RAW records (n, C, W) with raw lengths: validated once, every batch runs at the set's pass width (eval: no TimeOut)
            lengths = model._engine().check_raw_input(sample_values, lengths)
        logits = torch.empty(n, K, dtype=torch.float32, device=labels.device)
        losses = []
        with torch.no_grad():
            for s in range(0, n, self.bsz):
                if sample_values.dim() == 2:
                    xs, ls = ragged_slice(sample_values, lengths, s, min(s + self.bsz, n))
                elif isinstance(lengths, RawPaddedBatch):
                    xs, ls = sample_values[s:s + self.bsz], lengths.records(s, min(s + self.bsz, n))
                else:
                    xs, ls = sample_values[s:s + self.bsz], None if lengths is None else lengths[s:s + self.bsz]
                out = model(sample_values=xs, labels=labels[s:s + self.bsz], lengths=ls)
                logits[s:s + self.bsz] = out.logits
                losses.append(out.loss.detach().reshape(()))
        loss = torch.stack(losses).mean()
        lb = labels
        if self.gather and torch.distributed.is_available() and torch.distributed.is_initialized():
            import torch.distributed as dist
            ws = dist.get_world_size(self.pg)
            sizes = [torch.zeros(1, dtype=torch.int64, device=labels.device) for _ in range(ws)]
            dist.all_gather(sizes, torch.tensor([n], dtype=torch.int64, device=labels.device), group=self.pg)
            sizes = [int(v) for v in sizes]
            mx = max(sizes)

            def gather(t):
                pad = torch.zeros(mx, K, dtype=t.dtype, device=t.device)
                pad[:n] = t
                parts = [torch.empty_like(pad) for _ in range(ws)]
                dist.all_gather(parts, pad, group=self.pg)
                return torch.cat([p[:m] for p, m in zip(parts, sizes)], dim=0)
            logits, lb = gather(logits), gather(labels)
            wsum = loss * len(losses)
            cnt = torch.tensor([float(len(losses))], device=labels.device)
            dist.all_reduce(wsum, group=self.pg)
            dist.all_reduce(cnt, group=self.pg)
            loss = wsum / cnt[0]
        m = eval_counts(logits, lb.contiguous(), from_logits=True, return_auc=True, id2code=self.id2code).result()
        d = {'eval/loss': float(loss), **{f'eval/{k}': v for k, v in m.items()}}
        pred = dict(labels=lb, logits=logits)
        _add_bootstrap(d, pred, 'eval', bootstrap, logits, lb.contiguous(), True, self.id2code, pr)
        if training:
            model.train()
        return dict(metrics=d, predictions=pred) if return_predictions else d


def _add_bootstrap(d, predictions, prefix, bootstrap, scores, labels, from_logits, id2code, pr=False):
    """the interval keys of an evaluation that asked for them; with bootstrap=None nothing is added and nothing is launched.  pr: the keys of
    average precision and F-max as well, and then the AUROC intervals come from the same sort and the same draws"""
    if pr is not False and pr is not True:
        raise ValueError(f'pr must be True or False, got {pr!r}')
    if bootstrap is None and not pr:
        return
    from . import rank_metrics
    routes = (rank_metrics.AUC,)
    if pr:
        from . import pr_metrics
        routes += (pr_metrics.PR,)
    if bootstrap is None:
        point = pr_metrics.pr_counts(scores, labels, from_logits, id2code).result()
    else:
        results = rank_metrics._bootstrap(routes, scores, labels, from_logits=from_logits, id2code=id2code, **rank_metrics.bootstrap_keywords(bootstrap))
        for route, res in zip(routes, results):
            for metric in route.metrics:
                d[f'{prefix}/macro_{metric}_ci'], d[f'{prefix}/per_class_{metric}_ci'] = rank_metrics.intervals(res, metric)
            predictions[route.key] = res
        point = results[-1].point   # the PR route's, under pr
    if pr:
        d.update({f'{prefix}/{k}': v for k, v in point.items()})


class HipEncoder:
    """Pooled representations of a resident data set (`EcgVit.encode`), `batch_size` records per encoder pass: the feature cache of a linear
    probe on frozen features (`HipProbeStep`), of clustering or retrieval.  pool / norm: as `EcgVit.encode`."""

    def __init__(self, model, batch_size=64, pool='cls', norm=True):
        if pool not in ('cls', 'mean'):
            raise ValueError(f"pool must be 'cls' or 'mean', got {pool!r}")
        self.model, self.bsz, self.pool, self.norm = model, int(batch_size), pool, bool(norm)
        if self.bsz <= 0:
            raise ValueError(f'batch_size must be positive, got {batch_size!r}')

    def encode(self, sample_values, lengths=None):
        """sample_values: (n, C, L') f32 device tensor with optional (n,) lengths, sliced with the batches, or a ragged (C, S) batch with its
        (n,) lengths, cut by record range as `HipEvaluator.evaluate` cuts it (raw records and raw lengths under a per-record input transform).
        Returns (n, hidden_size) f32 on the device, row r = record r."""
        model = self.model
        ragged = sample_values.dim() == 2
        if ragged:   # validated once, then cut by record range on the host offsets
            sample_values = sample_values.contiguous().float()
            lengths = model._engine().check_ragged_input(sample_values, lengths)
            n = lengths.B
        else:
            n = sample_values.shape[0]
            if getattr(getattr(model, '_input_transform', None), 'per_record', False):
                lengths = model._engine().check_raw_input(sample_values, lengths)   # every batch runs at the set's pass width
        out = torch.empty(n, model.config.hidden_size, dtype=torch.float32, device=sample_values.device)
        for s in range(0, n, self.bsz):
            e = min(s + self.bsz, n)
            if ragged:
                xs, ls = ragged_slice(sample_values, lengths, s, e)
            elif isinstance(lengths, RawPaddedBatch):
                xs, ls = sample_values[s:e], lengths.records(s, e)
            else:
                xs, ls = sample_values[s:e], None if lengths is None else lengths[s:e]
            out[s:e] = model.encode(xs, lengths=ls, pool=self.pool, norm=self.norm)
        return out


class HipKnnProbe:
    """The weighted k-NN probe: a training-free score of an encoder.  The bank records' pooled representations (`HipEncoder`) are the bank;
    every evaluation record votes with the labels of its k nearest bank records under the cosine metric, weighted by
    exp((s_j - s_0) / temperature) (weights='softmax') or equally ('uniform').  The (Q, K) result, the weighted share of the neighbours that
    carry each label (the multi-label form), goes to `eval_counts(..., from_logits=False)` as probabilities.  k = 20 and temperature = 0.07
    are those of the usual weighted k-NN protocol (Wu et al., "Unsupervised Feature Learning via Non-Parametric Instance Discrimination",
    CVPR 2018).  No optimiser runs: the price is one `encode` pass over both sets, a search (`knn.KnnIndex`) and a vote."""

    def __init__(self, model, k=20, temperature=0.07, weights='softmax', batch_size=64, pool='cls', norm=True, id2code=None):
        from . import knn
        if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= knn.knn_abi.MAX_K:
            raise ValueError(f'k must be an integer in [1, {knn.knn_abi.MAX_K}], got {k!r}')
        if weights not in knn.WEIGHTS:
            raise ValueError(f'weights must be one of {knn.WEIGHTS}, got {weights!r}')
        if isinstance(temperature, bool) or not isinstance(temperature, (int, float)) or not 0 < temperature < float('inf'):
            raise ValueError(f'temperature must be a positive finite number, got {temperature!r}')
        self.model, self.k, self.temperature, self.weights, self.id2code = model, k, float(temperature), weights, id2code
        self.encoder = HipEncoder(model, batch_size=batch_size, pool=pool, norm=norm)

    def _encode(self, *sets):
        # (`EcgVit.encode` is an eval pass under no_grad whatever `model.training` says, and leaves the flag as it was)
        return [self.encoder.encode(x, lengths=ls) for x, ls in sets]

    def _score(self, index, feats, labels_bank, labels_query, exclude_self, return_predictions, bootstrap=None, pr=False):
        from . import knn
        for t, name in ((labels_bank, 'bank_y'), (labels_query, 'query_y')):
            if not isinstance(t, torch.Tensor) or t.dim() != 2 or t.dtype != torch.float32:
                raise ValueError(f'{name} must be a 2-d float32 tensor')
        if labels_bank.shape[0] != index.N:
            raise ValueError(f'bank_y has {labels_bank.shape[0]} rows, the bank has {index.N} records')
        if labels_query.shape != (feats.shape[0], labels_bank.shape[1]):
            raise ValueError(f'query_y must be {(feats.shape[0], labels_bank.shape[1])}, got {tuple(labels_query.shape)}')
        scores, indices = index.search(feats, self.k, exclude_self=exclude_self)
        probs = index.vote(scores, indices, labels_bank, weights=self.weights, temperature=self.temperature)
        m = eval_counts(probs, labels_query.contiguous(), from_logits=False, return_auc=True, id2code=self.id2code).result()
        d = {f'knn/{key}': v for key, v in m.items()}
        pred = dict(labels=labels_query, probabilities=probs, scores=scores, indices=indices)
        _add_bootstrap(d, pred, 'knn', bootstrap, probs, labels_query.contiguous(), False, self.id2code, pr)
        return dict(metrics=d, predictions=pred) if return_predictions else d

    def evaluate(self, bank_x, bank_y, query_x, query_y, bank_lengths=None, query_lengths=None, return_predictions=False, bootstrap=None, pr=False):
        """bank_x / query_x with their lengths: as `HipEncoder.encode` takes them (a rectangle, a rectangle with lengths, a ragged (C, S)
        batch, raw records under a per-record input transform); bank_y (N, K), query_y (Q, K) f32 multi-hot labels on the device.
        Returns the keys of `get_accuracy` under the `knn/` prefix (return_predictions: dict(metrics=..., predictions=...)).
        bootstrap: as `HipEvaluator.evaluate` takes it, over the query records: adds `knn/macro_auc_ci` and `knn/per_class_auc_ci`.
        pr: as `HipEvaluator.evaluate` takes it: the average-precision and F-max keys under `knn/` (thresholds are vote shares)."""
        from . import knn
        fb, fq = self._encode((bank_x, bank_lengths), (query_x, query_lengths))
        return self._score(knn.KnnIndex(fb, metric='cosine'), fq, bank_y, query_y, False, return_predictions, bootstrap, pr)

    def leave_one_out(self, x, y, lengths=None, return_predictions=False, bootstrap=None, pr=False):
        """`evaluate` with the set as its own bank: record r never receives itself (by index: a duplicate of it is still a neighbour)"""
        from . import knn
        f, = self._encode((x, lengths))
        return self._score(knn.KnnIndex(f, metric='cosine'), f, y, y, True, return_predictions, bootstrap, pr)


class HipRollout:
    """Attention maps of a resident data set (`EcgVit.attention_rollout_batch`), `batch_size` records per pass: what the reference derives one
    record at a time for the low / median / high-loss records of an evaluation (models/evaluate.py:31-55), for as many records as are asked."""

    def __init__(self, model, batch_size=64):
        self.model, self.bsz = model, int(batch_size)
        if self.bsz <= 0:
            raise ValueError(f'batch_size must be positive, got {batch_size!r}')

    def rollout(self, sample_values, lengths=None):
        """sample_values / lengths: as `HipEncoder.encode` takes and cuts them.  Returns (logits (n, K), maps (n, layers, n_max) f32 with
        n_max = the patches of the set's widest record and exact zeros past each record's own, patch_counts (n,) int64 on the host)."""
        model = self.model
        if sample_values.dim() not in (2, 3):
            raise ValueError(f'sample_values must be (n, C, L) or a ragged (C, S) batch, got {tuple(sample_values.shape)}')
        ragged = sample_values.dim() == 2
        if ragged:   # validated once, then cut by record range on the host offsets
            sample_values = sample_values.contiguous().float()
            lengths = model._engine().check_ragged_input(sample_values, lengths)
            n = lengths.B
        else:
            n = sample_values.shape[0]
            if getattr(getattr(model, '_input_transform', None), 'per_record', False):
                lengths = model._engine().check_raw_input(sample_values, lengths)   # every batch runs at the set's pass width
        parts = []
        for s in range(0, n, self.bsz):
            e = min(s + self.bsz, n)
            if ragged:
                xs, ls = ragged_slice(sample_values, lengths, s, e)
            elif isinstance(lengths, RawPaddedBatch):
                xs, ls = sample_values[s:e], lengths.records(s, e)
            else:
                xs, ls = sample_values[s:e], None if lengths is None else lengths[s:e]
            parts.append(model.attention_rollout_batch(xs, lengths=ls))
        counts = torch.cat([p.patch_counts for p in parts])
        logits = torch.cat([p.logits for p in parts])
        maps = torch.zeros(n, parts[0].maps.shape[1], int(counts.max()), dtype=torch.float32, device=logits.device)
        s = 0
        for p in parts:
            maps[s:s + p.maps.shape[0], :, :p.maps.shape[2]] = p.maps
            s += p.maps.shape[0]
        return logits, maps, counts
