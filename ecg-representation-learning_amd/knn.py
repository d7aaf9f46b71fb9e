"""
Exact k-nearest-neighbour search over pooled representations (`EcgVit.encode`, `HipEncoder`) and the weighted vote of a k-NN probe, on the
device: `include/ecgvit_hip_knn.h` states the contract (the f32 fmaf-chain score, the total order (score descending, bank index ascending),
what a non-finite score, `self_base` and `index_base` mean), `csrc/knn.hip` holds the kernels.  The (Q, N) similarity matrix is never stored.

    index = KnnIndex(bank_features)                       # metric='cosine': keeps the normalised copy
    scores, indices = index.search(query_features, k=20)
    probs = index.vote(scores, indices, bank_labels)      # (Q, K): the weighted share of neighbours that carry each label

A bank that arrives in chunks (host-resident, or one shard per rank) is searched chunk by chunk with `index_base` = the chunk's first row and
the lists are joined by `knn_merge`.  Torch supplies memory and the stream; there is no fallback.
"""
import torch

from . import hip, knn_abi
from .hip import ptr, stream

METRICS = ('cosine', 'dot')
WEIGHTS = ('softmax', 'uniform')


def _on_device(t, name):
    if not t.is_cuda:
        raise ValueError(f'{name} must be a device tensor (no CPU fallback exists)')
    return t


def _features(t, name, device=True):
    """a (rows, d) f32 device tensor whose rows are contiguous, or a ValueError that names the argument.  The device is looked at last
    (device=False: not at all; the caller does, after its own checks), so every other refusal can be met with a host tensor."""
    if not isinstance(t, torch.Tensor):
        raise ValueError(f'{name} must be a tensor, got {type(t).__name__}')
    if t.dtype != torch.float32:
        raise ValueError(f'{name} must be float32, got {t.dtype}')
    if t.dim() != 2 or t.shape[0] < 1 or t.shape[1] < 1:
        raise ValueError(f'{name} must be (rows, d) with at least one row and one column, got {tuple(t.shape)}')
    if t.stride(1) != 1:
        raise ValueError(f'{name} must have contiguous rows (last-dimension stride 1), got stride {t.stride(1)}')
    if t.shape[1] > hip.ROW_MAX_D:
        raise ValueError(f'{name}: d = {t.shape[1]} exceeds {hip.ROW_MAX_D}')
    return _on_device(t, name) if device else t


def _pitch(t):
    return t.stride(0) if t.shape[0] > 1 else t.shape[1]


def _check_k(k, most, what):
    if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= min(knn_abi.MAX_K, most):
        raise ValueError(f'k must be an integer in [1, {min(knn_abi.MAX_K, most)}] ({what}), got {k!r}')


def normalize(x):
    """rows of `x` scaled to unit length (sum and product in f64, a zero row stays zero) -> a dense (rows, d) f32 tensor"""
    x = _features(x, 'x')
    out = torch.empty(x.shape, dtype=torch.float32, device=x.device)
    knn_abi.run.ecgvit_knn_normalize(ptr(x), _pitch(x), ptr(out), x.shape[1], x.shape[0], x.shape[1], stream())
    return out


def _search(q, b, k, self_base, index_base, splits):
    Q, d = q.shape
    N = b.shape[0]
    splits = 0 if splits is None else splits
    if isinstance(splits, bool) or not isinstance(splits, int) or not 0 <= splits <= knn_abi.MAX_SPLITS:
        raise ValueError(f'splits must be None or an integer in [0, {knn_abi.MAX_SPLITS}], got {splits!r}')
    if max(_pitch(q), _pitch(b)) > knn_abi.MAX_PITCH:
        raise ValueError(f'queries / bank: a row pitch above {knn_abi.MAX_PITCH} elements')
    nbytes = knn_abi.lib().ecgvit_knn_workspace(Q, N, d, k, splits)
    if nbytes <= 0:
        raise ValueError(f'knn search: unsupported arguments (Q {Q}, N {N}, d {d}, k {k}, splits {splits})')
    ws = torch.empty(nbytes, dtype=torch.uint8, device=q.device)
    scores = torch.empty(Q, k, dtype=torch.float32, device=q.device)
    indices = torch.empty(Q, k, dtype=torch.int64, device=q.device)
    knn_abi.run.ecgvit_knn_search(ptr(q), _pitch(q), ptr(b), _pitch(b), Q, N, d, k, self_base, index_base, splits, ptr(scores), ptr(indices),
                                  ptr(ws), stream())
    return scores, indices


def _query_args(queries, N, d, k, exclude_self, self_base, index_base):
    """the refusals of a search against a bank of N rows of d columns, the device last -> queries"""
    queries = _features(queries, 'queries', device=False)
    if queries.shape[1] != d:
        raise ValueError(f'queries have d = {queries.shape[1]}, the bank has d = {d}')
    if exclude_self and (isinstance(self_base, bool) or not isinstance(self_base, int) or self_base < 0):
        raise ValueError(f'self_base must be a non-negative integer, got {self_base!r}')
    if isinstance(index_base, bool) or not isinstance(index_base, int):
        raise ValueError(f'index_base must be an integer, got {index_base!r}')
    _check_k(k, N - 1 if exclude_self else N, 'the bank rows a query may receive')
    return _on_device(queries, 'queries')


class KnnIndex:
    """A bank of (N, d) f32 feature rows on the device, searched exactly.  metric 'cosine': the bank and every query are normalised first
    (`normalize`; the normalised bank is kept, the caller's tensor is not touched); 'dot': the rows as they are."""

    def __init__(self, bank, metric='cosine'):
        if metric not in METRICS:
            raise ValueError(f'metric must be one of {METRICS}, got {metric!r}')
        bank = _features(bank, 'bank')
        self.metric = metric
        self.bank = normalize(bank) if metric == 'cosine' else bank
        self.N, self.d = bank.shape

    def search(self, queries, k, exclude_self=False, self_base=0, index_base=0, splits=None):
        """The first k bank rows of every query under (score descending, bank index ascending) -> (scores (Q, k) f32, indices (Q, k) int64);
        a query with fewer than k admissible rows (finite score, not its own row) ends on index -1 / score -inf.
        exclude_self: query q is bank row `self_base + q` and never receives it (leave-one-out).  index_base is added to every reported
        index (a chunk of a larger bank).  splits: row ranges of the bank across the grid, None = the library chooses; the result does not
        depend on it."""
        queries = _query_args(queries, self.N, self.d, k, exclude_self, self_base, index_base)
        if queries.device != self.bank.device:
            raise ValueError(f'queries are on {queries.device}, the bank on {self.bank.device}')
        q = normalize(queries) if self.metric == 'cosine' else queries
        return _search(q, self.bank, k, self_base if exclude_self else -1, index_base, splits)

    def vote(self, scores, indices, labels, weights='softmax', temperature=0.07):
        """out[q][c] = sum_j w_j labels[indices[q][j]][c] / sum_j w_j over the slots that hold a neighbour -> (Q, K) f32; a query with none
        gets 0.  weights 'uniform': w_j = 1; 'softmax': w_j = exp((s_j - s_0) / temperature), s_0 the query's best score.  `indices` are
        un-shifted bank rows (index_base = 0); labels: (N, K) f32, one row per bank row."""
        return vote(scores, indices, labels, weights=weights, temperature=temperature, n_bank=self.N)


def vote(scores, indices, labels, weights='softmax', temperature=0.07, n_bank=None):
    """`KnnIndex.vote` without an index: n_bank, when given, is the row count `labels` must have"""
    if weights not in WEIGHTS:
        raise ValueError(f'weights must be one of {WEIGHTS}, got {weights!r}')
    if isinstance(temperature, bool) or not isinstance(temperature, (int, float)) or not 0 < temperature < float('inf'):
        raise ValueError(f'temperature must be a positive finite number, got {temperature!r}')
    for t, name, dtype in ((scores, 'scores', torch.float32), (indices, 'indices', torch.int64), (labels, 'labels', torch.float32)):
        if not isinstance(t, torch.Tensor):
            raise ValueError(f'{name} must be a tensor, got {type(t).__name__}')
        if t.dtype != dtype or t.dim() != 2:
            raise ValueError(f'{name} must be a 2-d {dtype} tensor, got {t.dtype} {tuple(t.shape)}')
    if scores.shape != indices.shape or not 1 <= scores.shape[1] <= knn_abi.MAX_K or scores.shape[0] < 1:
        raise ValueError(f'scores {tuple(scores.shape)} and indices {tuple(indices.shape)} must be equal (Q, k) with k <= {knn_abi.MAX_K}')
    if n_bank is not None and labels.shape[0] != n_bank:
        raise ValueError(f'labels have {labels.shape[0]} rows, the bank has {n_bank}')
    if labels.stride(1) != 1 or not 1 <= labels.shape[1] <= knn_abi.MAX_CLASSES or labels.shape[0] < 1:
        raise ValueError(f'labels must be (N, K) with contiguous rows and K <= {knn_abi.MAX_CLASSES}, got {tuple(labels.shape)}')
    for t, name in ((scores, 'scores'), (indices, 'indices'), (labels, 'labels')):
        _on_device(t, name)
    scores, indices = scores.contiguous(), indices.contiguous()
    Q, k = scores.shape
    N, K = labels.shape
    out = torch.empty(Q, K, dtype=torch.float32, device=scores.device)
    mode = knn_abi.VOTE_SOFTMAX if weights == 'softmax' else knn_abi.VOTE_UNIFORM
    knn_abi.run.ecgvit_knn_vote(ptr(scores), ptr(indices), Q, k, ptr(labels), _pitch(labels), N, K, mode, float(temperature), ptr(out), stream())
    return out


def knn_search(queries, bank, k, metric='cosine', **kw):
    """`KnnIndex(bank, metric).search(queries, k, **kw)`, every argument looked at before anything is launched"""
    if metric not in METRICS:
        raise ValueError(f'metric must be one of {METRICS}, got {metric!r}')
    bank = _features(bank, 'bank', device=False)
    _query_args(queries, bank.shape[0], bank.shape[1], k, kw.get('exclude_self', False), kw.get('self_base', 0), kw.get('index_base', 0))
    return KnnIndex(bank, metric=metric).search(queries, k, **kw)


def knn_merge(parts, k):
    """parts: [(scores (Q, k_p), indices (Q, k_p)), ...] from searches of the chunks of one bank, each with its chunk's `index_base` -> the
    first k pairs of every query under the same total order, (Q, k) each.  Slots with index -1 are ignored; fewer than k pairs end on -1 / -inf."""
    parts = list(parts)
    if not parts:
        raise ValueError('parts must hold at least one (scores, indices) pair')
    for s, i in parts:
        for t, name, dtype in ((s, 'scores', torch.float32), (i, 'indices', torch.int64)):
            if not isinstance(t, torch.Tensor):
                raise ValueError(f'parts: {name} must be tensors, got {type(t).__name__}')
            if t.dtype != dtype or t.dim() != 2:
                raise ValueError(f'parts: {name} must be 2-d {dtype} tensors, got {t.dtype} {tuple(t.shape)}')
        if s.shape != i.shape or s.shape[0] != parts[0][0].shape[0] or s.shape[1] < 1 or s.shape[0] < 1:
            raise ValueError(f'parts: scores {tuple(s.shape)} / indices {tuple(i.shape)} must be equal (Q, k_p) with one Q for every part')
    _check_k(k, knn_abi.MAX_K, 'the limit of a list')
    for s, i in parts:
        _on_device(s, 'parts: scores')
        _on_device(i, 'parts: indices')
    s = torch.cat([p[0] for p in parts], dim=1).contiguous()      # one list of sum k_p slots per query: the merge assumes no order
    i = torch.cat([p[1] for p in parts], dim=1).contiguous()
    Q, M = s.shape
    if M > knn_abi.MAX_MERGE:
        raise ValueError(f'parts: {M} slots per query exceed {knn_abi.MAX_MERGE}')
    scores = torch.empty(Q, k, dtype=torch.float32, device=s.device)
    indices = torch.empty(Q, k, dtype=torch.int64, device=s.device)
    knn_abi.run.ecgvit_knn_merge(ptr(s), ptr(i), 1, 0, M, Q, M, k, 0, ptr(scores), ptr(indices), stream())
    return scores, indices
