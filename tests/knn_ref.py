"""numpy restatement of include/ecgvit_hip_knn.h: f64 scores, the total order (score descending, bank index ascending) by `np.lexsort`, the
merge, the normalisation and the vote.  A plain module: tests/test_knn.py holds it to torch.topk and to scikit-learn's brute-force search,
tests/test_gpu_knn.py holds the device to it."""
import numpy as np


def scores64(queries, bank):
    with np.errstate(invalid='ignore', over='ignore'):
        return np.asarray(queries, np.float64) @ np.asarray(bank, np.float64).T


def select(s, k, self_base=-1, index_base=0):
    """s: (Q, N) scores -> (scores (Q, k) in s's dtype, indices (Q, k) int64): per query the first k admissible rows (finite score, not row
    self_base + q) under (score descending, index ascending); -inf / -1 in the slots that are left"""
    Q, N = s.shape
    out_s = np.full((Q, k), -np.inf, s.dtype)
    out_i = np.full((Q, k), -1, np.int64)
    for q in range(Q):
        ok = np.isfinite(s[q])
        if self_base >= 0 and 0 <= self_base + q < N:
            ok[self_base + q] = False
        rows = np.flatnonzero(ok)
        order = rows[np.lexsort((rows, -s[q, rows]))][:k]
        out_s[q, :len(order)] = s[q, order]
        out_i[q, :len(order)] = order + index_base
    return out_s, out_i


def search(queries, bank, k, self_base=-1, index_base=0):
    return select(scores64(queries, bank), k, self_base, index_base)


def merge(parts, k):
    """parts: [(scores (Q, k_p), indices (Q, k_p))] -> the first k distinct pairs with a non-negative index and a finite score"""
    s = np.concatenate([p[0] for p in parts], axis=1)
    i = np.concatenate([p[1] for p in parts], axis=1)
    Q = s.shape[0]
    out_s = np.full((Q, k), -np.inf, s.dtype)
    out_i = np.full((Q, k), -1, np.int64)
    for q in range(Q):
        pairs = sorted({(-float(a), int(b)) for a, b in zip(s[q], i[q]) if b >= 0 and np.isfinite(a)})[:k]
        out_s[q, :len(pairs)] = [-a for a, _ in pairs]
        out_i[q, :len(pairs)] = [b for _, b in pairs]
    return out_s, out_i


def normalize(x):
    """fl32(x * (1 / sqrt(sum x^2))) in f64; a zero row stays zero"""
    x = np.asarray(x, np.float64)
    with np.errstate(invalid='ignore', over='ignore', divide='ignore'):
        n2 = (x * x).sum(axis=1, keepdims=True)
        inv = np.where(n2 == 0, 0.0, 1.0 / np.sqrt(n2))
        return (x * inv).astype(np.float32)


def vote(scores, indices, labels, weights='softmax', temperature=0.07):
    """out[q][c] = sum_j w_j y[idx_j][c] / sum_j w_j in f64 over j ascending, stored as f32; slots outside [0, N) skipped; no slot: 0"""
    Q, k = scores.shape
    N, K = labels.shape
    y = np.asarray(labels, np.float64)
    out = np.zeros((Q, K), np.float32)
    for q in range(Q):
        keep = [j for j in range(k) if 0 <= indices[q, j] < N]
        if not keep:
            continue
        s0 = max(np.float64(scores[q, j]) for j in keep)
        num, den = np.zeros(K, np.float64), np.float64(0.0)
        for j in keep:
            w = np.float64(1.0) if weights == 'uniform' else np.exp((np.float64(scores[q, j]) - s0) / np.float64(temperature))
            num = num + w * y[indices[q, j]]
            den = den + w
        out[q] = (num / den).astype(np.float32)
    return out


def integer_store(rng, rows, d):
    """small integers in [-8, 8] as f32: with d <= 2048 every partial sum of a product stays below 2^24, so every summation order, f32 or
    f64, gives the same score, and ties abound"""
    return rng.integers(-8, 9, (rows, d)).astype(np.float32)
