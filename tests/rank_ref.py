"""numpy restatement of include/ecgvit_hip_rank.h: the 32-bit monotone key, the order (key ascending, record index ascending) by `np.lexsort`, the
tie groups, the weighted rank sum in int64, the counter-based generator and the multiplicities.  A plain module: tests/test_rank_metrics.py holds
it to scikit-learn and to the oracle's all-pairs counts on the CPU, tests/test_gpu_rank_metrics.py holds the kernels to it, integer by integer."""
import numpy as np

NAN_KEY = np.uint32(0xFFFFFFFF)
M64 = (1 << 64) - 1
GAMMA = 0x9E3779B97F4A7C15


def as_prob(scores, from_logits):
    """f32 in, f32 out; the logistic form in f32 as csrc/metrics_common.h writes it (the device's expf may differ from numpy's in the last
    bit: the GPU tests that compare orders under from_logits use scores on which that cannot change an order, or compare counts with the
    all-pairs kernel, which shares the device's expression)"""
    s = np.asarray(scores, np.float32)
    if not from_logits:
        return s
    with np.errstate(over='ignore'):
        return (np.float32(1) / (np.float32(1) + np.exp(-s, dtype=np.float32))).astype(np.float32)


def keys(p):
    """f32 probabilities -> uint32 keys: NaN the largest, -0 and +0 one key, else the float order"""
    p = np.array(p, np.float32)
    nan = np.isnan(p)
    p[p == 0] = 0.0
    b = p.view(np.uint32)
    k = np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000)).astype(np.uint32)
    return np.where(nan, NAN_KEY, k)


def order(key):
    """the permutation under (key ascending, record index ascending)"""
    return np.lexsort((np.arange(len(key)), key))


def packed(key, y):
    """the word of every sorted position: record index | label bit << 30 | last-of-tie-group bit << 31, and the first NaN position"""
    o = order(key)
    s = key[o]
    last = np.r_[s[1:] != s[:-1], True]
    word = o.astype(np.uint32) | (np.asarray(y)[o] != 0).astype(np.uint32) << np.uint32(30) | last.astype(np.uint32) << np.uint32(31)
    nan = np.flatnonzero(s == NAN_KEY)
    return word, int(nan[0]) if len(nan) else len(key)


def rank_sum(key, y, w=None):
    """(num2, wp, wn) of one class: num2 = sum over positives t of w_t (Cn[before t's tie group] + Cn[end of t's tie group]), Cn the running
    sum of the negatives' weights in sorted order; a record with NaN's key adds nothing to num2 and counts in wp / wn"""
    n = len(key)
    w = np.ones(n, np.int64) if w is None else np.asarray(w, np.int64)
    o = order(key)
    s, yy, ww = key[o], np.asarray(y)[o] != 0, w[o]
    wp, wn = int(ww[yy].sum()), int(ww[~yy].sum())
    ww = np.where(s == NAN_KEY, 0, ww)
    start = np.r_[True, s[1:] != s[:-1]]
    gid = np.cumsum(start) - 1
    cn = np.cumsum(np.where(yy, 0, ww))
    gs = np.flatnonzero(start)
    ge = np.r_[gs[1:], n] - 1
    below, upto = np.r_[0, cn][gs][gid], cn[ge][gid]
    return int((np.where(yy, ww, 0) * (below + upto)).sum()), wp, wn


def triples(probs, labels, mult=None):
    """(R, K, 3) int64 for (R, n) multiplicities (None: one row of ones)"""
    n, K = probs.shape
    mult = np.ones((1, n), np.int64) if mult is None else np.asarray(mult)
    ks = [keys(probs[:, c]) for c in range(K)]
    return np.array([[rank_sum(ks[c], labels[:, c], m) for c in range(K)] for m in mult], np.int64)


def mix(z):
    z = np.asarray(z, dtype=np.uint64)
    with np.errstate(over='ignore'):
        z = z ^ (z >> np.uint64(30))
        z = z * np.uint64(0xBF58476D1CE4E5B9)
        z = z ^ (z >> np.uint64(27))
        z = z * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def mix_int(z):
    """the same finaliser on a Python integer: the generator once more, without numpy's wrapping arithmetic"""
    z ^= z >> 30
    z = z * 0xBF58476D1CE4E5B9 & M64
    z ^= z >> 27
    z = z * 0x94D049BB133111EB & M64
    return z ^ z >> 31


def draw_int(seed, r, j, n):
    return mix_int((mix_int((seed + GAMMA * (r + 1)) & M64) + GAMMA * (j + 1)) & M64) * n >> 64


def draws(seed, r, n):
    """(n,) int64 draws of replicate r: index = (mix(mix(seed + G (r + 1)) + G (j + 1)) * n) >> 64"""
    with np.errstate(over='ignore'):
        key = mix(np.uint64((seed + GAMMA * (r + 1)) & M64))
        u = mix(key + np.uint64(GAMMA) * np.arange(1, n + 1, dtype=np.uint64))
        hi, lo = u >> np.uint64(32), u & np.uint64(0xFFFFFFFF)
        return ((hi * np.uint64(n) + ((lo * np.uint64(n)) >> np.uint64(32))) >> np.uint64(32)).astype(np.int64)


def multiplicities(seed, r, n):
    return np.bincount(draws(seed, r, n), minlength=n).astype(np.int64)


def from_indices(idx, n):
    return np.stack([np.bincount(row, minlength=n) for row in np.asarray(idx)]).astype(np.int64)


# ---- the stores of the GPU tests --------------------------------------------------------------------------------------------------------------
def labels_for(rng, n, K):
    """multi-hot labels at mixed rates; both label values in every class when n >= 2"""
    y = (rng.random((n, K)) < rng.choice([0.5, 0.2, 0.05], K)).astype(np.float32)
    if n >= 2:
        y[0], y[n - 1] = 1, 0
    return y


def store(kind, rng, n, K):
    """(n, K) f32 scores of one kind"""
    if kind == 'grid':                      # ties across tile borders
        return (rng.integers(0, 17, (n, K)) / 16).astype(np.float32)
    if kind == 'equal':
        return np.full((n, K), 0.25, np.float32)
    if kind == 'distinct':                  # negatives, +-0, +-inf, denormals among distinct normals
        s = rng.standard_normal((n, K)).astype(np.float32)
        special = np.array([0.0, -0.0, np.inf, -np.inf, 1e-45, -1e-45, 1e-40, -3e-39, 1.17549435e-38, -1.0, 1.0], np.float32)
        for c in range(K):
            at = rng.permutation(n)[:min(n, len(special))]
            s[at, c] = special[:len(at)]
        return s
    if kind.startswith('byte'):             # bit patterns that differ in one byte only: one digit pass does all the work
        b = int(kind[4:])
        base = np.uint32(0x3F000000 if b < 3 else 0x00112233)
        v = (rng.integers(0, 256 if b < 3 else 0x7F, (n, K)).astype(np.uint32) << np.uint32(8 * b))
        return ((base & ~np.uint32(0xFF << 8 * b)) | v).astype(np.uint32).view(np.float32)
    if kind == 'nan':
        s = (rng.integers(0, 9, (n, K)) / 8).astype(np.float32)
        s[rng.random((n, K)) < 0.2] = np.nan
        return s
    raise ValueError(kind)


KINDS = ('grid', 'equal', 'distinct', 'byte0', 'byte1', 'byte2', 'byte3', 'nan')
