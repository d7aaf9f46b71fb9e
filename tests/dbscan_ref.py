"""A numpy restatement of the DBSCAN contract of include/ecgvit_hip.h (csrc/dbscan.hip, `EcgTokenizer.dbscan`): the segments in the reference's
flat order with the f32 mean rule, the unfused f32 squared distance, core points by count, components by union under the smaller index, clusters
ranked by their smallest core index, border segments by the smallest label among their core neighbours.  tests/test_dbscan.py holds it to
sklearn.cluster.DBSCAN; tests/test_gpu_dbscan.py holds the kernels to it.  It also reports the band: how close any pair comes to eps."""
import numpy as np
from sklearn.cluster import DBSCAN

import tokenizer_ref as R


def remove_mean32(raw):
    """the header's mean rule in f32: (((x0 + x1) + x2) + ...) * (1 / k) -> (segments minus mean, means)"""
    raw = np.asarray(raw, np.float32)
    k = raw.shape[1]
    s = raw[:, 0].copy()
    for e in range(1, k):
        s = s + raw[:, e]
    mean = s * np.float32(1.0 / k)
    with np.errstate(invalid='ignore'):                  # (inf - inf of a segment with a non-finite sample)
        return raw - mean[:, None], mean


def segments32(recs, k, mode):
    """a list of (C, l_r) float32 records (or an (n, C, L) array) -> (segs (n_total, k) f32, means (n_total,) f32) in the order
    `padded.reshape(-1, k)` record by record: record, then lead, then segment"""
    raw = np.concatenate([R.pad(np.asarray(r, np.float32), k, mode).reshape(-1, k) for r in recs])
    return remove_mean32(raw)


def d2_rows(segs, lo, hi):
    """(hi - lo, n) in the dtype of `segs`: sum_e (a_e - b_e)^2, unfused, in sample order -- every difference, product and addition rounds on
    its own"""
    a, acc = segs[lo:hi], None
    for e in range(segs.shape[1]):
        d = a[:, e][:, None] - segs[:, e][None, :]
        np.multiply(d, d, out=d)
        acc = d if acc is None else np.add(acc, d, out=acc)
    return acc


def eps_squared(eps):
    e = np.float32(eps)
    return np.float32(e * e)


def neighbours(segs32, eps, chunk=512):
    """-> (adjacency (n, n) bool, band): i ~ j iff d2 <= fl32(fl32(eps)^2) (a NaN distance is no neighbour); band = the smallest
    |d - eps| / eps over all pairs with d the f64 distance of the f32 segments (non-finite distances left out)"""
    segs32 = np.ascontiguousarray(segs32, np.float32)
    n, eps2 = len(segs32), eps_squared(eps)
    adj = np.zeros((n, n), bool)
    s64, band = segs32.astype(np.float64), np.inf
    for lo in range(0, n, chunk):
        with np.errstate(invalid='ignore', over='ignore'):
            adj[lo:lo + chunk] = d2_rows(segs32, lo, min(lo + chunk, n)) <= eps2
            d = np.sqrt(d2_rows(s64, lo, min(lo + chunk, n)))
        gap = np.abs(d - float(eps)) / float(eps)
        gap = gap[np.isfinite(gap)]
        if gap.size:
            band = min(band, float(gap.min()))
    return adj, band


def run(segs32, eps, min_samples):
    """-> dict: core (m,) int64 ascending, labels (n,) int64, band, ties (pairs i < j at exactly eps: d2 == eps2 in f32), contested (border
    segments with core neighbours in more than one cluster: the tie the smallest-label rule settles), clusters, noise"""
    adj, band = neighbours(segs32, eps)
    n = len(adj)
    core = np.flatnonzero(adj.sum(axis=1) >= min_samples)
    # union under the smaller index over the core points, in compact (ascending) order: root[x] is the smallest member of x's component so far
    m = len(core)
    sub = adj[np.ix_(core, core)]
    root = np.arange(m)
    for i in range(m):
        below = np.flatnonzero(sub[i, :i])
        if below.size:
            rs = np.unique(root[below])
            root[i] = rs[0]
            for o in rs[1:]:
                root[root == o] = rs[0]
    labels = np.full(n, -1, np.int64)
    core_label = np.unique(root, return_inverse=True)[1]         # ascending root = ascending smallest core index
    labels[core] = core_label
    is_core = np.zeros(n, bool)
    is_core[core] = True
    contested = 0
    for i in np.flatnonzero(~is_core):
        nb = np.flatnonzero(adj[i, core])
        if nb.size:
            labels[i] = core_label[nb].min()
            contested += len(np.unique(core_label[nb])) > 1
    segs32 = np.ascontiguousarray(segs32, np.float32)
    with np.errstate(invalid='ignore', over='ignore'):
        ties = sum(int((np.triu(d2_rows(segs32, lo, min(lo + 512, n)) == eps_squared(eps), lo + 1)).sum()) for lo in range(0, n, 512))
    return dict(core=core.astype(np.int64), labels=labels, band=band, ties=ties, contested=int(contested), clusters=len(np.unique(root)),
                noise=int((labels < 0).sum()))


def dbscan(segs32, eps, min_samples):
    """-> (core_sample_indices, labels), as sklearn.cluster.dbscan returns them"""
    r = run(segs32, eps, min_samples)
    return r['core'], r['labels']


# ---- the stores both test files use --------------------------------------------------------------------
def integer_store(seed, k, plant=False):
    """(n, 12, L) integer samples in -2 .. 2: every segment is one of a few motifs that differ in one or two samples, with a few unit steps on
    top.  plant: the first seven segments of lead 0 are t * u for t in (-2, -2, -1, 0, 1, 2, 2), shuffled, u = +1 +1 -1 -1 on four samples
    (|u| = 2): at eps = 2, min_samples = 4 the segments -u and +u are core points of two clusters and 0 is a border segment of both"""
    rng = np.random.default_rng(seed)
    n, T = int(rng.integers(1, 3)), int(rng.integers(7, 10)) if plant else int(rng.integers(3, 7))
    L = T * k + int(rng.integers(0, k))
    motifs = [rng.integers(-1, 2, k)]
    for _ in range(int(rng.integers(2, 5))):
        m = motifs[int(rng.integers(len(motifs)))].copy()
        for p in rng.choice(k, int(rng.integers(1, 3)), replace=False):
            m[p] = np.clip(m[p] + rng.choice([-1, 1]), -1, 1)
        motifs.append(m)
    x = np.array(motifs)[rng.integers(0, len(motifs), (n, 12, T + 1))].reshape(n, 12, -1)
    step = rng.random(x.shape) < rng.choice([0.02, 0.05, 0.1])
    x = np.clip(x + step * rng.choice([-1, 1], x.shape), -2, 2)
    if plant:
        u = np.zeros(k, np.int64)
        c = rng.choice(k, 4, replace=False)
        u[c[:2]], u[c[2:]] = 1, -1
        x[0, 0, :7 * k] = (rng.permutation(np.array([-2, -2, -1, 0, 1, 2, 2]))[:, None] * u[None, :]).reshape(-1)
    return x[..., :L].astype(np.float32)


def integer_case(seed):
    """-> (k, pad, eps, min_samples, store): k and the padding cycle, eps a half-integer from 1 to 2.5, min_samples 2 to 5; every fourth
    store carries the planted pair of clusters at eps = 2, min_samples = 4"""
    k, mode = (8, 16, 32)[seed % 3], ('zero', 'shift')[(seed // 3) % 2]
    rng = np.random.default_rng(seed + 1000)
    eps, ms = float(rng.integers(2, 6)) / 2, int(rng.integers(2, 6))
    plant = seed % 4 == 0
    if plant:
        eps, ms = 2.0, 4
    return k, mode, eps, ms, integer_store(seed, k, plant)


def random_walk_store(seed, k, shape=(2, 12, 150)):
    rng = np.random.default_rng(seed)
    return np.cumsum(rng.standard_normal(shape) * 0.05, axis=-1).astype(np.float32)


def sklearn_dbscan(segs32, eps, min_samples):
    m = DBSCAN(eps=eps, min_samples=min_samples).fit(np.asarray(segs32, np.float64))
    return m.core_sample_indices_.astype(np.int64), m.labels_.astype(np.int64)
