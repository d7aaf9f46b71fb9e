"""A numpy float64 restatement of the reference's segment tokenizer (ecg_transformer/models/ecg_tokenizer.py): the padder (:88-137), segment means
(:246-247), nearest centre by brute force (the reference asks a KDTree) and one Lloyd update.  Shared by tests/test_tokenizer.py (against the
fixture the reference itself wrote) and tests/test_gpu_tokenizer.py (against the kernels)."""
import numpy as np


def n_pad(l, k):
    return k - (l % k)      # a whole segment when k divides l: the reference's `n_pad == 0` branch never fires


def pad(sig, k, mode):
    """(..., l) -> (..., l + n_pad): 'zero' fills with 0, 'shift' puts sample l - n_pad + j at position l + j"""
    sig = np.asarray(sig)
    l = sig.shape[-1]
    n = n_pad(l, k)
    out = np.zeros(sig.shape[:-1] + (l + n,), sig.dtype)
    out[..., :l] = sig
    if mode == 'shift':
        if l < n:
            raise ValueError(f'shift padding needs l >= n_pad ({l} < {n})')
        out[..., l:] = sig[..., l - n:]
    elif mode != 'zero':
        raise ValueError(mode)
    return out


def segments(sig, k, mode):
    """-> (mean-removed segments (N, k) f64, means (N,) f64), N = prod(leading) * (l // k + 1), in C order"""
    p = pad(np.asarray(sig, np.float64), k, mode)
    segs = p.reshape(-1, k)
    means = segs.mean(axis=-1)
    return segs - means[:, None], means


def sqdist(segs, centers, chunk=4096):
    """(N, V) squared distances, directly as sum (s - c)^2 in f64 -- for small cases"""
    centers = np.asarray(centers, np.float64)
    return np.concatenate([((segs[i:i + chunk, None, :] - centers[None]) ** 2).sum(-1) for i in range(0, len(segs), chunk)])


def nearest(segs, centers, chunk=2048):
    """-> (argmin (N,) int64, its squared distance (N,) f64); ties to the smaller index.  The search runs on |c|^2 - 2 s.c in f64 (every
    term is below 1e-15 relative, far inside the margins the tests allow) and the distance of the winner is recomputed directly."""
    centers = np.asarray(centers, np.float64)
    cn = (centers ** 2).sum(-1)
    ids = np.empty(len(segs), np.int64)
    for i in range(0, len(segs), chunk):
        ids[i:i + chunk] = np.argmin(cn[None, :] - 2.0 * segs[i:i + chunk] @ centers.T, axis=1)
    return ids, ((segs - centers[ids]) ** 2).sum(-1)


def dist_to(segs, centers, ids):
    return ((segs - np.asarray(centers, np.float64)[ids]) ** 2).sum(-1)


def update(segs, ids, centers):
    """one Lloyd update: grouped f64 means; an empty centre keeps its value -> (centers (V, k) f64, lens (V,) int64)"""
    centers = np.array(centers, np.float64)
    V = len(centers)
    lens = np.bincount(ids, minlength=V).astype(np.int64)
    sums = np.zeros_like(centers)
    np.add.at(sums, ids, segs)
    nz = lens > 0
    centers[nz] = sums[nz] / lens[nz, None]
    return centers, lens


def lloyd(segs, init, max_iter=256):
    """assign, stop when no id changed, else update -> (centers, lens, ids, changes per iteration): the loop of EcgTokenizer.fit"""
    centers = np.array(init, np.float64)
    ids = np.full(len(segs), -1, np.int64)
    lens = np.zeros(len(centers), np.int64)
    history = []
    for _ in range(max_iter):
        new, _ = nearest(segs, centers)
        history.append(int((new != ids).sum()))
        ids = new
        if history[-1] == 0:
            break
        centers, lens = update(segs, ids, centers)
    return centers, lens, ids, history
