"""A numpy restatement of the device's k-means++ seeding (include/ecgvit_hip.h, ecgvit_tok_seed): sklearn's greedy `_kmeans_plusplus` with the
first centre and the uniform draws handed in, squared distances as the kernels' unfused f32 chain and every sum an integer.  Shared by
tests/test_tokenizer_seed.py (against sklearn itself) and tests/test_gpu_tokenizer_seed.py (against the kernels).

Segments come in the order g = c * n_seg + p: lead c, position p among that lead's segments in record order."""
import numpy as np

import tokenizer_ref as R


def segments32(sig, k, mode):
    """(n, C, L) float32 records of one length -> ((C * n_seg, k) f32 mean-removed segments in g order, n_seg): the padder of tokenizer_ref.py,
    then the header's mean rule in f32: (((x0 + x1) + x2) + ...) * (1 / k)"""
    p = R.pad(np.asarray(sig, np.float32), k, mode)
    n, C, Lp = p.shape
    raw = np.ascontiguousarray(p.reshape(n, C, Lp // k, k).transpose(1, 0, 2, 3)).reshape(-1, k)
    return remove_mean32(raw), n * (Lp // k)


def ragged_segments32(recs, k, mode):
    """a list of (C, l_r) float32 records of any lengths -> the same"""
    per = [R.pad(np.asarray(r, np.float32), k, mode) for r in recs]
    C = per[0].shape[0]
    raw = np.concatenate([np.concatenate([p[c].reshape(-1, k) for p in per]) for c in range(C)])
    return remove_mean32(raw), len(raw) // C


def remove_mean32(raw):
    raw = np.asarray(raw, np.float32)
    k = raw.shape[1]
    s = raw[:, 0].copy()
    for e in range(1, k):
        s = s + raw[:, e]
    return raw - (s * np.float32(1.0 / k))[:, None]


def d2_chain(cols32, centres32):
    """sum_e (s_e - c_e)^2 in f32, unfused, in sample order: every difference, product and addition rounds on its own.
    cols32: the segments transposed, (k, N) contiguous; centres32: (T, k) -> (T, N)"""
    acc = None
    for e in range(cols32.shape[0]):
        d = cols32[e][None, :] - centres32[:, e][:, None]
        np.multiply(d, d, out=d)
        acc = d if acc is None else np.add(acc, d, out=acc)
    return acc


def exponent(A):
    """E with 2^(E - 1) <= A < 2^E for the f32 maximum A, as the kernels read it off the bit pattern (A = 0 or denormal: -125)"""
    ex = int(np.float32(A).view(np.uint32)) >> 23
    return (ex if ex else 1) - 127 + 1


def fraction_bits(segs32, A=None):
    """F = 63 - H - (2 E + 2 + log2 k): the weight of a squared distance d2 is rint(d2 * 2^F)"""
    N, k = segs32.shape
    if A is None:
        finite = np.where(np.isfinite(segs32), np.abs(segs32), np.float32(0))
        A = finite.max() if not np.isinf(segs32).any() else np.float32(np.inf)
    return 63 - int(N).bit_length() - (2 * exponent(A) + 2 + int(np.log2(k)))


def quant(d2, F):
    """rint(d2 * 2^F) as uint64 (the product is exact in f64); a non-finite distance weighs nothing"""
    d = np.asarray(d2, np.float64)
    ok = np.isfinite(d)
    if not ok.all():
        d = np.where(ok, d, 0.0)
    return np.rint(np.ldexp(d, F)).astype(np.uint64)


def target(U, pot):
    """(U * pot) >> 53 from the high and the low half of the 117-bit product, as the device forms it: uint64 arithmetic only"""
    U, pot = np.uint64(U), np.uint64(pot)
    m = np.uint64(0xFFFFFFFF)
    a1, a0, b1, b0 = U >> np.uint64(32), U & m, pot >> np.uint64(32), pot & m
    p00, p01, p10, p11 = a0 * b0, a0 * b1, a1 * b0, a1 * b1
    mid = (p00 >> np.uint64(32)) + (p01 & m) + (p10 & m)
    hi = p11 + (p01 >> np.uint64(32)) + (p10 >> np.uint64(32)) + (mid >> np.uint64(32))
    lo = (p00 & m) | ((mid & m) << np.uint64(32))
    return int((hi << np.uint64(11)) | (lo >> np.uint64(53)))


def u53(u):
    """floor(u * 2^53): exact for the multiples of 2^-53 that Generator.random returns"""
    return np.floor(np.asarray(u, np.float64) * 2.0 ** 53).astype(np.uint64)


def u_for(q, g):
    """a U whose target lands on segment g (of non-zero weight q[g]): the smallest with (U * pot) >> 53 >= the running sum before g"""
    q = [int(v) for v in q]
    pot, before = sum(q), sum(q[:g])
    U = -(-(before << 53) // pot)
    assert q[g] > 0 and U < 2 ** 53 and before <= (U * pot) >> 53 < before + q[g]
    return U


def seed(segs32, V, first, U53, T, A=None, plan=None):
    """-> (indices (V,) int64, candidates (V - 1, T) int64, potentials (V - 1, T) uint64, F).  U53: (V - 1, T) uint64, or None with
    plan(c, q) -> the T values of step c, chosen on the weights q the step draws from (they are written into the returned `plan.rows`)"""
    segs32 = np.asarray(segs32, np.float32)
    N = len(segs32)
    F = fraction_bits(segs32, A)
    U53 = np.zeros((max(V - 1, 0), T), np.uint64) if U53 is None else np.array(U53, np.uint64).reshape(max(V - 1, 0), T)
    inf = np.float32(np.inf)
    cols = np.ascontiguousarray(segs32.T)
    d = d2_chain(cols, segs32[[first]])[0]
    closest = np.where(d < inf, d, inf)                 # a NaN distance leaves +inf: weight 0
    q = quant(closest, F)
    indices, cands, pots = [int(first)], np.zeros((max(V - 1, 0), T), np.int64), np.zeros((max(V - 1, 0), T), np.uint64)
    for c in range(1, V):
        pot = int(q.sum(dtype=np.uint64))
        assert pot < 2 ** 63
        if plan is not None:
            U53[c - 1] = np.asarray(plan(c, q), np.uint64)
        cum = np.cumsum(q, dtype=np.uint64)
        tg = np.array([target(U53[c - 1, t], pot) for t in range(T)], np.uint64)
        g = np.searchsorted(cum, tg, side='right') if pot else np.zeros(T, np.int64)      # the smallest g whose running sum exceeds the target
        assert int(g.max()) < N
        d = d2_chain(cols, segs32[g])
        new = np.where(d < closest[None, :], d, closest[None, :])
        qn = quant(new, F)
        cands[c - 1], pots[c - 1] = g, qn.sum(axis=1, dtype=np.uint64)
        win = int(np.argmin(pots[c - 1]))                # ties go to the smaller trial index
        closest, q = new[win], qn[win]
        indices.append(int(g[win]))
    if plan is not None:
        plan.rows = U53
    return np.array(indices, np.int64), cands, pots, F
