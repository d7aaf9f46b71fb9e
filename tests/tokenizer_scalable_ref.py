"""A numpy restatement of the device's scalable k-means++ seeding (include/ecgvit_hip_tok_scalable.h, ecgvit_tok_scalable_seed): k-means||
(Bahmani et al. 2012) with the draws handed in, squared distances as the kernels' unfused f32 chain and every sum an integer.  Shared by
tests/test_tokenizer_scalable.py (the recluster against sklearn, the rule against Python integers) and tests/test_gpu_tokenizer_scalable.py
(against the kernels).  Segments come in the order g = c * n_seg + p, as in tokenizer_seed_ref.py."""
import math

import numpy as np

from tokenizer_seed_ref import d2_chain, quant, target, fraction_bits

M64 = np.uint64(0xFFFFFFFFFFFFFFFF)
GOLDEN, MUL1, MUL2 = np.uint64(0x9E3779B97F4A7C15), np.uint64(0xBF58476D1CE4E5B9), np.uint64(0x94D049BB133111EB)


def _u(n):
    return np.uint64(n)


def mix(key, g):
    """splitmix64's finaliser of key + g * golden (mod 2^64), over an array of g -> uint64"""
    with np.errstate(over='ignore'):
        z = np.uint64(key) + np.asarray(g, np.uint64) * GOLDEN
        z = (z ^ (z >> _u(30))) * MUL1
        z = (z ^ (z >> _u(27))) * MUL2
        return z ^ (z >> _u(31))


def mul128(a, b):
    """(high, low) 64-bit halves of the product of uint64 arrays, from 32-bit limbs: uint64 arithmetic only"""
    a, b = np.asarray(a, np.uint64), np.asarray(b, np.uint64)
    m = _u(0xFFFFFFFF)
    a1, a0, b1, b0 = a >> _u(32), a & m, b >> _u(32), b & m
    p00, p01, p10, p11 = a0 * b0, a0 * b1, a1 * b0, a1 * b1
    mid = (p00 >> _u(32)) + (p01 & m) + (p10 & m)
    hi = p11 + (p01 >> _u(32)) + (p10 >> _u(32)) + (mid >> _u(32))
    lo = (p00 & m) | ((mid & m) << _u(32))
    return hi, lo


def selected(u, pot, ell, q):
    """q > 0 and ((u * pot) >> 53) < ell * q, for arrays u (< 2^53) and q and scalars pot (< 2^63) and ell: the left side from the 117-bit
    product, the right side a 128-bit product"""
    q = np.asarray(q, np.uint64)
    hi, lo = mul128(u, _u(pot))
    lhs = (hi << _u(11)) | (lo >> _u(53))
    rhi, rlo = mul128(q, _u(ell))
    return (q > 0) & ((rhi != 0) | (lhs < rlo))


def cap_of(ell):
    return ell + 8 * (math.isqrt(ell - 1) + 1)


def fold(cols, rows, j0, closest, owner, chunk=64):
    """rows j0, j0 + 1, ... in order against every segment, in place: a strict <, so the smaller row wins a tie; a NaN distance changes nothing"""
    inf = np.float32(np.inf)
    for lo in range(0, len(rows), chunk):
        d = d2_chain(cols, rows[lo:lo + chunk])
        d = np.where(d == d, d, inf)
        am = d.argmin(axis=0)                              # the first of equal minima: the smaller row
        m = d[am, np.arange(d.shape[1])]
        upd = m < closest
        closest[upd] = m[upd]
        owner[upd] = j0 + lo + am[upd]


def recluster(rows32, w, V, u0, U53, T, F):
    """weighted greedy k-means++ over the rows of a table -> (the chosen rows' indices (V,), candidates (V - 1, T), potentials (V - 1, T) uint64).
    Every weight is w_j * q(d2(row_j, nearest chosen row)); centre 0 is the smallest j whose running sum of w exceeds (u0 * sum w) >> 53"""
    rows32, w = np.asarray(rows32, np.float32), np.asarray(w, np.uint64)
    U53 = np.asarray(U53, np.uint64).reshape(max(V - 1, 0), T)
    cols = np.ascontiguousarray(rows32.T)
    inf = np.float32(np.inf)
    wsum = int(w.sum(dtype=np.uint64))
    j0 = int(np.searchsorted(np.cumsum(w, dtype=np.uint64), np.uint64(target(u0, wsum)), side='right')) if wsum else 0
    d = d2_chain(cols, rows32[[j0]])[0]
    closest = np.where(d < inf, d, inf)
    wq = w * quant(closest, F)
    chosen, cands, pots = [j0], np.zeros((max(V - 1, 0), T), np.int64), np.zeros((max(V - 1, 0), T), np.uint64)
    for c in range(1, V):
        pot = int(wq.sum(dtype=np.uint64))
        assert pot < 2 ** 63
        tg = np.array([target(U53[c - 1, t], pot) for t in range(T)], np.uint64)
        j = np.searchsorted(np.cumsum(wq, dtype=np.uint64), tg, side='right') if pot else np.zeros(T, np.int64)
        d = d2_chain(cols, rows32[j])
        new = np.where(d < closest[None, :], d, closest[None, :])
        wqn = w[None, :] * quant(new, F)
        cands[c - 1], pots[c - 1] = j, wqn.sum(axis=1, dtype=np.uint64)
        win = int(np.argmin(pots[c - 1]))                # ties go to the smaller trial index
        closest, wq = new[win], wqn[win]
        chosen.append(int(j[win]))
    return np.array(chosen, np.int64), cands, pots


def potential(segs32, centres32, F):
    """the full-store potential of a set of centres: sum_g q(min_j d2(s_g, c_j))"""
    cols = np.ascontiguousarray(np.asarray(segs32, np.float32).T)
    closest = np.full(cols.shape[1], np.inf, np.float32)
    fold(cols, np.asarray(centres32, np.float32), 0, closest, np.zeros(cols.shape[1], np.int64))
    return int(quant(closest, F).sum(dtype=np.uint64))


def seed(segs32, V, ell, R, T, first, keys, u0, U53, cap=None, A=None):
    """the whole seeding -> dict: rounds (the g appended by each round, ascending), selected, truncated, pots (R,) uint64, potential (after the
    last fold), cand_g, weights, closest, owner, n_c, F and -- when n_c >= V -- chosen (table rows), indices (their g), centers"""
    segs32 = np.asarray(segs32, np.float32)
    N = len(segs32)
    cap = cap_of(ell) if cap is None else cap
    F = fraction_bits(segs32, A)
    cols = np.ascontiguousarray(segs32.T)
    g_all = np.arange(N, dtype=np.uint64)
    closest, owner = np.full(N, np.inf, np.float32), np.full(N, -1, np.int64)
    cand_g, folded = [int(first)], 0
    out = dict(rounds=[], selected=[], truncated=[], pots=[], F=F)
    for r in range(R):
        fold(cols, segs32[cand_g[folded:]], folded, closest, owner)
        folded = len(cand_g)
        q = quant(closest, F)
        pot = int(q.sum(dtype=np.uint64))
        assert pot < 2 ** 63
        take = np.flatnonzero(selected(mix(keys[r], g_all) >> _u(11), pot, ell, q)) if pot else np.zeros(0, np.int64)
        out['pots'].append(pot)
        out['selected'].append(len(take))
        out['truncated'].append(len(take) - min(len(take), cap))
        out['rounds'].append(take[:cap].astype(np.int64))
        cand_g += take[:cap].tolist()
    fold(cols, segs32[cand_g[folded:]], folded, closest, owner)
    n_c = len(cand_g)
    out.update(pots=np.array(out['pots'], np.uint64), selected=np.array(out['selected'], np.int64), truncated=np.array(out['truncated'], np.int64),
               potential=int(quant(closest, F).sum(dtype=np.uint64)), cand_g=np.array(cand_g, np.int64), closest=closest, owner=owner, n_c=n_c,
               weights=np.bincount(owner[owner >= 0], minlength=n_c).astype(np.int64))
    assert np.array_equal(owner >= 0, np.isfinite(closest))
    if n_c >= V:
        table = segs32[out['cand_g']]
        chosen, _, _ = recluster(table, out['weights'], V, u0, U53, T, F)
        out.update(chosen=chosen, indices=out['cand_g'][chosen], centers=table[chosen])
    return out
