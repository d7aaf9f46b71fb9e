"""CPU: the restatement of the device's scalable k-means++ seeding (tests/tokenizer_scalable_ref.py) -- its weighted recluster against
`sklearn.cluster.kmeans_plusplus(sample_weight=)` fed the same draws, its selection rule and mixer against Python integers, its quality against
the k-means++ restatement -- and the host contract of `EcgTokenizer.kmeans_parallel` / `ScalableKMeansPlusPlus`: every refusal, the binding
table against include/ecgvit_hip_tok_scalable.h, the kernels' register budgets from the code objects.  No GPU is touched."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT
import abi_header
import ecg_representation_learning_amd as E
from ecg_representation_learning_amd import hip, tokenizer, tok_scalable_abi as A
import tokenizer_seed_ref as S
import tokenizer_scalable_ref as P
from test_tokenizer_seed import FedRandomState

HEADER = os.path.join(ROOT, 'include', 'ecgvit_hip_tok_scalable.h')


def fraction_bits(rows32, total):
    """F for a table whose weights sum to `total`: H = bit_length(total) keeps every weighted potential below 2^63"""
    k = rows32.shape[1]
    return 63 - int(total).bit_length() - (2 * S.exponent(np.abs(rows32).max()) + 2 + int(np.log2(k)))


# ---- the weighted recluster against sklearn ----------------------------------------------------------------
def recluster_case(i):
    """a random walk cut into 600 rows of k samples, weights 0 .. 1999 with twenty zeros"""
    k = (8, 16, 32)[i % 3]
    rng = np.random.default_rng(7000 + i)
    rows = S.remove_mean32(np.cumsum(rng.standard_normal(600 * k)).astype(np.float32).reshape(600, k))
    w = rng.integers(0, 2000, 600)
    w[rng.choice(600, 20, replace=False)] = 0
    return rows, w.astype(np.int64), int(S.u53(rng.random())), rng.random((47, 5))


def test_weighted_recluster_draws_what_sklearn_draws():
    cluster = pytest.importorskip('sklearn.cluster')
    from threadpoolctl import threadpool_limits
    bad = []
    for i in range(40):
        rows, w, u0, u = recluster_case(i)
        assert (w == 0).sum() >= 20 and w.max() <= 1999
        chosen, _, _ = P.recluster(rows, w, 48, u0, S.u53(u), 5, fraction_bits(rows, w.sum()))
        assert w[chosen[0]] > 0 and w[:chosen[0]].sum() <= (u0 * int(w.sum())) >> 53 < w[:chosen[0] + 1].sum()
        with threadpool_limits(1):
            _, want = cluster.kmeans_plusplus(rows.astype(np.float64), 48, sample_weight=w.astype(np.float64),
                                              random_state=FedRandomState(chosen[0], u), n_local_trials=5)
        if not np.array_equal(chosen, want):
            bad.append((i, int(np.flatnonzero(chosen != want)[0])))
    assert not bad, bad


@pytest.mark.parametrize('k', [8, 16, 32])
def test_recluster_with_unit_weights_is_the_kmeans_plusplus_restatement(k):
    rng = np.random.default_rng(k)
    sig = np.cumsum(rng.standard_normal((2, 12, 1501)), axis=-1).astype(np.float32)
    segs, _ = S.segments32(sig, k, 'shift')
    N, V, T = len(segs), 20, 4
    first, U = int(rng.integers(N)), S.u53(rng.random((V - 1, T)))
    want, want_c, want_p, F = S.seed(segs, V, first, U, T)
    ones = np.ones(N, np.int64)
    chosen, cands, pots = P.recluster(segs, ones, V, S.u_for(ones, first), U, T, F)
    assert chosen[0] == first and np.array_equal(chosen, want) and np.array_equal(cands, want_c) and np.array_equal(pots, want_p)


# ---- the selection rule and the mixer against Python integers ---------------------------------------------------
def mix_int(key, g):
    m = 2 ** 64 - 1
    z = (key + g * 0x9E3779B97F4A7C15) & m
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & m
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & m
    return z ^ (z >> 31)


def test_mixer_is_splitmix64s_finaliser():
    rng = np.random.default_rng(64)
    keys = [0, 1, 2 ** 64 - 1, 0x9E3779B97F4A7C15] + rng.integers(0, 2 ** 64, 6, dtype=np.uint64).tolist()
    g = np.concatenate([np.arange(5), [2 ** 31 - 1, 2 ** 31, 2 ** 32 - 1], rng.integers(0, 2 ** 32, 50)]).astype(np.uint64)
    for key in keys:
        got = P.mix(key, g)
        assert got.dtype == np.uint64 and got.tolist() == [mix_int(int(key), int(v)) for v in g]
    assert mix_int(0, 0) == 0 and mix_int(0, 1) == 0xE220A8397B1DCDAF      # splitmix64's first output from state 0
    u = P.mix(12345, np.arange(200000)) >> np.uint64(11)
    assert int(u.max()) < 2 ** 53 and abs(float(u.mean()) / 2.0 ** 53 - 0.5) < 0.005


def take_int(u, pot, ell, q):
    return q > 0 and ((u * pot) >> 53) < ell * q


def test_selection_rule_is_the_integer_comparison():
    top = 2 ** 53 - 1
    cases = []
    for pot in (2 ** 63 - 1, 2 ** 62 + 12345, 3 ** 39, 2 ** 53 + 1, 1000, 1):
        for ell in (1, 2, 128, 65536):
            for q in (0, 1, 2, pot // (3 * ell) + 1, pot // ell, min(pot, 2 ** 60)):
                if q > pot:
                    continue
                edge = -(-(ell * q << 53) // pot)                # the smallest u with (u pot) >> 53 >= ell q: both sides of the boundary
                for u in (0, 1, top, edge - 1, edge, edge + 1):
                    if 0 <= u <= top:
                        cases.append((u, pot, ell, q))
    rng = np.random.default_rng(5)
    for _ in range(2000):
        pot = int(rng.integers(1, 2 ** 63))
        cases.append((int(rng.integers(0, 2 ** 53)), pot, int(rng.integers(1, 65537)), int(rng.integers(0, min(pot, 2 ** 61) + 1))))
    seen = set()
    for u, pot, ell, q in cases:
        got = bool(P.selected(np.array([u], np.uint64), pot, ell, np.array([q], np.uint64))[0])
        assert got == take_int(u, pot, ell, q), (u, pot, ell, q)
        seen.add((got, ell * q >= 2 ** 64, q == 0))
    assert {(True, True, False), (True, False, False), (False, False, False), (False, False, True)} <= seen      # both outcomes, a 128-bit right side, q = 0
    boundary = [(u, pot, ell, q) for u, pot, ell, q in cases if q and take_int(u, pot, ell, q) != take_int(u + 1, pot, ell, q)]
    assert len(boundary) >= 20                                   # u and u + 1 on either side of the comparison
    # ell q >= pot: taken whatever u is; q = 0: never; pot = 0 leaves no positive q, and the restatement's rounds then take nothing
    assert P.selected(np.array([top], np.uint64), 1000, 10, np.array([100], np.uint64))[0]
    assert not P.selected(np.array([0], np.uint64), 1000, 10, np.array([0], np.uint64))[0]
    assert not P.selected(np.array([0], np.uint64), 0, 10, np.array([0], np.uint64))[0]
    for a, b in [(2 ** 64 - 1, 2 ** 64 - 1), (2 ** 53 - 1, 2 ** 63 - 1), (65536, 2 ** 60), (0, 5)]:
        hi, lo = P.mul128(np.uint64(a), np.uint64(b))
        assert (int(hi) << 64) | int(lo) == a * b


def test_rounds_end_when_the_potential_is_zero():
    segs = np.zeros((300, 8), np.float32)
    r = P.seed(segs, 1, 4, 3, 2, 7, np.array([1, 2, 3], np.uint64), 0, np.zeros((0, 2), np.uint64))
    assert r['n_c'] == 1 and r['pots'].tolist() == [0, 0, 0] and r['selected'].tolist() == [0, 0, 0] and r['weights'].tolist() == [300]
    assert r['indices'].tolist() == [7] and not r['owner'].any()
    assert 'indices' not in P.seed(segs, 2, 4, 3, 2, 7, np.array([1, 2, 3], np.uint64), 0, np.zeros((1, 2), np.uint64))


# ---- quality: the selection rule in simulation ---------------------------------------------------------------
def walk_store(seed):
    """3 x 12 random-walk leads of 9 999 samples: 45 000 segments at k = 8"""
    return np.cumsum(np.random.default_rng(seed).standard_normal((3, 12, 9999)), axis=-1).astype(np.float32)


@pytest.mark.parametrize('seed', [0, 1, 2])
def test_potential_against_the_kmeans_plusplus_restatement(seed):
    """k = 8, V = 64, ell = 128, 5 rounds, T = 6, the draws in the public call's order.  Both seedings are random draws, hence the margin of
    1.10 on the ratio of the full-store potentials; every round stays within the cap of 224 and no candidate is left without weight"""
    V, R, T, ell = 64, 5, 6, 128
    segs, _ = S.segments32(walk_store(seed), 8, 'shift')
    N = len(segs)
    assert N == 45000 and P.cap_of(ell) == 224
    first, keys, u0, U = E.EcgTokenizer._scalable_draws(np.random.default_rng(seed), N, V, T, R)
    r = P.seed(segs, V, ell, R, T, first, keys, u0, U)
    plus = S.seed(segs, V, first, U, T)[0]
    ratio = P.potential(segs, r['centers'], r['F']) / P.potential(segs, segs[plus], r['F'])
    print(f'seed {seed}: selected per round {r["selected"].tolist()}, n_c = {r["n_c"]}, zero-weight candidates {int((r["weights"] == 0).sum())}, '
          f'potential / k-means++ potential = {ratio:.3f}')
    assert r['selected'].max() <= 224 and not r['truncated'].any()
    assert r['n_c'] == 1 + r['selected'].sum() and r['weights'].sum() == N and r['weights'].min() >= 1
    assert len(set(r['indices'].tolist())) == V
    assert ratio <= 1.10


# ---- host contract -----------------------------------------------------------------------------------------------
def test_exports_defaults_and_the_draw_order():
    assert E.ScalableKMeansPlusPlus is tokenizer.ScalableKMeansPlusPlus and 'ScalableKMeansPlusPlus' in E.__all__
    s = E.ScalableKMeansPlusPlus()
    assert (s.oversampling_factor, s.n_rounds, s.n_local_trials) == (2.0, 5, None) and not isinstance(s, E.KMeansPlusPlus)
    assert s.plan(64) == (6, 5, 128, 224) and E.ScalableKMeansPlusPlus(1.5, 3, 4).plan(37) == (4, 3, 56, 56 + 8 * 8)
    assert [tokenizer.scalable_cap(e) for e in (1, 2, 4, 5, 16, 17, 128)] == [9, 18, 20, 29, 48, 57, 224] == [P.cap_of(e) for e in (1, 2, 4, 5, 16, 17, 128)]
    rng, again = np.random.default_rng(9), np.random.default_rng(9)
    first, keys, u0, U = E.EcgTokenizer._scalable_draws(rng, 1000, 5, 3, 4)
    assert first == int(again.integers(1000)) and np.array_equal(keys, again.integers(0, 2 ** 64, size=4, dtype=np.uint64))
    assert u0 == int(S.u53(again.random())) and np.array_equal(U, S.u53(again.random((4, 3)))) and keys.dtype == np.uint64


def test_argument_refusals_come_before_a_device_is_asked_for():
    t = E.EcgTokenizer()
    x = torch.zeros(2, 12, 64)                                   # 216 segments, on the host
    for bad in (0, -1.0, float('inf'), float('nan'), 'two', None, True):
        with pytest.raises(ValueError, match='oversampling_factor'):
            E.ScalableKMeansPlusPlus(oversampling_factor=bad)
        with pytest.raises(ValueError, match='oversampling_factor'):
            t.kmeans_parallel(x, 4, oversampling_factor=bad)
    for bad in (0, 17, -1, 2.0, None, True):
        with pytest.raises(ValueError, match='n_rounds'):
            E.ScalableKMeansPlusPlus(n_rounds=bad)
        with pytest.raises(ValueError, match='n_rounds'):
            t.kmeans_parallel(x, 4, n_rounds=bad)
    for bad in (0, 17, -1):
        with pytest.raises(ValueError, match='n_local_trials'):
            E.ScalableKMeansPlusPlus(n_local_trials=bad)
        with pytest.raises(ValueError, match='n_local_trials'):
            t.kmeans_parallel(x, 4, n_local_trials=bad)
    for bad in (0, 65537):
        with pytest.raises(ValueError, match='n_clusters'):
            t.kmeans_parallel(x, bad)
    with pytest.raises(ValueError, match='exceeds the 216 segments'):
        t.kmeans_parallel(x, 217)
    with pytest.raises(ValueError, match='device'):
        t.kmeans_parallel(x, 4, random_state=0)
    with pytest.raises(ValueError, match='device'):
        t.fit(x, cls_kwargs=dict(n_clusters=4, init=E.ScalableKMeansPlusPlus(), n_init=2, random_state=0))
    with pytest.raises(ValueError, match='exceeds the 216 segments'):
        t.fit(x, cls_kwargs=dict(n_clusters=217, init=E.ScalableKMeansPlusPlus()))
    with pytest.raises(NotImplementedError, match='random'):     # the string stays refused exactly as it was
        t.fit(x, cls_kwargs=dict(n_clusters=4, init='scalable-k-means++'))


def test_cap_and_table_size_refusals():
    """1 + n_rounds * cap rows must fit a table of 65 536: held on the host, before the store is looked at"""
    t = E.EcgTokenizer()
    x = torch.zeros(2, 12, 64)
    assert E.ScalableKMeansPlusPlus(2.0, 5).plan(6000)[3] == 12000 + 8 * 110        # 1 + 5 * 12 880 = 64 401 rows
    for kw in (dict(n_clusters=6200), dict(n_clusters=4096, n_rounds=8), dict(n_clusters=1000, oversampling_factor=70.0),
               dict(n_clusters=4, _cap=0), dict(n_clusters=4, _cap=13108)):
        with pytest.raises(ValueError, match='a table holds at most 65536'):
            t.kmeans_parallel(x, **kw)
    with pytest.raises(ValueError, match='a table holds at most 65536'):
        t.fit(x, cls_kwargs=dict(n_clusters=4096, init=E.ScalableKMeansPlusPlus(n_rounds=8)))
    with pytest.raises(ValueError, match='device'):                               # 1 + 5 * 13 107 = 65 536 rows are a table
        t.kmeans_parallel(x, 4, _cap=13107)
    w = A.lib().ecgvit_tok_scalable_workspace
    assert w(12, 1000, 50, 8, 5, 5, 13107) > 0 and w(12, 1000, 50, 8, 5, 5, 13108) == 0
    assert w(12, 1000, 50, 8, 5, 5, 200) > 2 * 12 * 1000 * 4 + 1001 * 8 * 4
    for bad in ((12, 1000, 50, 12, 5, 5, 200), (12, 1000, 50, 8, 0, 5, 200), (12, 1000, 50, 8, 17, 5, 200), (12, 1000, 0, 8, 5, 5, 200),
                (12, 1000, 50, 8, 5, 0, 200), (12, 1000, 50, 8, 5, 17, 200), (12, 1000, 50, 8, 5, 5, 0), (12, 2 ** 32 // 12 + 1, 50, 8, 5, 5, 200),
                (0, 1000, 50, 8, 5, 5, 200), (12, 0, 50, 8, 5, 5, 200), (12, 4, 50, 8, 5, 5, 200)):
        assert w(*bad) == 0, bad


PTR = 0x10000000      # never dereferenced: a refused call launches nothing
KEYS = (ctypes.c_uint64 * 16)()


@pytest.mark.parametrize('bad', [dict(k=12), dict(V=0), dict(V=65537), dict(V=12 * 36 + 1), dict(n_trials=0), dict(n_trials=17), dict(n_rounds=0),
                                 dict(n_rounds=17), dict(ell=0), dict(ell=65537), dict(cap=0), dict(cap=21846), dict(first=-1), dict(first=12 * 36),
                                 dict(keys=None), dict(u0=2 ** 53), dict(u53=None), dict(u53=PTR + 4), dict(centers=None), dict(centers=PTR + 2),
                                 dict(indices=None), dict(indices=PTR + 4), dict(cand_g=None), dict(cand_g=PTR + 4), dict(weights=None),
                                 dict(weights=PTR + 4), dict(info=None), dict(info=PTR + 4), dict(workspace=None), dict(workspace=PTR + 8),
                                 dict(keep_amax=2), dict(keep_amax=-1), dict(n_seg=2 ** 32 // 12 + 1), dict(x=None), dict(seg_cum=None), dict(pad=2),
                                 dict(R=0), dict(C=0), dict(n_seg=0)],
                         ids=lambda d: ','.join(f'{k}={v}' for k, v in d.items()))
def test_entry_point_refusals(bad):
    a = dict(x=PTR, src_off=PTR, lead_stride=64, raw_len=PTR, seg_cum=PTR, dst_off=PTR, dst_stride=9, R=4, C=12, n_seg=36, k=8, pad=1, V=37, n_trials=5,
             n_rounds=3, ell=74, cap=146, first=0, keys=KEYS, u0=0, u53=PTR, centers=PTR, indices=PTR, cand_g=PTR, weights=PTR, info=PTR, workspace=PTR,
             keep_amax=0, stream=None)
    a.update(bad)
    assert A.lib().ecgvit_tok_scalable_seed(*a.values()) == 1


# ---- the binding ---------------------------------------------------------------------------------------------------
def test_binding_table_is_the_header():
    decls = abi_header.declarations(HEADER)
    assert sorted(decls) == ['ecgvit_tok_scalable_seed', 'ecgvit_tok_scalable_workspace'] == sorted(A.SIGNATURES)
    assert abi_header.mismatches(A.SIGNATURES, decls) == []
    assert len(decls['ecgvit_tok_scalable_seed'][1]) == 29 and decls['ecgvit_tok_scalable_seed'][1][:12] == abi_header.declarations()['ecgvit_tok_seed'][1][:12]
    wrong = dict(A.SIGNATURES, ecgvit_tok_scalable_workspace=(ctypes.c_int64, [hip._I] * 7))       # the comparison sees an int64_t bound as int
    assert len(abi_header.mismatches(wrong, decls)) == 2
    assert not set(A.SIGNATURES) & set(hip.SIGNATURES) and len(hip.SIGNATURES) == 108 and hip.ABI_VERSION == 6
    lib = A.lib()
    assert lib is hip.lib() and lib.ecgvit_abi_version() == 6 and all(hasattr(lib, n) for n in A.SIGNATURES)
    # the one checked-call mechanism, over this table: a status call through `run`, the query through lib()
    assert type(A.run) is type(hip.run) and A.run.ecgvit_tok_scalable_seed.__name__ == 'ecgvit_tok_scalable_seed'
    with pytest.raises(AttributeError):
        A.run.ecgvit_tok_scalable_workspace
    with pytest.raises(AttributeError):
        A.run.ecgvit_tok_seed
    with pytest.raises(AttributeError):
        hip.run.ecgvit_tok_scalable_seed
    a = dict(x=PTR, src_off=PTR, lead_stride=64, raw_len=PTR, seg_cum=PTR, dst_off=PTR, dst_stride=9, R=4, C=12, n_seg=36, k=12)
    with pytest.raises(RuntimeError, match='ecgvit_tok_scalable_seed: ECGVIT_EINVAL'):
        A.run.ecgvit_tok_scalable_seed(*a.values(), 1, 37, 5, 3, 74, 146, 0, KEYS, 0, PTR, PTR, PTR, PTR, PTR, PTR, PTR, 0, None)


def test_limits_are_the_headers_defines():
    text = open(HEADER).read()
    defs = {m.group(1): int(m.group(2)) for m in re.finditer(r'^#define ECGVIT_TOK_SCALABLE_([A-Z0-9_]+)\s+(-?\d+)\b', text, re.M)}
    mirrored = {n: v for n, v in vars(A).items() if n.isupper() and type(v) is int}
    assert defs == mirrored and len(defs) == 4, (defs, mirrored)
    assert tokenizer.MAX_ROUNDS == A.MAX_ROUNDS == 16 and A.info_words(5) == 4 + 15 + 1
    assert not re.search(r'SCALABLE', open(os.path.join(ROOT, 'include', 'ecgvit_hip.h')).read())       # the main header is as it was


# ---- the kernels' budgets --------------------------------------------------------------------------------------------
def test_kernel_register_budgets():
    """the budgets csrc/tok_scalable.hip states: no spill and no scratch anywhere; the fold within 256 VGPRs (two workgroups per CU with four
    segments of 32 samples in registers), the 1024-thread recluster within 128 (four waves per SIMD), the streaming passes within 64"""
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import code_objects
    if not os.path.exists(hip.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    ks = {n: k for n, k in code_objects.kernels(hip.LIB_PATH).items() if 'kmpar_' in n}
    stems = ('kmpar_init_kernel', 'kmpar_fold_kernel', 'kmpar_pot_kernel', 'kmpar_select_count_kernel', 'kmpar_select_scan_kernel',
             'kmpar_select_scatter_kernel', 'kmpar_weights_kernel', 'kmpar_recluster_kernel')
    count = {s: sum(s in n for n in ks) for s in stems}
    assert count == dict(kmpar_init_kernel=3, kmpar_fold_kernel=3, kmpar_pot_kernel=1, kmpar_select_count_kernel=1, kmpar_select_scan_kernel=1,
                         kmpar_select_scatter_kernel=3, kmpar_weights_kernel=1, kmpar_recluster_kernel=3) and len(ks) == 16, count
    for n, k in ks.items():
        assert k['vgpr_spill_count'] == 0 and k['sgpr_spill_count'] == 0 and k['private_segment_fixed_size'] == 0, (n, k)
        limit = 256 if 'kmpar_fold_kernel' in n else 128 if 'kmpar_recluster_kernel' in n else 64
        assert k['vgpr_count'] + k['agpr_count'] <= limit, (n, k)
        assert k['group_segment_fixed_size'] <= (33 * 1024 if 'kmpar_fold_kernel' in n else 8 * 1024), (n, k)
