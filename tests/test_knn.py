"""CPU: the restatement of the device's k-NN search and vote (tests/knn_ref.py) against torch.topk and scikit-learn's brute-force search, and
the host contract of `KnnIndex` / `knn_search` / `knn_merge` / `HipKnnProbe`: every refusal, the exports, the binding table against
include/ecgvit_hip_knn.h, the kernels' register budgets from the code objects.  No GPU is touched."""
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
from ecg_representation_learning_amd import hip, knn, knn_abi as A
import knn_ref as R

HEADER = os.path.join(ROOT, 'include', 'ecgvit_hip_knn.h')


# ---- the restatement against other implementations ------------------------------------------------------------------
@pytest.mark.parametrize('seed', [0, 1, 2])
def test_restatement_is_topk_on_stores_without_ties(seed):
    rng = np.random.default_rng(seed)
    q, b = rng.standard_normal((17, 24)), rng.standard_normal((300, 24))
    s = R.scores64(q, b)
    assert all(len(np.unique(row)) == 300 for row in s)            # no ties: topk's order among equals is not pinned
    for k in (1, 7, 300):
        want = torch.topk(torch.from_numpy(s), k, dim=1)
        got_s, got_i = R.search(q, b, k)
        assert np.array_equal(got_i, want.indices.numpy()) and np.array_equal(got_s, want.values.numpy())
    # leave-one-out drops exactly the own row; index_base shifts what is reported
    got_s, got_i = R.select(R.scores64(b[:17], b), 5, self_base=0, index_base=1000)
    masked = R.scores64(b[:17], b)
    masked[np.arange(17), np.arange(17)] = -np.inf
    want = torch.topk(torch.from_numpy(masked), 5, dim=1)
    assert np.array_equal(got_i, want.indices.numpy() + 1000) and np.array_equal(got_s, want.values.numpy())


def test_restatement_is_sklearns_brute_force_cosine_search():
    neighbors = pytest.importorskip('sklearn.neighbors')
    rng = np.random.default_rng(33)
    b, q = R.integer_store(rng, 200, 33).astype(np.float64), R.integer_store(rng, 16, 33).astype(np.float64)
    unit = lambda x: x / np.sqrt((x * x).sum(axis=1))[:, None]      # noqa: E731  (scikit-learn's own normalisation: a division)
    got_s, got_i = R.search(unit(q), unit(b), 10)
    dist, idx = neighbors.NearestNeighbors(n_neighbors=10, algorithm='brute', metric='cosine').fit(b).kneighbors(q)
    assert np.array_equal(idx, got_i)
    assert np.array_equal(dist, 1.0 - got_s)


def test_restatement_orders_ties_by_index_and_skips_non_finite_scores():
    s = np.array([[1.0, 3.0, 3.0, np.nan, np.inf, -np.inf, 3.0, 2.0]])
    got_s, got_i = R.select(s, 6)
    assert got_i.tolist() == [[1, 2, 6, 7, 0, -1]] and got_s.tolist() == [[3.0, 3.0, 3.0, 2.0, 1.0, -np.inf]]
    got_s, got_i = R.select(s, 2, self_base=1)                    # query 0 is bank row 1
    assert got_i.tolist() == [[2, 6]]
    ms, mi = R.merge([(np.array([[3.0, 1.0]]), np.array([[2, 0]])), (np.array([[3.0, 3.0, -np.inf]]), np.array([[1, 2, -1]]))], 4)
    assert mi.tolist() == [[1, 2, 0, -1]] and ms.tolist() == [[3.0, 3.0, 1.0, -np.inf]]      # the pair that stands twice is taken once


def test_restatement_vote():
    y = np.array([[1, 0], [0, 1], [1, 1]], np.float32)
    s, i = np.array([[0.9, 0.5, 0.1], [0.3, 0.0, 0.0]], np.float32), np.array([[2, 0, 1], [-1, -1, -1]])
    assert R.vote(s, i, y, 'uniform').tolist() == [[np.float32(2 / 3), np.float32(2 / 3)], [0.0, 0.0]]
    w = np.exp((s[0].astype(np.float64) - np.float64(s[0, 0])) / 0.07)
    want = (w[0] * y[2] + w[1] * y[0] + w[2] * y[1]) / w.sum()
    assert np.allclose(R.vote(s, i, y, 'softmax', 0.07)[0], want, rtol=1e-7) and w.max() == 1.0
    assert np.array_equal(R.normalize(np.array([[3.0, 4.0], [0.0, 0.0]])), np.array([[0.6, 0.8], [0.0, 0.0]], np.float32))


# ---- every refusal, met before the device is looked at -----------------------------------------------------------------
def test_refusals_name_their_argument():
    f = torch.zeros(8, 16)
    with pytest.raises(ValueError, match='bank must be a device tensor'):
        E.KnnIndex(f)
    with pytest.raises(ValueError, match='queries must be a device tensor'):
        E.knn_search(f, f, 3)
    with pytest.raises(ValueError, match='metric'):
        E.KnnIndex(f, metric='l2')
    with pytest.raises(ValueError, match='metric'):
        E.knn_search(f, f, 3, metric='euclidean')
    with pytest.raises(ValueError, match='bank must be float32'):
        E.KnnIndex(f.double())
    with pytest.raises(ValueError, match='queries must be float32'):
        E.knn_search(f.half(), f, 3)
    with pytest.raises(ValueError, match='bank must have contiguous rows'):
        E.KnnIndex(torch.zeros(16, 8).t())
    with pytest.raises(ValueError, match='queries must have contiguous rows'):
        E.knn_search(torch.zeros(8, 32)[:, ::2], f, 3)
    with pytest.raises(ValueError, match=r'queries have d = 15, the bank has d = 16'):
        E.knn_search(torch.zeros(8, 15), f, 3)
    with pytest.raises(ValueError, match='bank: d = 2049 exceeds 2048'):
        E.KnnIndex(torch.zeros(2, 2049))
    with pytest.raises(ValueError, match='queries: d = 2049 exceeds 2048'):
        E.knn_search(torch.zeros(2, 2049), torch.zeros(2, 2049)[:, :2048], 1)
    for k in (0, -1, 9, 257, 2.0, True, None):
        with pytest.raises(ValueError, match='k must be an integer'):
            E.knn_search(f, f, k)
    with pytest.raises(ValueError, match=r'k must be an integer in \[1, 7\]'):       # leave-one-out: one row fewer
        E.knn_search(f, f, 8, exclude_self=True)
    with pytest.raises(ValueError, match=r'k must be an integer in \[1, 256\]'):
        E.knn_search(torch.zeros(2, 4), torch.zeros(300, 4), 257)
    with pytest.raises(ValueError, match='self_base'):
        E.knn_search(f, f, 3, exclude_self=True, self_base=-1)
    s, i, y = torch.zeros(4, 3), torch.zeros(4, 3, dtype=torch.int64), torch.zeros(8, 5)
    with pytest.raises(ValueError, match='weights'):
        knn.vote(s, i, y, weights='gaussian')
    for t in (0, 0.0, -0.07, float('inf'), float('nan'), None):
        with pytest.raises(ValueError, match='temperature'):
            knn.vote(s, i, y, temperature=t)
    with pytest.raises(ValueError, match='labels have 8 rows, the bank has 9'):
        knn.vote(s, i, y, n_bank=9)
    with pytest.raises(ValueError, match='indices must be a 2-d torch.int64'):
        knn.vote(s, i.int(), y)
    with pytest.raises(ValueError, match='labels must be a 2-d torch.float32'):
        knn.vote(s, i, y.double())
    with pytest.raises(ValueError, match='scores must be a device tensor'):
        knn.vote(s, i, y)
    with pytest.raises(ValueError, match='parts'):
        E.knn_merge([], 3)
    with pytest.raises(ValueError, match='parts: scores .* must be equal'):
        E.knn_merge([(s, i), (torch.zeros(5, 3), torch.zeros(5, 3, dtype=torch.int64))], 3)
    with pytest.raises(ValueError, match='k must be an integer'):
        E.knn_merge([(s, i)], 0)
    with pytest.raises(ValueError, match='parts: scores must be a device tensor'):
        E.knn_merge([(s, i)], 3)
    for kw in (dict(k=0), dict(k=257), dict(weights='rank'), dict(temperature=0.0), dict(temperature=-1), dict(pool='max'), dict(batch_size=0)):
        with pytest.raises(ValueError, match=next(iter(kw))):
            E.HipKnnProbe(None, **kw)
    p = E.HipKnnProbe(None)
    assert (p.k, p.temperature, p.weights, p.encoder.bsz, p.encoder.pool, p.encoder.norm) == (20, 0.07, 'softmax', 64, 'cls', True)


def test_exports():
    for name in ('HipKnnProbe', 'KnnIndex', 'knn_search', 'knn_merge', 'knn'):
        assert name in E.__all__ and hasattr(E, name), name
    assert E.KnnIndex is knn.KnnIndex and E.HipKnnProbe is E.metrics.HipKnnProbe


# ---- the binding table against the header -----------------------------------------------------------------------------
def test_table_is_the_header_type_by_type():
    decls = abi_header.declarations(HEADER)
    names = ['ecgvit_knn_merge', 'ecgvit_knn_normalize', 'ecgvit_knn_search', 'ecgvit_knn_splits', 'ecgvit_knn_vote', 'ecgvit_knn_workspace']
    assert sorted(decls) == names == sorted(A.SIGNATURES)
    assert abi_header.mismatches(A.SIGNATURES, decls) == []
    assert len(decls['ecgvit_knn_search'][1]) == 15 and decls['ecgvit_knn_vote'][1][9] == 'double'
    wrong = dict(A.SIGNATURES, ecgvit_knn_workspace=(ctypes.c_int64, [hip._I] * 5))              # the comparison sees an int64_t bound as int
    assert len(abi_header.mismatches(wrong, decls)) == 2
    assert not set(A.SIGNATURES) & set(hip.SIGNATURES) and len(hip.SIGNATURES) == 108 and hip.ABI_VERSION == 6
    lib = A.lib()
    assert lib is hip.lib() and lib.ecgvit_abi_version() == 6 and all(hasattr(lib, n) for n in A.SIGNATURES)
    assert type(A.run) is type(hip.run) and A.run.ecgvit_knn_search.__name__ == 'ecgvit_knn_search'
    for query in ('ecgvit_knn_workspace', 'ecgvit_knn_splits'):                                  # queries go through lib()
        with pytest.raises(AttributeError):
            getattr(A.run, query)


def test_limits_are_the_headers_defines():
    text = open(HEADER).read()
    defs = {m.group(1): int(m.group(2)) for m in re.finditer(r'^#define ECGVIT_KNN_([A-Z0-9_]+)\s+(-?\d+)\b', text, re.M)}
    mirrored = {n: v for n, v in vars(A).items() if n.isupper() and type(v) is int}
    assert defs == mirrored and len(defs) == 9, (defs, mirrored)
    assert A.MAX_K == 256 and hip.ROW_MAX_D == 2048
    assert not re.search(r'KNN', open(os.path.join(ROOT, 'include', 'ecgvit_hip.h')).read())     # the main header is as it was
    assert not any('KNN' in n or 'knn' in n for n in vars(hip))                                  # and so is hip.py


def test_host_side_of_the_entry_points_refuses_before_launching():
    """every entry point returns ECGVIT_EINVAL on bad arguments; with null pointers nothing could have been launched"""
    lib = A.lib()
    assert lib.ecgvit_knn_splits(1, 1, 0) == 1 and lib.ecgvit_knn_splits(2200, 17400, 0) == 28 and lib.ecgvit_knn_splits(4096, 800000, 0) == 16
    assert lib.ecgvit_knn_splits(21837, 21837, 0) == 2 and lib.ecgvit_knn_splits(10 ** 6, 10 ** 6, 0) == 1              # never more than 512 workgroups in a round
    assert lib.ecgvit_knn_splits(100, 1000, 7) == 7 and lib.ecgvit_knn_splits(100, 1000, 100) == 8       # capped by the bank's tiles
    assert lib.ecgvit_knn_splits(0, 5, 0) == 0 and lib.ecgvit_knn_splits(5, 0, 0) == 0 and lib.ecgvit_knn_splits(5, 5, 1025) == 0
    assert lib.ecgvit_knn_workspace(10, 1000, 768, 20, 2) == 10 * 2 * 20 * 12
    assert lib.ecgvit_knn_workspace(3, 1000, 768, 1, 1) == 16 + 24                               # the scores rounded up to 16 bytes
    for bad in ((10, 1000, 0, 20, 0), (10, 1000, 2049, 20, 0), (10, 1000, 8, 0, 0), (10, 1000, 8, 257, 0), (10, 1000, 8, 20, -1)):
        assert lib.ecgvit_knn_workspace(*bad) == 0, bad
    p = 4096                                                        # never dereferenced: every call below is refused on its numbers
    ok = dict(ldq=8, ldb=8, Q=4, N=10, d=8, k=3, self_base=-1, index_base=0, splits=0)
    def search(**kw):
        a = dict(ok, **kw)
        return lib.ecgvit_knn_search(p, a['ldq'], p, a['ldb'], a['Q'], a['N'], a['d'], a['k'], a['self_base'], a['index_base'], a['splits'], p, p, p, None)
    for kw in (dict(Q=0), dict(N=0), dict(d=0), dict(d=2049, ldq=4096, ldb=4096), dict(k=0), dict(k=11), dict(k=257, N=1000), dict(k=10, self_base=0),
               dict(self_base=-2), dict(N=2 ** 31), dict(ldq=7), dict(ldb=7), dict(ldb=A.MAX_PITCH + 1), dict(splits=-1), dict(splits=1025)):
        assert search(**kw) == 1, kw
    assert lib.ecgvit_knn_search(None, 8, p, 8, 4, 10, 8, 3, -1, 0, 0, p, p, p, None) == 1
    assert lib.ecgvit_knn_search(p, 8, p, 8, 4, 10, 8, 3, -1, 0, 0, p, p, None, None) == 1
    for args in ((0, 0, 3, 4, 3, 3), (1, 0, 3, 0, 3, 3), (1, 0, 3, 4, 0, 3), (1, 0, 3, 4, 3, 0), (1, 0, 3, 4, 3, 257), (1, 0, 2, 4, 3, 3), (2048, 0, 600, 4, 600, 3)):
        P, stride, ld, Q, kp, k = args
        assert lib.ecgvit_knn_merge(p, p, P, stride, ld, Q, kp, k, 0, p, p, None) == 1, args
    for args in ((8, 8, 0, 8), (8, 8, 4, 0), (8, 8, 4, 2049), (7, 8, 4, 8), (8, 7, 4, 8)):
        ldx, ldo, rows, d = args
        assert lib.ecgvit_knn_normalize(p, ldx, p, ldo, rows, d, None) == 1, args
    for args in ((0, 3, 5, 8, 5, 1, 0.07), (4, 0, 5, 8, 5, 1, 0.07), (4, 257, 5, 8, 5, 1, 0.07), (4, 3, 4, 8, 5, 1, 0.07), (4, 3, 5, 0, 5, 1, 0.07),
                 (4, 3, 5, 8, 0, 1, 0.07), (4, 3, 5, 8, 5, 2, 0.07), (4, 3, 5, 8, 5, 1, 0.0), (4, 3, 5, 8, 5, 1, -1.0), (4, 3, 5, 8, 5, 1, float('nan'))):
        Q, k, ldy, N, K, mode, T = args
        assert lib.ecgvit_knn_vote(p, p, Q, k, p, ldy, N, K, mode, T, p, None) == 1, args


# ---- the kernels' budgets, from the built library ----------------------------------------------------------------------
def test_kernels_do_not_spill():
    """what csrc/knn.hip states: no spill and no scratch in any knn_ kernel; the search (its two forms: lists in LDS for k <= 32, in the
    workspace above) within 256 registers and 65 KiB of LDS (operand tiles 33 KiB, lists 32 KiB): two workgroups per CU; the merge (its two
    forms: up to 2 048 entries per query in registers, or streamed) within 128"""
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import code_objects
    if not os.path.exists(hip.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    ks = {n: k for n, k in code_objects.kernels(hip.LIB_PATH).items() if 'knn_' in n}
    stems = ('knn_search_kernel', 'knn_merge_kernel', 'knn_normalize_kernel', 'knn_vote_kernel')
    assert {s: sum(s in n for n in ks) for s in stems} == dict(dict.fromkeys(stems, 1), knn_search_kernel=2, knn_merge_kernel=2) and len(ks) == 6, sorted(ks)
    for n, k in ks.items():
        assert 'kernel_4w' not in n and 'gemm_nt_kernel' not in n
        assert k['vgpr_spill_count'] == 0 and k['sgpr_spill_count'] == 0 and k['private_segment_fixed_size'] == 0, (n, k)
        assert k['vgpr_count'] + k['agpr_count'] <= (256 if 'knn_search_kernel' in n else 128 if 'knn_merge_kernel' in n else 64), (n, k)
        assert k['group_segment_fixed_size'] <= (65 * 1024 if 'knn_search_kernel' in n else 8 * 1024), (n, k)
