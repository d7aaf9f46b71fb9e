"""CPU: the restatement of the rank route to AUROC (tests/rank_ref.py) against the oracle's all-pairs counts, `get_accuracy_np` and scikit-learn's
`roc_auc_score`; the counter-based generator; and the host contract of `rank_scores` / `auroc_counts` / `bootstrap_auc`: every refusal, the
exports, the binding table against include/ecgvit_hip_rank.h, the kernels' register budgets from the code objects.  No GPU is touched."""
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
from ecg_representation_learning_amd import hip, rank_abi as A, rank_metrics as RM
from oracle.metrics_oracle import eval_counts_np, get_accuracy_np
import rank_ref as R

HEADER = os.path.join(ROOT, 'include', 'ecgvit_hip_rank.h')


def grid_store(seed, n=300, K=5):
    rng = np.random.default_rng(seed)
    s = (rng.integers(0, 17, (n, K)) / 16).astype(np.float32)
    y = (rng.random((n, K)) < np.array([0.5, 0.2, 0.05, 0.01, 0.0])[:K]).astype(np.float32)
    y[:3, 3] = 1
    return s, y


# ---- the restatement against other implementations ------------------------------------------------------------------
@pytest.mark.parametrize('kind', R.KINDS)
def test_unit_weights_give_the_all_pairs_integers(kind):
    rng = np.random.default_rng(R.KINDS.index(kind))
    s, y = R.store(kind, rng, 257, 4), R.labels_for(rng, 257, 4)
    y[:, 2], y[:, 3] = 0, 1                                         # a class without a positive, one without a negative
    with np.errstate(invalid='ignore'):
        want = eval_counts_np(s, y)
    got = R.triples(s, y)[0]
    assert np.array_equal(got[:, 0], want[4 + 4:]) and np.array_equal(got[:, 1], want[4:8]) and np.array_equal(got[:, 1] + got[:, 2], [257] * 4)


def test_keys_order_as_floats_do():
    v = np.array([-np.inf, -1.0, -1e-45, -0.0, 0.0, 1e-45, 1.17549435e-38, 0.5, np.inf, np.nan], np.float32)
    k = R.keys(v)
    assert k[3] == k[4] and k[9] == 0xFFFFFFFF and (np.diff(k[[0, 1, 2, 3, 5, 6, 7, 8, 9]].astype(np.int64)) > 0).all()
    assert R.keys(np.array([-np.nan], np.float32))[0] == 0xFFFFFFFF
    word, nan0 = R.packed(R.keys(np.array([0.5, np.nan, 0.5, 0.25], np.float32)), np.array([1, 0, 0, 1]))
    assert word.tolist() == [3 | 1 << 30 | 1 << 31, 0 | 1 << 30, 2 | 1 << 31, 1 | 1 << 31] and nan0 == 3


@pytest.mark.parametrize('seed', [0, 1])
def test_weighted_rank_sum_is_the_reference_on_the_resample(seed):
    s, y = grid_store(seed)
    rng = np.random.default_rng(seed + 10)
    idx = rng.integers(0, 300, (24, 300))
    t = R.triples(s, y, R.from_indices(idx, 300))
    for b, row in enumerate(idx):
        want = get_accuracy_np(s[row], y[row])
        for c in range(5):
            num2, wp, wn = (int(v) for v in t[b, c])
            if wp == 0 or wn == 0:
                assert c not in want['per_class_auc']
            else:
                assert abs(num2 / (2 * wp * wn) - want['per_class_auc'][c]) <= 1e-12
        res = RM.BootstrapResult(None, t)
        assert abs(res.macro_auc[b] - want['macro_auc']) <= 1e-12


def test_weighted_rank_sum_is_sklearns_roc_auc_score():
    metrics = pytest.importorskip('sklearn.metrics')
    s, y = grid_store(3)
    rng = np.random.default_rng(5)
    idx = rng.integers(0, 300, (16, 300))
    mult = R.from_indices(idx, 300)
    t = R.triples(s, y, mult)
    seen = 0
    for b in range(16):
        for c in range(4):
            num2, wp, wn = (int(v) for v in t[b, c])
            if wp == 0 or wn == 0:
                continue
            got = num2 / (2 * wp * wn)
            assert abs(got - metrics.roc_auc_score(y[idx[b], c], s[idx[b], c])) <= 1e-12
            assert abs(got - metrics.roc_auc_score(y[:, c], s[:, c], sample_weight=mult[b])) <= 1e-12
            seen += 1
    assert seen >= 40


def test_bootstrap_result_rules():
    t = np.array([[[6, 2, 3], [0, 0, 5], [4, 1, 2]], [[0, 5, 0], [0, 0, 5], [0, 0, 3]]], np.int64)
    res = RM.BootstrapResult(dict(per_class_auc={0: 0.5, 2: 1.0}), t)
    assert np.array_equal(res.per_class_auc, [[0.5, np.nan, 1.0], [np.nan] * 3], equal_nan=True)
    assert res.macro_auc[0] == 0.75 and np.isnan(res.macro_auc[1]) and res.n_valid.tolist() == [1, 0, 1]
    assert res.ci() == (0.75, 0.75) and res.ci(0.5) == (0.75, 0.75)
    cc = res.class_ci()
    assert cc.shape == (3, 2) and cc[0].tolist() == [0.5, 0.5] and np.isnan(cc[1]).all()
    assert RM.intervals(res) == ((0.75, 0.75), {0: (0.5, 0.5), 2: (1.0, 1.0)})
    for alpha in (0, 1, -0.1, True, None):
        with pytest.raises(ValueError, match='alpha'):
            res.ci(alpha)


# ---- the generator ----------------------------------------------------------------------------------------------------------
def test_generator_is_its_integer_form_and_sums_to_n():
    for seed, r, n in ((0, 0, 1), (0, 0, 7), (2 ** 64 - 1, 999, 1000), (12345, 3, 2 ** 30)):
        d = R.draws(seed, r, min(n, 512)) if n <= 512 else None
        js = range(min(n, 64))
        if d is not None:
            assert all(R.draw_int(seed, r, j, n) == d[j] for j in js)
        else:                                                        # the first draws of a long replicate: the map's split product at n near 2^30
            with np.errstate(over='ignore'):
                u = R.mix(R.mix(np.uint64((seed + R.GAMMA * (r + 1)) & R.M64)) + np.uint64(R.GAMMA) * np.arange(1, 65, dtype=np.uint64))
            assert [int(v) * n >> 64 for v in u] == [R.draw_int(seed, r, j, n) for j in js]
    assert np.array_equal(RM.draws(9, 4, 1000), R.draws(9, 4, 1000)) and np.array_equal(RM.multiplicities(9, 4, 1000), R.multiplicities(9, 4, 1000))
    m = R.multiplicities(5, 2, 1000)
    assert m.sum() == 1000 and m.shape == (1000,)


def test_generator_statistics():
    """(1 - 1/n)^n = 0.36788 of the records are left out of a replicate: within 0.01 in each of 64 replicates at n = 100 000 (the binomial
    deviation is 0.0015; numpy's own generator spans 0.3656 .. 0.3715 there)"""
    n = 100000
    zero = []
    for r in range(64):
        m = R.multiplicities(77, r, n)
        assert m.sum() == n
        zero.append(float((m == 0).mean()))
    assert max(abs(z - (1 - 1 / n) ** n) for z in zero) < 0.01, (min(zero), max(zero))
    a, b, c = R.draws(77, 0, 4096), R.draws(77, 1, 4096), R.draws(78, 0, 4096)
    assert (a != b).mean() > 0.99 and (a != c).mean() > 0.99                       # replicates and seeds differ
    # the draws are a function of (seed, replicate, draw): a chunk that starts at replicate 5 makes replicate 5's draws
    assert np.array_equal(np.stack([R.draws(77, r, 333) for r in range(8)])[5:], np.stack([R.draws(77, 5 + r, 333) for r in range(3)]))


# ---- every refusal, met before the device is looked at -----------------------------------------------------------------
def test_refusals_name_their_argument():
    s, y = torch.zeros(8, 3), torch.zeros(8, 3)
    for fn in (E.rank_scores, E.auroc_counts, E.bootstrap_auc):
        with pytest.raises(ValueError, match='scores must be a device tensor'):
            fn(s, y)
        with pytest.raises(ValueError, match='scores must be float32'):
            fn(s.double(), y)
        with pytest.raises(ValueError, match='labels must be float32'):
            fn(s, y.int())
        with pytest.raises(ValueError, match='scores must be a torch tensor'):
            fn(s.numpy(), y)
        with pytest.raises(ValueError, match=r'scores must be \(n, K\)'):
            fn(torch.zeros(8), y)
        with pytest.raises(ValueError, match=r'labels must be \(8, 3\) as scores'):
            fn(s, torch.zeros(8, 4))
        with pytest.raises(ValueError, match='scores must have contiguous rows'):
            fn(torch.zeros(3, 8).t(), y)
        with pytest.raises(ValueError, match='labels must have contiguous rows'):
            fn(s, torch.zeros(8, 6)[:, ::2])
        with pytest.raises(ValueError, match='at least one record'):
            fn(torch.zeros(0, 3), torch.zeros(0, 3))
        big = torch.empty(A.MAX_ROWS + 1, 1, device='meta')
        with pytest.raises(ValueError, match=f'n = {A.MAX_ROWS + 1} exceeds {A.MAX_ROWS}'):
            fn(big, big)
        wide = torch.empty(2, A.MAX_CLASSES + 1, device='meta')
        with pytest.raises(ValueError, match=f'K = {A.MAX_CLASSES + 1} exceeds {A.MAX_CLASSES}'):
            fn(wide, wide)
    for n_boot in (0, -1, 2.0, True, None):
        with pytest.raises(ValueError, match='n_boot'):
            E.bootstrap_auc(s, y, n_boot=n_boot)
    with pytest.raises(ValueError, match=f'n_boot = {A.MAX_REPLICATES + 1} exceeds'):
        E.bootstrap_auc(s, y, n_boot=A.MAX_REPLICATES + 1)
    for seed in (-1, 2 ** 64, 1.5, True, None):
        with pytest.raises(ValueError, match='seed'):
            E.bootstrap_auc(s, y, seed=seed)
    idx = np.zeros((2, 8), np.int64)
    with pytest.raises(ValueError, match='seed and indices are both given'):
        E.bootstrap_auc(s, y, seed=3, indices=idx)
    for bad in (np.full((2, 8), 8), np.full((2, 8), -1), torch.full((1, 8), 9)):
        with pytest.raises(ValueError, match=r'indices must lie in \[0, 8\)'):
            E.bootstrap_auc(s, y, indices=bad)
    with pytest.raises(ValueError, match=r'indices must be \(R, 8\)'):
        E.bootstrap_auc(s, y, indices=np.zeros((2, 7), np.int64))
    with pytest.raises(ValueError, match='indices must be an'):
        E.bootstrap_auc(s, y, indices=np.zeros((2, 8)))
    for ws in (0, -5, 1.5, True):
        with pytest.raises(ValueError, match='workspace_bytes'):
            E.bootstrap_auc(s, y, workspace_bytes=ws)
    with pytest.raises(ValueError, match='scores must be a device tensor'):             # in-range host indices pass; the device is asked for last
        E.bootstrap_auc(s, y, indices=idx)
    from ecg_representation_learning_amd.metrics import _add_bootstrap
    for bootstrap in (True, 1.5, 'yes'):
        with pytest.raises(ValueError, match='bootstrap must be'):
            _add_bootstrap({}, {}, 'eval', bootstrap, s, y, False, None)
    with pytest.raises(ValueError, match='unknown keywords'):
        _add_bootstrap({}, {}, 'eval', dict(n_boot=3, from_logits=True), s, y, False, None)
    with pytest.raises(ValueError, match='n_boot'):
        _add_bootstrap({}, {}, 'eval', 0, s, y, False, None)


def test_exports_and_signatures():
    import inspect
    for name in ('rank_scores', 'auroc_counts', 'bootstrap_auc', 'RankedScores', 'BootstrapResult', 'rank_metrics'):
        assert name in E.__all__ and hasattr(E, name), name
    assert E.bootstrap_auc is RM.bootstrap_auc and set(RM.__all__) <= set(vars(RM))
    assert list(inspect.signature(E.bootstrap_auc).parameters) == ['scores', 'labels', 'n_boot', 'seed', 'indices', 'from_logits', 'id2code', 'workspace_bytes']
    assert inspect.signature(E.bootstrap_auc).parameters['n_boot'].default == 1000
    for fn in (E.HipEvaluator.evaluate, E.HipKnnProbe.evaluate, E.HipKnnProbe.leave_one_out):
        assert inspect.signature(fn).parameters['bootstrap'].default is None


# ---- the binding table against the header -----------------------------------------------------------------------------
def test_table_is_the_header_type_by_type():
    decls = abi_header.declarations(HEADER)
    names = ['ecgvit_rank_multiplicities', 'ecgvit_rank_multiplicities_seeded', 'ecgvit_rank_sort', 'ecgvit_rank_walk', 'ecgvit_rank_workspace']
    assert sorted(decls) == names == sorted(A.SIGNATURES)
    assert abi_header.mismatches(A.SIGNATURES, decls) == []
    assert len(decls['ecgvit_rank_sort'][1]) == 11 and decls['ecgvit_rank_multiplicities_seeded'][1][0] == 'uint64_t'
    wrong = dict(A.SIGNATURES, ecgvit_rank_workspace=(ctypes.c_int64, [hip._I] * 3))              # the comparison sees an int64_t bound as int
    assert len(abi_header.mismatches(wrong, decls)) == 2
    assert not set(A.SIGNATURES) & set(hip.SIGNATURES) and len(hip.SIGNATURES) == 108 and hip.ABI_VERSION == 6
    assert len(abi_header.declarations()) == 108
    lib = A.lib()
    assert lib is hip.lib() and lib.ecgvit_abi_version() == 6 and all(hasattr(lib, n) for n in A.SIGNATURES)
    assert type(A.run) is type(hip.run) and A.run.ecgvit_rank_walk.__name__ == 'ecgvit_rank_walk'
    with pytest.raises(AttributeError):                                                           # the query goes through lib()
        getattr(A.run, 'ecgvit_rank_workspace')


def test_limits_are_the_headers_defines():
    text = open(HEADER).read()
    defs = {m.group(1): int(m.group(2)) for m in re.finditer(r'^#define ECGVIT_RANK_([A-Z0-9_]+)\s+(-?\d+)\b', text, re.M)}
    mirrored = {n: v for n, v in vars(A).items() if n.isupper() and type(v) is int}
    assert defs == mirrored and len(defs) == 7, (defs, mirrored)
    assert A.MAX_ROWS == 1 << 30 and A.TILE % 256 == 0 and A.WALK_ROWS % 64 == 0
    assert not re.search(r'RANK', open(os.path.join(ROOT, 'include', 'ecgvit_hip.h')).read())    # the main header is as it was
    assert not any('RANK' in n for n in vars(hip))                                               # and so is hip.py


def test_host_side_of_the_entry_points_refuses_before_launching():
    """every entry point returns ECGVIT_EINVAL on bad arguments; with null or never-dereferenced pointers nothing could have been launched"""
    lib = A.lib()
    plane = lambda b: (b + 255) // 256 * 256                       # noqa: E731
    assert lib.ecgvit_rank_workspace(2200, 71, 0) == 4 * plane(71 * 2200 * 4) + plane(71 * 2 * 1024) + plane(71 * 1024)
    assert lib.ecgvit_rank_workspace(2200, 71, 1) == plane(4 * 8800) == lib.ecgvit_rank_workspace(2200, 71, 4)          # four replicates wide
    assert lib.ecgvit_rank_workspace(2200, 71, 1000) == plane(8800000) and lib.ecgvit_rank_workspace(2200, 71, 5) == plane(8 * 8800)
    for bad in ((0, 5, 0), (A.MAX_ROWS + 1, 5, 0), (10, 0, 0), (10, A.MAX_CLASSES + 1, 0), (10, 5, -1), (10, 5, A.MAX_REPLICATES + 1)):
        assert lib.ecgvit_rank_workspace(*bad) == 0, bad
    p = 4096                                                        # never dereferenced: every call below is refused on its numbers
    ok = dict(ld=5, ldl=5, n=10, K=5)

    def sort(ws=p, **kw):
        a = dict(ok, **kw)
        return lib.ecgvit_rank_sort(p, a['ld'], p, a['ldl'], a['n'], a['K'], 0, p, p, ws, None)
    for kw in (dict(n=0), dict(n=A.MAX_ROWS + 1), dict(K=0), dict(K=A.MAX_CLASSES + 1, ld=10 ** 6, ldl=10 ** 6), dict(ld=4), dict(ldl=4), dict(ws=None),
               dict(ws=4096 + 64)):
        assert sort(**kw) == 1, kw
    assert lib.ecgvit_rank_sort(None, 5, p, 5, 10, 5, 0, p, p, p, None) == 1
    for args in ((p, 9, 2, 10, p), (None, 10, 2, 10, p), (p, 10, 0, 10, p), (p, 10, 2, 0, p), (p, 10, 2, 10, None), (p, 10, A.MAX_REPLICATES + 1, 10, p)):
        assert lib.ecgvit_rank_multiplicities(*args, None) == 1, args
    for args in ((0, -1, 2, 10, p), (0, 0, 0, 10, p), (0, 0, 2, 0, p), (0, 0, 2, A.MAX_ROWS + 1, p), (0, 0, 2, 10, None), (0, 0, 2, 10, p + 4)):
        assert lib.ecgvit_rank_multiplicities_seeded(*args, None) == 1, args
    for args in ((None, p, 10, 5, p, 2, p, None), (p, None, 10, 5, p, 2, p, None), (p, p, 0, 5, p, 2, p, None), (p, p, 10, 0, p, 2, p, None),
                 (p, p, 10, 5, p, 0, p, None), (p, p, 10, 5, p, 2, None, None), (p, p, 10, 5, p, 2, p, p), (p, p, 10, 5, p, A.MAX_REPLICATES + 1, p, None), (p, p, 10, 5, p + 8, 2, p, None)):
        assert lib.ecgvit_rank_walk(*args, None) == 1, args


# ---- the kernels' budgets, from the built library ----------------------------------------------------------------------
def test_kernels_do_not_spill():
    """what csrc/rank_metrics.hip states: seven kernels, no spill and no scratch in any; the walk (four replicates' state per lane) within 128
    registers, everything else within 64; LDS: the key transpose 16.25 KiB, the scatter's four wave histograms 4 KiB"""
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import code_objects
    if not os.path.exists(hip.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    ks = {n: k for n, k in code_objects.kernels(hip.LIB_PATH).items() if 'rank_' in n}
    stems = ('rank_keys_kernel', 'rank_hist_kernel', 'rank_scan_kernel', 'rank_scatter_kernel', 'rank_pack_kernel', 'rank_multiplicity_kernel', 'rank_walk_kernel')
    assert {s: sum(s in n for n in ks) for s in stems} == dict.fromkeys(stems, 1) and len(ks) == 7, sorted(ks)
    for n, k in ks.items():
        assert k['vgpr_spill_count'] == 0 and k['sgpr_spill_count'] == 0 and k['private_segment_fixed_size'] == 0, (n, k)
        assert k['vgpr_count'] + k['agpr_count'] <= (128 if 'rank_walk_kernel' in n else 64), (n, k)
        assert k['group_segment_fixed_size'] <= (17 * 1024 if 'rank_keys_kernel' in n else 4 * 1024), (n, k)
