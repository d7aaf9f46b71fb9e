"""CPU: the restatement of average precision and class-wise F-max (tests/pr_ref.py) against scikit-learn's `average_precision_score` and
`precision_recall_curve`; the host contract of `pr_walk` / `pr_counts` / `bootstrap_pr` / `paired_diff_ci`: every refusal, the exports, the binding
table against include/ecgvit_hip_pr.h, the entry point's own refusals, the kernel's register budget from the code object.  No GPU is touched."""
import inspect
import itertools
import os
import re
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT
import abi_header
import ecg_representation_learning_amd as E
from ecg_representation_learning_amd import hip, pr_abi as A, pr_metrics as PM, rank_abi, rank_metrics as RM
import pr_ref as P
import rank_ref as R

HEADER = os.path.join(ROOT, 'include', 'ecgvit_hip_pr.h')
AP_TOL = 2.0 ** -32 + 1e-12          # the truncation bound of the header plus scikit-learn's own f64 rounding
F_TOL = 1e-12


def sklearn_values(y, s, w=None):
    """(AP, F-max, the highest threshold that attains it) from scikit-learn; F ties are exact rationals, so 1e-12 tells them from near misses"""
    metrics = pytest.importorskip('sklearn.metrics')
    ap = metrics.average_precision_score(y, s, sample_weight=w)
    p, r, t = metrics.precision_recall_curve(y, s, sample_weight=w)
    with np.errstate(divide='ignore', invalid='ignore'):
        f = np.where(p + r > 0, 2 * p * r / (p + r), 0.0)[:-1]
    return ap, f.max(), float(t[np.flatnonzero(f >= f.max() - 1e-12)[-1]])


def held(s, y, w=None, resample=None):
    v = P.six(R.keys(s), y, w)
    assert v[1] > 0 and v[2] > 0, 'a test case must define the value'
    ap, f, thr = P.values(v, s)
    refs = [sklearn_values(y, s, w)] + ([sklearn_values(y[resample], s[resample])] if resample is not None else [])
    for ap2, f2, thr2 in refs:
        assert abs(ap - ap2) <= AP_TOL and ap <= ap2 + 1e-12, (ap, ap2)
        assert abs(f - f2) <= F_TOL, (f, f2)
        assert thr == thr2, (thr, thr2)
    return v


# ---- the restatement against scikit-learn ---------------------------------------------------------------------------------------------------
def test_every_tie_pattern_of_four_records():
    """all 75 weak orderings of four scores, under all 14 labellings that hold both values"""
    seen = 0
    for sc in itertools.product(range(4), repeat=4):
        if set(sc) != set(range(max(sc) + 1)):
            continue
        s = np.array(sc, np.float32) / 4
        for lab in range(1, 15):
            held(s, np.array([(lab >> i) & 1 for i in range(4)], np.float32))
        seen += 1
    assert seen == 75


@pytest.mark.parametrize('kind', ['grid', 'gauss'])
def test_weights_and_resamples(kind):
    """sample_weight = the multiplicities of a resample, and the resampled arrays themselves: one value"""
    rng = np.random.default_rng(['grid', 'gauss'].index(kind))
    seen = 0
    for trial in range(40):
        n = int(rng.integers(2, 301))
        s = (rng.integers(0, 9, n) / 8).astype(np.float32) if kind == 'grid' else rng.standard_normal(n).astype(np.float32)
        y = (rng.random(n) < rng.choice([0.5, 0.2, 0.05])).astype(np.float32)
        idx = rng.integers(0, n, n)
        w = np.bincount(idx, minlength=n)
        if w[y != 0].sum() and w[y == 0].sum():
            held(s, y, w, idx)
            seen += 1
        if 0 < y.sum() < n:
            held(s, y)
    assert seen >= 25


def test_hand_cases():
    s, y = np.array([0.9, 0.8, 0.8, 0.1], np.float32), np.array([1, 0, 1, 0], np.float32)
    # groups from the top: {0.9: +}, {0.8: + -}, {0.1: -}: AP = 1/2 * 1 + 1/2 * 2/3; F: 2/3, 4/5, 2/3 -> the group of 0.8, ascending position 1
    assert P.six(R.keys(s), y) == [(1 << 32) + (1 * 2 * (1 << 32)) // 3, 2, 2, 2, 1, 1]
    # NaN: counted in wp, never predicted; all positives NaN: (0, 0, -1)
    s2 = np.array([np.nan, 0.8, 0.5, 0.1], np.float32)
    assert P.six(R.keys(s2), y) == [(1 << 32) // 2, 2, 2, 1, 1, 1]
    assert P.six(R.keys(np.array([np.nan, 0.8, np.nan, 0.1], np.float32)), y) == [0, 2, 2, 0, 0, -1]
    assert P.six(R.keys(s), np.zeros(4)) == [0, 0, 4, 0, 0, -1]
    # an F tie between two thresholds goes to the higher one: wp = 2, F(1, 0) = 2 / 3 = 4 / 6 = F(2, 2)
    s3, y3 = np.array([4, 3, 2, 1], np.float32), np.array([1, 0, 0, 1], np.float32)
    assert P.six(R.keys(s3), y3)[3:] == [1, 0, 3] and P.six(R.keys(s3), 1 - y3)[3:] == [2, 1, 1]
    # weights beyond 2^26: a term past 2^53, where an f64 quotient is wrong
    w = np.array([1 << 26] * 4 + [(1 << 26) - 1] * 4, np.int64)
    s4, y4 = np.array([1, 1, 1, 1, 0, 0, 0, 0], np.float32), np.array([1, 1, 1, 0, 1, 0, 1, 0], np.float32)
    tp, fp = 3 << 26, 1 << 26
    assert tp * tp > 1 << 53 and P.six(R.keys(s4), y4, w)[0] == tp * tp * (1 << 32) // (tp + fp) + (int(w[4:].sum()) // 2) * (tp + int(w[4]) * 2) * (1 << 32) // int(w.sum())


def test_result_classes_and_paired_differences():
    six = np.array([[[3 << 31, 2, 3, 2, 1, 4], [0, 0, 5, 0, 0, -1]], [[1 << 32, 1, 1, 1, 0, 1], [0, 5, 0, 0, 0, -1]]], np.int64)
    res = PM.PrBootstrapResult(dict(per_class_ap={0: 0.75}, per_class_fmax={0: 0.8}), six)
    assert np.array_equal(res.per_class_ap, [[0.75, np.nan], [1.0, np.nan]], equal_nan=True)
    assert np.array_equal(res.per_class_fmax, [[0.8, np.nan], [1.0, np.nan]], equal_nan=True)
    assert res.macro_ap.tolist() == [0.75, 1.0] and res.macro_fmax.tolist() == [0.8, 1.0] and res.n_valid.tolist() == [2, 0]
    assert res.ci('ap', 0.5) == (0.8125, 0.9375) and res.class_ci('fmax').shape == (2, 2) and np.isnan(res.class_ci('ap')[1]).all()
    assert RM.intervals(res, 'ap', 0.5) == ((0.8125, 0.9375), {0: (0.8125, 0.9375)})
    with pytest.raises(ValueError, match='metric must be one of'):
        res.ci('auc')
    with pytest.raises(ValueError, match='alpha'):
        res.ci('ap', 1.5)
    other = PM.PrBootstrapResult(None, six[::-1].copy())
    with pytest.raises(ValueError, match='a carries no record of its draws'):
        E.paired_diff_ci(res, other, 'ap')
    for r in (res, other):
        r.n, r.n_boot, r.seed, r.source = 5, 2, 7, RM.draw_source(7, None)
    assert E.paired_diff_ci(res, other, 'ap', 0.5) == (-0.125, 0.125) and E.paired_diff_ci(res, res, 'fmax') == (0.0, 0.0)
    other.source = RM.draw_source(8, None)
    with pytest.raises(ValueError, match='b was not resampled as a: source'):
        E.paired_diff_ci(res, other, 'ap')
    other.source, other.n = res.source, 6
    with pytest.raises(ValueError, match='b was not resampled as a: n is 6 against 5'):
        E.paired_diff_ci(res, other, 'ap')
    with pytest.raises(ValueError, match="metric must be 'auc', 'ap' or 'fmax'"):
        E.paired_diff_ci(res, res, 'f1')
    with pytest.raises(ValueError, match='a must be a BootstrapResult'):
        E.paired_diff_ci(res, res, 'auc')
    auc = RM.BootstrapResult(None, np.array([[[6, 2, 3]], [[4, 1, 2]]], np.int64))
    assert auc.source is None and auc.seed is None
    with pytest.raises(ValueError, match='b must be a PrBootstrapResult'):
        E.paired_diff_ci(res, auc, 'ap')
    auc.n, auc.n_boot, auc.source = 5, 2, RM.draw_source(0, torch.tensor([[0, 1], [1, 1]]))
    assert auc.source[:2] == ('indices', 2) and auc.source == RM.draw_source(0, torch.tensor([[0, 1], [1, 1]], dtype=torch.int32))
    assert auc.source != RM.draw_source(0, torch.tensor([[1, 0], [1, 1]])) and E.paired_diff_ci(auc, auc, 'auc') == (0.0, 0.0)


# ---- every refusal, met before the device is looked at ---------------------------------------------------------------------------------------
def test_refusals_name_their_argument():
    s, y = torch.zeros(8, 3), torch.zeros(8, 3)
    for fn in (E.pr_counts, E.bootstrap_pr):
        with pytest.raises(ValueError, match='scores must be a device tensor'):
            fn(s, y)
        with pytest.raises(ValueError, match='scores must be float32'):
            fn(s.double(), y)
        with pytest.raises(ValueError, match='labels must be float32'):
            fn(s, y.int())
        with pytest.raises(ValueError, match=r'labels must be \(8, 3\) as scores'):
            fn(s, torch.zeros(8, 4))
        with pytest.raises(ValueError, match='scores must have contiguous rows'):
            fn(torch.zeros(3, 8).t(), y)
        big = torch.empty(rank_abi.MAX_ROWS + 1, 1, device='meta')
        with pytest.raises(ValueError, match=f'n = {rank_abi.MAX_ROWS + 1} exceeds'):
            fn(big, big)
    for n_boot in (0, -1, 2.0, True, None):
        with pytest.raises(ValueError, match='n_boot'):
            E.bootstrap_pr(s, y, n_boot=n_boot)
    for seed in (-1, 2 ** 64, 1.5, True):
        with pytest.raises(ValueError, match='seed'):
            E.bootstrap_pr(s, y, seed=seed)
    with pytest.raises(ValueError, match='seed and indices are both given'):
        E.bootstrap_pr(s, y, seed=3, indices=np.zeros((2, 8), np.int64))
    with pytest.raises(ValueError, match=r'indices must lie in \[0, 8\)'):
        E.bootstrap_pr(s, y, indices=np.full((2, 8), 8))
    with pytest.raises(ValueError, match='workspace_bytes'):
        E.bootstrap_pr(s, y, workspace_bytes=0)
    with pytest.raises(ValueError, match='ranked must be a RankedScores'):
        E.pr_walk(s)
    ranked = RM.RankedScores(torch.zeros(3, 8, dtype=torch.int32), torch.zeros(3, dtype=torch.int32), s, y, False)
    for reps in (0, -1, 1.0, True, rank_abi.MAX_REPLICATES + 1):
        with pytest.raises(ValueError, match='replicates must be an integer in'):
            E.pr_walk(ranked, None, reps)
    with pytest.raises(ValueError, match='replicates must be 1 without mult'):
        E.pr_walk(ranked, None, 2)
    with pytest.raises(ValueError, match='mult must be an int32 tensor'):
        E.pr_walk(ranked, torch.zeros(8, 4), 2)
    with pytest.raises(ValueError, match=r'mult must be contiguous and hold at least n \* R4 = 8 \* 8'):
        E.pr_walk(ranked, torch.zeros(8, 4, dtype=torch.int32), 5)
    with pytest.raises(ValueError, match='mult must be contiguous'):
        E.pr_walk(ranked, torch.zeros(8, 8, dtype=torch.int32)[:, ::2], 2)
    with pytest.raises(ValueError, match='mult must be on cpu as ranked'):
        E.pr_walk(ranked, torch.zeros(8, 4, dtype=torch.int32, device='meta'), 2)
    with pytest.raises(ValueError, match='mult must be 16-byte aligned'):
        E.pr_walk(ranked, torch.zeros(8 * 4 + 1, dtype=torch.int32)[1:], 2)
    huge = RM.RankedScores(torch.empty(1, A.MAX_WEIGHT, dtype=torch.int32, device='meta'), None, None, None, False)
    with pytest.raises(ValueError, match=f'the weights of a replicate must sum to less than {A.MAX_WEIGHT}'):
        E.pr_walk(huge)
    from ecg_representation_learning_amd.metrics import _add_bootstrap
    for pr in (1, 0, None, 'yes'):
        with pytest.raises(ValueError, match='pr must be True or False'):
            _add_bootstrap({}, {}, 'eval', None, s, y, True, None, pr)
    d = {}
    _add_bootstrap(d, {}, 'eval', None, s, y, True, None)                  # the default: nothing added, nothing looked at
    assert d == {}


def test_exports_and_signatures():
    for name in ('pr_walk', 'pr_counts', 'bootstrap_pr', 'paired_diff_ci', 'PrCounts', 'PrBootstrapResult', 'pr_metrics'):
        assert name in E.__all__ and hasattr(E, name), name
    assert E.__all__.index('workload') < E.__all__.index('pr_walk') and len(set(E.__all__)) == len(E.__all__)      # appended: no earlier name moved
    assert E.bootstrap_pr is PM.bootstrap_pr and set(PM.__all__) <= set(vars(PM))
    assert list(inspect.signature(E.bootstrap_pr).parameters) == list(inspect.signature(E.bootstrap_auc).parameters)
    assert [p.default for p in inspect.signature(E.bootstrap_pr).parameters.values()] == [p.default for p in inspect.signature(E.bootstrap_auc).parameters.values()]
    assert list(inspect.signature(E.pr_walk).parameters) == ['ranked', 'mult', 'replicates']
    assert list(inspect.signature(E.pr_counts).parameters) == ['scores', 'labels', 'from_logits', 'id2code']
    assert list(inspect.signature(E.paired_diff_ci).parameters) == ['a', 'b', 'metric', 'alpha']
    for fn in (E.HipEvaluator.evaluate, E.HipKnnProbe.evaluate, E.HipKnnProbe.leave_one_out):
        ps = inspect.signature(fn).parameters
        assert ps['pr'].default is False and list(ps)[-1] == 'pr' and ps['bootstrap'].default is None


# ---- the binding table against the header ---------------------------------------------------------------------------------------------------
def test_table_is_the_header_type_by_type():
    decls = abi_header.declarations(HEADER)
    assert sorted(decls) == ['ecgvit_pr_walk'] == sorted(A.SIGNATURES)
    assert abi_header.mismatches(A.SIGNATURES, decls) == []
    assert decls['ecgvit_pr_walk'] == ('int', ['uint32_t *', 'int32_t *', 'int64_t', 'int', 'uint32_t *', 'int64_t', 'int64_t *', 'void *'])
    rank = abi_header.declarations(os.path.join(ROOT, 'include', 'ecgvit_hip_rank.h'))['ecgvit_rank_walk']
    assert decls['ecgvit_pr_walk'][1] == rank[1][:7] + rank[1][8:]                                 # the AUROC walk's parameters without `pairs`
    wrong = dict(A.SIGNATURES, ecgvit_pr_walk=(hip._I, [hip._P, hip._P, hip._I] + A.SIGNATURES['ecgvit_pr_walk'][1][3:]))
    assert len(abi_header.mismatches(wrong, decls)) == 1
    assert not set(A.SIGNATURES) & (set(hip.SIGNATURES) | set(rank_abi.SIGNATURES)) and len(hip.SIGNATURES) == 108 and hip.ABI_VERSION == 6
    assert len(abi_header.declarations()) == 108 and len(rank_abi.SIGNATURES) == 5
    lib = A.lib()
    assert lib is hip.lib() and lib.ecgvit_abi_version() == 6 and hasattr(lib, 'ecgvit_pr_walk')
    assert type(A.run) is type(hip.run) and A.run.ecgvit_pr_walk.__name__ == 'ecgvit_pr_walk'


def test_constants_are_the_headers_defines():
    text = open(HEADER).read()
    defs = {m.group(1): int(m.group(2)) for m in re.finditer(r'^#define ECGVIT_PR_([A-Z0-9_]+)\s+(-?\d+)\b', text, re.M)}
    mirrored = {n: v for n, v in vars(A).items() if n.isupper() and type(v) is int}
    assert defs == mirrored == dict(SLOTS=6, MAX_WEIGHT=1 << 30), (defs, mirrored)
    assert '#include "ecgvit_hip_rank.h"' in text and 'ecgvit_pr' not in open(os.path.join(ROOT, 'include', 'ecgvit_hip_rank.h')).read()


def test_host_side_of_the_entry_point_refuses_before_launching():
    """ECGVIT_EINVAL on bad arguments; with null or never-dereferenced pointers nothing could have been launched"""
    lib = A.lib()
    p = 4096
    good = dict(packed=p, first_nan=p, n=10, K=5, mult=p, R=2, out=p)
    for kw in (dict(packed=None), dict(first_nan=None), dict(out=None), dict(n=0), dict(n=-1), dict(n=rank_abi.MAX_ROWS + 1), dict(K=0),
               dict(K=rank_abi.MAX_CLASSES + 1), dict(R=0), dict(R=-4), dict(R=rank_abi.MAX_REPLICATES + 1), dict(mult=p + 8), dict(mult=p + 4)):
        a = dict(good, **kw)
        assert lib.ecgvit_pr_walk(a['packed'], a['first_nan'], a['n'], a['K'], a['mult'], a['R'], a['out'], None) == 1, kw
    with pytest.raises(RuntimeError, match='ecgvit_pr_walk'):
        A.run.ecgvit_pr_walk(None, None, 10, 5, None, 1, None, None)


# ---- the kernel's budget, from the built library ----------------------------------------------------------------------------------------------
def test_kernel_does_not_spill():
    """what csrc/pr_metrics.hip states: one kernel, no spill, no scratch, no LDS, within 128 registers (four waves of a workgroup per SIMD pair,
    as the AUROC walk); its name carries none of the stems by which the other features count their kernels"""
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import code_objects
    if not os.path.exists(hip.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    ks = {n: k for n, k in code_objects.kernels(hip.LIB_PATH).items() if 'prc_' in n}
    assert len(ks) == 1 and 'prc_walk_kernel' in next(iter(ks)), sorted(ks)
    (name, k), = ks.items()
    assert not any(stem in name for stem in ('rank_', 'knn_', 'kmpar_', 'rollout_', 'rs_')), name
    assert k['vgpr_spill_count'] == 0 and k['sgpr_spill_count'] == 0 and k['private_segment_fixed_size'] == 0 and k['group_segment_fixed_size'] == 0, k
    assert k['vgpr_count'] + k['agpr_count'] <= 128, k
    stated = int(re.search(r'prc_walk_kernel: (\d+) VGPRs', open(os.path.join(ROOT, 'ecg-representation-learning_amd', 'csrc', 'pr_metrics.hip')).read()).group(1))
    assert k['vgpr_count'] <= stated <= 128, (k, stated)
