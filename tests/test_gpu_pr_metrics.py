"""-m gpu: average precision and class-wise F-max on the device (csrc/pr_metrics.hip) against the Python-integer restatement (tests/pr_ref.py).
All six integers of every (replicate, class) are compared exactly; only the host's f64 divisions are held to a tolerance, against the restatement's
own.  The restatement itself is held to scikit-learn on the CPU (tests/test_pr_metrics.py)."""
import numpy as np
import pytest
import torch

import ecg_representation_learning_amd as E
from ecg_representation_learning_amd import pr_abi as A, rank_abi
from ecg_representation_learning_amd.hip import ptr, stream
import pr_ref as P
import rank_ref as R

pytestmark = pytest.mark.gpu
NS = (1, 2, 63, 64, 65, 255, 256, 257, 1025, 2049)          # lane (4), step (256) and sort-tile (2048) edges of the walk
RS = (1, 4, 5, 16, 17)                                       # a partial quad, a whole workgroup of four waves, one replicate past it
NAN = float('nan')


def dev(a, gap=3):
    """the (n, K) array on the device with row pitch K + gap and NaN in the gap"""
    n, K = a.shape
    buf = torch.full((n + 1, K + gap), NAN, device='cuda')
    buf[:n, :K] = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return buf[:n, :K]


def mult_tensor(mult):
    """(R, n) multiplicities -> the record-major (n, R4) int32 device tensor of the header"""
    m = np.asarray(mult)
    R_, n = m.shape
    out = np.zeros((n, (R_ + 3) // 4 * 4), np.int32)
    out[:, :R_] = m.T
    return torch.from_numpy(out).cuda()


def same(got, want):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    assert got.shape == want.shape and got.dtype == np.int64
    bad = np.argwhere((got != want).any(axis=-1))
    assert len(bad) == 0, (bad[:4].tolist(), [(got[tuple(b)].tolist(), want[tuple(b)].tolist()) for b in bad[:4]])


# ---- every store at every n: unit weights and seeded replicates ----------------------------------------------------------------------------------
@pytest.mark.parametrize('n', NS)
def test_every_store_at_every_edge(n):
    """the ten stores of pr_ref.COLUMNS (all equal, all distinct, a 1/8 grid, a tie group across a step's end and one across a lane's end, NaN rows, a
    class whose positives are all NaN, a class without a positive, one without a negative, -0 / +0): unit weights, then R seeded replicates"""
    s, y = P.special_store(np.random.default_rng([7, n]), n)
    ds, dy = dev(s), dev(y)
    ranked = E.rank_scores(ds, dy)
    same(E.pr_walk(ranked), P.sixes(s, y))
    R_ = RS[NS.index(n) % len(RS)]
    res = E.bootstrap_pr(ds, dy, n_boot=R_, seed=n)
    want = P.sixes(s, y, np.stack([R.multiplicities(n, r, n) for r in range(R_)]))
    same(res.sixes, want)
    point = res.point
    if n >= 2:
        valid = [c for c in range(len(P.COLUMNS)) if 0 < y[:, c].sum() < n]
        assert list(point['per_class_ap']) == valid == list(point['per_class_fmax']) == list(point['per_class_threshold'])
        for c, v in zip(valid, P.sixes(s, y)[0][valid]):
            ap, f, thr = P.values(v, s[:, c])
            assert abs(point['per_class_ap'][c] - ap) <= 1e-15 and abs(point['per_class_fmax'][c] - f) <= 1e-15
            assert point['per_class_threshold'][c] == (float('inf') if thr is None else thr)
        assert abs(point['macro_ap'] - np.mean(list(point['per_class_ap'].values()))) <= 1e-15
        if 6 in valid:
            assert point['per_class_ap'][6] == 0.0 and point['per_class_fmax'][6] == 0.0 and point['per_class_threshold'][6] == float('inf')
    else:
        assert point == dict(macro_ap=None, per_class_ap=None, macro_fmax=None, per_class_fmax=None, per_class_threshold=None)


@pytest.mark.parametrize('R_', RS)
@pytest.mark.parametrize('K', [1, 3, 71])
def test_every_replicate_count_and_width(K, R_):
    """n = 257: a whole step and one position, K classes on the grid's y, R replicates from given indices through the entry points themselves"""
    n = 257
    rng = np.random.default_rng([11, K, R_])
    s, y = R.store('nan' if K == 3 else 'grid', rng, n, K), R.labels_for(rng, n, K)
    idx = rng.integers(0, n, (R_, n))
    idx[0] = np.arange(n)                                                    # the identity: the point estimate
    mult = R.from_indices(idx, n)
    ranked = E.rank_scores(dev(s), dev(y))
    m = torch.full((n, (R_ + 3) // 4 * 4), -1, dtype=torch.int32, device='cuda')
    rank_abi.run.ecgvit_rank_multiplicities(ptr(torch.from_numpy(idx).cuda()), n, R_, n, ptr(m), stream())
    got = E.pr_walk(ranked, m, R_)
    same(got, P.sixes(s, y, mult))
    same(got[:1], P.sixes(s, y))
    assert torch.equal(E.pr_walk(ranked, mult_tensor(mult), R_), got)
    assert torch.equal(E.pr_walk(ranked), got[:1])                           # null mult: unit weights


def test_terms_beyond_53_bits():
    """hand-made weights near 2^26 on n = 8: (TP_g - TP_{g-1}) * TP_g passes 2^53, where an f64 quotient is no longer the floor; the sum of the
    weights stays below 2^30"""
    s = np.array([[1, 3], [1, 2], [1, 2], [1, 2], [0, 1], [0, 1], [0, 0], [0, 0]], np.float32)
    y = np.array([[1, 1], [1, 1], [1, 1], [0, 0], [1, 1], [0, 0], [1, 1], [0, 0]], np.float32)
    big = (1 << 26) - np.array([[0, 1, 2, 3, 5, 7, 11, 13], [13, 11, 7, 5, 3, 2, 1, 0], [1, 0, 0, 0, 0, 0, 0, 0]], np.int64)
    mult = np.concatenate([big, np.array([[(1 << 29) - 9, 0, 0, 1, 0, 0, 0, 0], [1, 1, 1, 1, 1, 1, 1, 1]], np.int64)])
    assert (mult.sum(axis=1) < A.MAX_WEIGHT).all()
    want = P.sixes(s, y, mult)
    tp = int(big[0, :3].sum())
    assert tp * tp > 1 << 53 and int(float(tp * tp * (1 << 32)) / float(tp + int(big[0, 3]))) != tp * tp * (1 << 32) // (tp + int(big[0, 3]))
    ranked = E.rank_scores(dev(s), dev(y))
    same(E.pr_walk(ranked, mult_tensor(mult), 5), want)


# ---- replicates: chunking, indices, the AUROC route beside it ------------------------------------------------------------------------------------
N, KB = 333, 5


def boot_case(kind='grid'):
    rng = np.random.default_rng([3, N, R.KINDS.index(kind)])
    s, y = R.store(kind, rng, N, KB), R.labels_for(rng, N, KB)
    y[:, 3] = 0
    y[:6, 3] = 1                                                             # a rare class: replicates without a positive exist
    return s, y


@pytest.mark.parametrize('kind', ['grid', 'nan'])
def test_chunking_and_the_auroc_route(kind):
    s, y = boot_case(kind)
    ds, dy = dev(s), dev(y)
    quad = rank_abi.lib().ecgvit_rank_workspace(N, KB, 4)
    whole = E.bootstrap_pr(ds, dy, n_boot=37, seed=11)
    cut = E.bootstrap_pr(ds, dy, n_boot=37, seed=11, workspace_bytes=2 * quad + 7)
    assert (whole.chunk, cut.chunk) == (37, 8)
    mult = np.stack([R.multiplicities(11, r, N) for r in range(37)])
    want = P.sixes(s, y, mult)
    same(whole.sixes, want)
    same(cut.sixes, want)
    assert np.array_equal(whole.per_class_ap, cut.per_class_ap, equal_nan=True) and whole.ci('ap') == cut.ci('ap') and whole.ci('fmax') == cut.ci('fmax')
    assert whole.point == cut.point == E.pr_counts(ds, dy).result()
    again = E.bootstrap_pr(ds, dy, n_boot=37, seed=11)                       # a second run: equal bits
    assert np.array_equal(again.sixes, whole.sixes) and again.point == whole.point
    assert (whole.n, whole.n_boot, whole.seed, whole.source) == (N, 37, 11, ('seed', 11))
    # the AUROC replicates are what they were: the restatement's triples, and the same resamples as the PR replicates
    auc = E.bootstrap_auc(ds, dy, n_boot=37, seed=11)
    assert np.array_equal(auc.triples, R.triples(s, y, mult)) and auc.point == E.get_accuracy(ds, dy)
    assert np.array_equal(auc.triples[..., 1:], whole.sixes[..., 1:3]) and (auc.n, auc.n_boot, auc.seed, auc.source) == (N, 37, 11, ('seed', 11))
    assert np.array_equal(E.bootstrap_auc(ds, dy, n_boot=37, seed=11, workspace_bytes=2 * quad + 7).triples, auc.triples)
    # values on the resample: AP and F-max of the restatement, replicate by replicate
    for b in (0, 5, 36):
        for c in range(KB):
            if want[b, c, 1] > 0 and want[b, c, 2] > 0:
                ap, f, _ = P.values(want[b, c])
                assert abs(whole.per_class_ap[b, c] - ap) <= 1e-15 and abs(whole.per_class_fmax[b, c] - f) <= 1e-15
            else:
                assert np.isnan(whole.per_class_ap[b, c]) and np.isnan(whole.per_class_fmax[b, c])
    assert np.array_equal(whole.n_valid, (~np.isnan(whole.per_class_ap)).sum(axis=0)) and whole.class_ci('fmax').shape == (KB, 2)
    # paired differences: one seed pairs, another is refused
    worse = E.bootstrap_pr(dev(1 - np.nan_to_num(s)), dy, n_boot=37, seed=11)
    lo, hi = E.paired_diff_ci(whole, worse, 'ap')
    assert lo <= hi and E.paired_diff_ci(whole, whole, 'fmax') == (0.0, 0.0) and E.paired_diff_ci(auc, auc, 'auc') == (0.0, 0.0)
    with pytest.raises(ValueError, match='b was not resampled as a: source'):
        E.paired_diff_ci(whole, E.bootstrap_pr(ds, dy, n_boot=37, seed=12), 'ap')
    with pytest.raises(ValueError, match='b was not resampled as a: n_boot'):
        E.paired_diff_ci(whole, E.bootstrap_pr(ds, dy, n_boot=36, seed=11), 'ap')


def test_replicates_from_indices():
    s, y = boot_case()
    ds, dy = dev(s), dev(y)
    rng = np.random.default_rng(4)
    idx = rng.integers(0, N, (6, N))
    idx[0], idx[1] = np.arange(N), 17                                        # the identity; one record N times: every class invalid
    idx[2] = rng.choice(np.flatnonzero(y[:, 3] == 0), N)                     # no positive of class 3
    row = rank_abi.lib().ecgvit_rank_workspace(N, KB, 4) // 4
    res = E.bootstrap_pr(ds, dy, indices=idx, workspace_bytes=4 * row)
    mult = R.from_indices(idx, N)
    same(res.sixes, P.sixes(s, y, mult))
    assert res.chunk == 4 and res.seed is None and res.source[:2] == ('indices', 6)
    same(res.sixes[:1], P.sixes(s, y))
    assert np.isnan(res.per_class_ap[1]).all() and np.isnan(res.macro_fmax[1]) and np.isnan(res.per_class_fmax[2, 3]) and not np.isnan(res.macro_ap[2])
    on_device = E.bootstrap_pr(ds, dy, indices=torch.from_numpy(idx).cuda())
    assert np.array_equal(on_device.sixes, res.sixes) and on_device.source == res.source
    auc = E.bootstrap_auc(ds, dy, indices=idx)
    assert np.array_equal(auc.triples, R.triples(s, y, mult)) and auc.source == res.source and auc.seed is None


# ---- the surfaces ------------------------------------------------------------------------------------------------------------------------------
LMAX, PATCH, KS = 600, 20, 7
POINT = ('macro_ap', 'per_class_ap', 'macro_fmax', 'per_class_fmax', 'per_class_threshold')
CI = ('macro_auc_ci', 'per_class_auc_ci', 'macro_ap_ci', 'per_class_ap_ci', 'macro_fmax_ci', 'per_class_fmax_ci')


def _model():
    torch.manual_seed(3)
    conf = E.EcgVitConfig(max_signal_length=LMAX, patch_size=PATCH, hidden_size=128, num_hidden_layers=2, num_attention_heads=2,
                          intermediate_size=256, hidden_dropout_prob=0.1, attention_probs_dropout_prob=0.1)
    return E.EcgVit(num_class=KS, config=conf, compute_dtype=torch.bfloat16).cuda()


def _records():
    g = torch.Generator().manual_seed(29)
    x = torch.randn(48, 12, LMAX, generator=g).cuda()
    y = (torch.rand(48, KS, generator=g) < 0.3).float().cuda()
    return x, y


def _check_surface(old, boot, new, both, prefix):
    assert not any(k.split('/')[1] in POINT + CI[2:] for k in old) and not any(k.split('/')[1] in POINT + CI[2:] for k in boot)
    assert set(new) == set(old) | {f'{prefix}/{k}' for k in POINT} and all(new[k] == old[k] for k in old)
    assert set(both) == set(new) | {f'{prefix}/{k}' for k in CI} and all(both[k] == new[k] for k in new)
    assert all(both[f'{prefix}/{k}'] == boot[f'{prefix}/{k}'] for k in CI[:2])                     # the AUROC intervals are what `bootstrap` alone gives
    classes = set(old[f'{prefix}/per_class_auc'])
    for k in ('per_class_ap', 'per_class_fmax', 'per_class_threshold'):
        assert set(new[f'{prefix}/{k}']) == classes
    for m in ('ap', 'fmax'):
        lo, hi = both[f'{prefix}/macro_{m}_ci']
        assert 0.0 <= lo <= hi <= 1.0 and 0.0 < new[f'{prefix}/macro_{m}'] <= 1.0
        per = both[f'{prefix}/per_class_{m}_ci']
        assert set(per) == classes and all(0.0 <= a <= b <= 1.0 for a, b in per.values())


def test_evaluator_keys():
    x, y = _records()
    ev = E.HipEvaluator(_model(), eval_batch_size=16)
    old, boot, new = ev.evaluate(x, y), ev.evaluate(x, y, bootstrap=16), ev.evaluate(x, y, pr=True)
    out = ev.evaluate(x, y, bootstrap=16, pr=True, return_predictions=True)
    _check_surface(old, boot, new, out['metrics'], 'eval')
    pred = out['predictions']
    by_hand = E.bootstrap_pr(pred['logits'], y, n_boot=16, from_logits=True)
    assert np.array_equal(by_hand.sixes, pred['bootstrap_pr'].sixes) and by_hand.point == pred['bootstrap_pr'].point
    assert np.array_equal(E.bootstrap_auc(pred['logits'], y, n_boot=16, from_logits=True).triples, pred['bootstrap'].triples)
    assert new['eval/per_class_ap'] == by_hand.point['per_class_ap']
    # predicting `logit >= threshold` attains F-max
    c = next(iter(new['eval/per_class_threshold']))
    hit = pred['logits'][:, c] >= new['eval/per_class_threshold'][c]
    tp, fp, wp = int((hit & (y[:, c] != 0)).sum()), int((hit & (y[:, c] == 0)).sum()), int((y[:, c] != 0).sum())
    assert abs(2 * tp / (tp + fp + wp) - new['eval/per_class_fmax'][c]) <= 1e-15
    assert set(ev.evaluate(x, y, pr=True, return_predictions=True)['predictions']) == {'labels', 'logits'}


def test_knn_probe_keys():
    x, y = _records()
    probe = E.HipKnnProbe(_model(), k=5, batch_size=16)
    old, boot, new = probe.leave_one_out(x, y), probe.leave_one_out(x, y, bootstrap=16), probe.leave_one_out(x, y, pr=True)
    _check_surface(old, boot, new, probe.leave_one_out(x, y, bootstrap=16, pr=True), 'knn')
    plain = probe.evaluate(x[:32], y[:32], x[32:], y[32:])
    out = probe.evaluate(x[:32], y[:32], x[32:], y[32:], bootstrap=dict(n_boot=8, seed=5), pr=True, return_predictions=True)
    assert not any(k.split('/')[1] in POINT for k in plain) and all(f'knn/{k}' in out['metrics'] for k in POINT + CI)
    assert out['predictions']['bootstrap_pr'].sixes.shape == (8, KS, 6) and out['predictions']['bootstrap_pr'].source == ('seed', 5)
