"""-m gpu: the rank route to AUROC (csrc/rank_metrics.hip) against the numpy restatement (tests/rank_ref.py) and against the all-pairs kernel of
`eval_counts` on the same device.  Everything is an integer and is compared exactly: the packed order word for word, the 4 + 2K counts element for
element, the (num2, wp, wn) triples of every replicate; only the host's f64 divisions are held to 1e-12 against `get_accuracy_np` on the resampled
arrays."""
import numpy as np
import pytest
import torch

import ecg_representation_learning_amd as E
from ecg_representation_learning_amd import rank_abi as A
from ecg_representation_learning_amd.hip import ptr, stream
from oracle.metrics_oracle import get_accuracy_np
import rank_ref as R

pytestmark = pytest.mark.gpu
T = A.TILE
NAN = float('nan')


def fenced(a, gap=3):
    """the (n, K) array on the device with row pitch K + gap: NaN in the gap, and a NaN row directly after the last one"""
    n, K = a.shape
    buf = torch.full((n + 1, K + gap), NAN, device='cuda')
    buf[:n, :K] = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    view = buf[:n, :K]
    assert view.stride(0) == K + gap
    return view


def case(kind, n, K, seed=0):
    rng = np.random.default_rng([seed, n, K, R.KINDS.index(kind)])
    return R.store(kind, rng, n, K), R.labels_for(rng, n, K)


# ---- the sort ------------------------------------------------------------------------------------------------------------------------------
# (n, K): the edges of a wave step (64) and of a tile (T), several tiles, both class counts at every n; 70 001 rows: indices past 16 bits; the scan's
# internal widths, K = 1 -- ECGVIT_RANK_SCAN_BATCH = 8 tiles per step of the run over a digit's tiles: 9 tiles is the smallest count that takes a
# second step (the scan's other width, the 256 digit totals summed by one workgroup, does not depend on the shape: every case runs it whole)
SHAPES = [(n, K) for n in (1, 2, 63, 64, 65, T - 1, T, T + 1, 3 * T + 5) for K in (1, 71)] + [(70001, 2), (A.SCAN_BATCH * T + 1, 1)]


@pytest.mark.parametrize('kind', R.KINDS)
@pytest.mark.parametrize('n,K', SHAPES)
def test_order_is_the_restatements(n, K, kind):
    s, y = case(kind, n, K)
    ranked = E.rank_scores(fenced(s), fenced(y))
    got, first = ranked.packed.cpu().numpy().view(np.uint32), ranked.first_nan.cpu().numpy()
    assert got.shape == (K, n)
    for c in range(K):
        word, nan0 = R.packed(R.keys(s[:, c]), y[:, c])
        assert np.array_equal(got[c], word) and first[c] == nan0, (c, np.flatnonzero(got[c] != word)[:8])
    assert np.array_equal(ranked.order(K - 1).cpu().numpy(), R.order(R.keys(s[:, K - 1])))


def test_sort_is_the_same_bits_twice():
    s, y = case('nan', 3 * T + 5, 5)
    a, b = E.rank_scores(fenced(s), fenced(y)), E.rank_scores(fenced(s), fenced(y))
    assert torch.equal(a.packed, b.packed) and torch.equal(a.first_nan, b.first_nan)


# ---- the point estimate: the all-pairs kernel on the same device is the reference --------------------------------------------------------------
def point_case(kind, n, seed=1):
    """six classes; class 4 without a positive, class 5 without a negative"""
    s, y = case(kind, n, 6, seed)
    y[:, 4], y[:, 5] = 0, 1
    if kind != 'nan':
        s[::7, 1] = np.nan                                   # NaN scores in every kind's store as well
    return s, y


@pytest.mark.parametrize('from_logits', [False, True])
@pytest.mark.parametrize('kind', R.KINDS)
def test_counts_are_the_all_pairs_kernels(kind, from_logits):
    s, y = point_case(kind, T + 5)
    if from_logits:
        with np.errstate(over='ignore'):
            s = (s - np.float32(0.5)) * np.float32(8)        # both signs, ties kept (the two kernels share one as_prob)
    ds, dy = fenced(s), fenced(y)
    want = E.eval_counts(ds, dy, from_logits=from_logits)
    got = E.auroc_counts(ds, dy, from_logits=from_logits)
    assert got.counts.dtype == want.counts.dtype and torch.equal(got.counts, want.counts), (got.counts.tolist(), want.counts.tolist())
    assert got.result() == want.result()
    assert set(got.result()['per_class_auc']) == {0, 1, 2, 3}


def test_counts_at_70001_rows_and_names():
    s, y = case('grid', 70001, 2, 2)
    s[5::11, 0] = np.nan
    ds, dy = fenced(s), fenced(y)
    want, got = E.eval_counts(ds, dy, id2code=['a', 'b']), E.auroc_counts(ds, dy, id2code=['a', 'b'])
    assert torch.equal(got.counts, want.counts) and got.result() == want.result() and set(got.result()['per_class_auc']) == {'a', 'b'}
    assert np.array_equal(got.counts.cpu().numpy()[4 + 2:], R.triples(s, y)[0, :, 0])


# ---- replicates ------------------------------------------------------------------------------------------------------------------------------
N, KB = 333, 5


def boot_case(kind='grid', n=N):
    s, y = case(kind, n, KB, 3)
    y[:, 3] = 0
    y[:6, 3] = 1                                             # a rare class: replicates without a positive exist
    return s, y


def indices_for(R_, y, seed=4):
    """row 0 the identity permutation, row 1 one record N times, row 2 no positive of class 3, then plain draws"""
    rng = np.random.default_rng(seed)
    idx = rng.integers(0, N, (R_, N))
    idx[0] = np.arange(N)
    if R_ > 1:
        idx[1] = 17
    if R_ > 2:
        idx[2] = rng.choice(np.flatnonzero(y[:, 3] == 0), N)
    return idx


def check_against_reference(res, s, y, idx):
    for b, row in enumerate(idx):
        want = get_accuracy_np(s[row], y[row])
        per = want['per_class_auc'] or {}
        for c in range(KB):
            got = res.per_class_auc[b, c]
            assert (np.isnan(got) and c not in per) or abs(got - per[c]) <= 1e-12, (b, c, got, per.get(c))
        assert (np.isnan(res.macro_auc[b]) and want['macro_auc'] is None) or abs(res.macro_auc[b] - want['macro_auc']) <= 1e-12, b


@pytest.mark.parametrize('kind', ['grid', 'nan'])
@pytest.mark.parametrize('R_,chunk', [(1, 4), (3, 4), (5, 4), (37, 36)])      # chunks are whole quads of replicates: 4 + 1, 36 + 1
def test_replicates_from_indices(R_, chunk, kind):
    s, y = boot_case(kind)
    idx = indices_for(R_, y)
    ds, dy = fenced(s), fenced(y)
    row = A.lib().ecgvit_rank_workspace(N, KB, 4) // 4
    res = E.bootstrap_auc(ds, dy, indices=idx, workspace_bytes=chunk * row)
    assert res.chunk == min(chunk, R_) and res.triples.shape == (R_, KB, 3) and res.triples.dtype == np.int64
    assert np.array_equal(res.triples, R.triples(s, y, R.from_indices(idx, N)))
    point = E.eval_counts(ds, dy)
    assert res.point == point.result()
    assert np.array_equal(res.triples[0, :, 0], point.counts.cpu().numpy()[4 + KB:])          # the identity permutation is the point estimate
    if R_ > 1:
        assert np.isnan(res.per_class_auc[1]).all() and np.isnan(res.macro_auc[1])               # one record N times: every class invalid
    if R_ > 2:
        assert res.triples[2, 3, 1] == 0 and np.isnan(res.per_class_auc[2, 3]) and not np.isnan(res.macro_auc[2])
    with np.errstate(invalid='ignore'):
        check_against_reference(res, s, y, idx)                                                  # (numpy compares NaN as the all-pairs kernel does)
    assert np.array_equal(res.n_valid, (~np.isnan(res.per_class_auc)).sum(axis=0))
    again = E.bootstrap_auc(ds, dy, indices=torch.from_numpy(idx).cuda(), workspace_bytes=chunk * row)      # device indices, a second run: equal bits
    assert np.array_equal(again.triples, res.triples) and np.array_equal(again.per_class_auc, res.per_class_auc, equal_nan=True)
    lo, hi = res.ci()
    assert (np.isnan(lo) and np.isnan(res.macro_auc).all()) or lo <= hi
    assert res.class_ci().shape == (KB, 2)


def test_seeded_multiplicities_are_the_restatements():
    n, R_, seed, first = 1000, 6, 2 ** 63 + 12345, 3
    mult = torch.full((n, 8), -1, dtype=torch.int32, device='cuda')            # record-major, six replicates padded to eight columns
    assert A.lib().ecgvit_rank_workspace(n, 1, R_) == n * 8 * 4 + (-n * 8 * 4) % 256
    A.run.ecgvit_rank_multiplicities_seeded(seed, first, R_, n, ptr(mult), stream())
    want = np.stack([R.multiplicities(seed, first + r, n) for r in range(R_)])
    got = mult.cpu().numpy()
    assert np.array_equal(got[:, :R_].T, want) and (got[:, R_:] == 0).all() and (want.sum(axis=1) == n).all()
    idx = np.stack([R.draws(seed, first + r, n) for r in range(R_)])
    mult.fill_(-1)
    A.run.ecgvit_rank_multiplicities(ptr(torch.from_numpy(idx).cuda()), n, R_, n, ptr(mult), stream())
    assert np.array_equal(mult.cpu().numpy(), got)


@pytest.mark.parametrize('n', [N, 3 * A.WALK_ROWS + 5])             # a partial second step of the walk; several steps
@pytest.mark.parametrize('kind', ['grid', 'nan'])
def test_seeded_replicates_and_chunking(kind, n):
    s, y = boot_case(kind, n)
    ds, dy = fenced(s), fenced(y)
    quad = A.lib().ecgvit_rank_workspace(n, KB, 4)
    whole = E.bootstrap_auc(ds, dy, n_boot=37, seed=11)
    cut = E.bootstrap_auc(ds, dy, n_boot=37, seed=11, workspace_bytes=2 * quad + 7)
    tiny = E.bootstrap_auc(ds, dy, n_boot=37, seed=11, workspace_bytes=1)                       # below one quad: one replicate at a time
    assert (whole.chunk, cut.chunk, tiny.chunk) == (37, 8, 1) and np.array_equal(tiny.triples, whole.triples)
    want = R.triples(s, y, np.stack([R.multiplicities(11, r, n) for r in range(37)]))
    assert np.array_equal(whole.triples, want) and np.array_equal(cut.triples, want)
    assert np.array_equal(whole.per_class_auc, cut.per_class_auc, equal_nan=True) and np.array_equal(whole.macro_auc, cut.macro_auc, equal_nan=True)
    assert whole.ci() == cut.ci() and whole.point == cut.point
    other = E.bootstrap_auc(ds, dy, n_boot=37, seed=12)
    assert not np.array_equal(other.triples, whole.triples)
    # two score sets under one seed are resampled identically: wp / wn of every replicate agree
    paired = E.bootstrap_auc(fenced(1 - np.nan_to_num(s)), dy, n_boot=37, seed=11)
    assert np.array_equal(paired.triples[..., 1:], whole.triples[..., 1:])


# ---- the surfaces ------------------------------------------------------------------------------------------------------------------------------
LMAX, PATCH, KS = 600, 20, 7
OLD = ('binary_accuracy', 'weighted_binary_accuracy', 'binary_negative_recall', 'binary_positive_recall', 'macro_auc', 'per_class_auc')


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


def _check_surface(old, new, prefix):
    assert set(old) == {f'{prefix}/{k}' for k in OLD} | ({'eval/loss'} if prefix == 'eval' else set())
    assert set(new) == set(old) | {f'{prefix}/macro_auc_ci', f'{prefix}/per_class_auc_ci'}
    assert all(new[k] == old[k] for k in old)
    lo, hi = new[f'{prefix}/macro_auc_ci']
    assert 0.0 <= lo <= hi <= 1.0
    per = new[f'{prefix}/per_class_auc_ci']
    assert set(per) == set(old[f'{prefix}/per_class_auc']) and all(0.0 <= a <= b <= 1.0 for a, b in per.values())


def test_evaluator_bootstrap():
    x, y = _records()
    ev = E.HipEvaluator(_model(), eval_batch_size=16)
    old = ev.evaluate(x, y)
    new = ev.evaluate(x, y, bootstrap=16, return_predictions=True)
    _check_surface(old, new['metrics'], 'eval')
    res = new['predictions']['bootstrap']
    assert res.triples.shape == (16, KS, 3) and res.ci() == new['metrics']['eval/macro_auc_ci']
    by_hand = E.bootstrap_auc(new['predictions']['logits'], y, n_boot=16, from_logits=True)
    assert np.array_equal(by_hand.triples, res.triples)
    assert ev.evaluate(x, y, bootstrap=dict(n_boot=16, seed=0)) == new['metrics']
    assert set(ev.evaluate(x, y, return_predictions=True)['predictions']) == {'labels', 'logits'}


def test_knn_probe_bootstrap():
    x, y = _records()
    probe = E.HipKnnProbe(_model(), k=5, batch_size=16)
    old = probe.leave_one_out(x, y)
    new = probe.leave_one_out(x, y, bootstrap=16)
    _check_surface(old, new, 'knn')
    out = probe.evaluate(x[:32], y[:32], x[32:], y[32:], bootstrap=dict(n_boot=8, seed=5), return_predictions=True)
    assert out['predictions']['bootstrap'].triples.shape == (8, KS, 3) and 'knn/macro_auc_ci' in out['metrics']
