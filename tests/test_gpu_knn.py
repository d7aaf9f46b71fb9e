"""-m gpu: the k-NN search, merge, normalise and vote kernels (csrc/knn.hip) against the numpy restatement (tests/knn_ref.py), and `HipKnnProbe`
against its parts composed by hand.

Exact stores: integers in [-8, 8] as f32; with d <= 2048 every partial sum of a score stays below 2^24, so the f32 chain, numpy's f32 product
and the f64 product are the same number and indices AND scores must equal the restatement's, ties included (every query row has ties).
Random store: the bound of a d-term f32 chain, tol = (d + 2) 2^-24 sum_i |q_i b_i|, with no cap on mismatches and no left-out case."""
import numpy as np
import pytest
import torch

import ecg_representation_learning_amd as E
from ecg_representation_learning_amd import knn
import knn_ref as R

pytestmark = pytest.mark.gpu
NAN = float('nan')


def fenced(a, gap=3):
    """the (rows, d) array on the device with row pitch d + gap: NaN in the gap, and a NaN row directly after the last one"""
    rows, d = a.shape
    buf = torch.full((rows + 1, d + gap), NAN, device='cuda')
    buf[:rows, :d] = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    view = buf[:rows, :d]
    assert view.stride(0) == d + gap or rows == 1
    return view


def dot_search(q, b, k, **kw):
    s, i = E.KnnIndex(b, metric='dot').search(q, k, **kw)
    return s.cpu().numpy(), i.cpu().numpy()


def same(got, want):
    return np.array_equal(got[0], want[0].astype(np.float32)) and np.array_equal(got[1], want[1])


# ---- exact stores -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('d', [1, 31, 32, 33, 768, 2048])
def test_exact_stores_equal_the_restatement_ties_included(d):
    rng = np.random.default_rng(d)
    bank_all, query_all = R.integer_store(rng, 1000, d), R.integer_store(rng, 129, d)
    s_all = R.scores64(query_all, bank_all)
    assert np.array_equal((query_all @ bank_all.T).astype(np.float64), s_all)           # f32 product == f64 product: the store is exact
    assert all(len(np.unique(row)) < 1000 for row in s_all)                             # every query row has ties
    done = 0
    for k in (1, 20, 256):
        for N in sorted({1, k, 127, 128, 129, 1000}):
            if N < k:
                continue
            b = fenced(bank_all[:N])
            for Q in (1, 33, 129):
                q = fenced(query_all[:Q])
                got = dot_search(q, b, k)
                want = R.select(s_all[:Q, :N], k)
                assert same(got, want), (d, Q, N, k, np.argwhere(got[1] != want[1])[:4])
                done += 1
    assert done == 3 * (5 + 5 + 2)


@pytest.mark.parametrize('k', [31, 32, 33, 64])
def test_both_list_forms_at_their_boundary(k):
    """k <= 32: the lists in LDS, a pair per lane; above: in the workspace, an owner thread per query"""
    rng = np.random.default_rng(k)
    b, q = R.integer_store(rng, 1000, 33), R.integer_store(rng, 129, 33)
    s_all = R.scores64(q, b)
    bd, qd = fenced(b), fenced(q)
    for splits in (1, 3):
        assert same(dot_search(qd, bd, k, splits=splits), R.select(s_all, k)), splits
    assert same(dot_search(qd, bd[:k], k), R.select(s_all[:, :k], k))
    assert same(dot_search(bd[:129], bd, k, exclude_self=True), R.select(R.scores64(b[:129], b), k, self_base=0))


# ---- the selection path -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('k', [1, 20, 32, 33, 256])
def test_selection_rising_falling_and_all_equal(k):
    N, Q = 1000, 33
    q = np.zeros((Q, 2), np.float32)
    q[:, 0] = np.arange(1, Q + 1)                                     # positive multiples of the bank's first column: small integers, exact
    ramp = np.zeros((N, 2), np.float32)
    ramp[:, 0] = np.arange(N)
    qd = torch.from_numpy(q).cuda()
    rising = dot_search(qd, torch.from_numpy(ramp).cuda(), k)         # every row beats the threshold
    assert same(rising, R.search(q, ramp, k)) and rising[1][0].tolist() == list(range(N - 1, N - 1 - k, -1))
    falling = dot_search(qd, torch.from_numpy(-ramp).cuda(), k)       # none does after the first k
    assert same(falling, R.search(q, -ramp, k)) and falling[1][0].tolist() == list(range(k))
    ones = np.ones((N, 2), np.float32)
    equal = dot_search(qd, torch.from_numpy(ones).cuda(), k, splits=7)
    assert np.array_equal(equal[1], np.tile(np.arange(k), (Q, 1))) and same(equal, R.search(q, ones, k))


def test_splits_give_the_same_bits():
    rng = np.random.default_rng(5)
    bi, qi = R.integer_store(rng, 1000, 33), R.integer_store(rng, 129, 33)
    bf, qf = rng.standard_normal((1000, 96)).astype(np.float32), rng.standard_normal((129, 96)).astype(np.float32)
    for b, q, exact in ((bi, qi, True), (bf, qf, False)):
        bd, qd = torch.from_numpy(b).cuda(), torch.from_numpy(q).cuda()
        index = E.KnnIndex(bd, metric='dot')
        first = None
        for splits in (1, 2, 7, 0, None, 1024):
            s, i = index.search(qd, 20, splits=splits)
            if first is None:
                first = (s, i)
                if exact:
                    assert same((s.cpu().numpy(), i.cpu().numpy()), R.search(q, b, 20))
            assert torch.equal(s.view(torch.int32), first[0].view(torch.int32)) and torch.equal(i, first[1]), splits
    # a batch of queries and each query alone: the same bits
    index = E.KnnIndex(torch.from_numpy(bf).cuda(), metric='dot')
    whole = index.search(torch.from_numpy(qf).cuda(), 20)
    for r in (0, 64, 128):
        alone = index.search(torch.from_numpy(qf[r:r + 1]).cuda(), 20)
        assert torch.equal(alone[0].view(torch.int32), whole[0][r:r + 1].view(torch.int32)) and torch.equal(alone[1], whole[1][r:r + 1])


# ---- leave-one-out -----------------------------------------------------------------------------------------------------
def test_exclude_self_is_by_index():
    rng = np.random.default_rng(9)
    b = R.integer_store(rng, 129, 33)
    b[100] = b[3]                                                     # twins: the excluded row's twin is still returned
    b[50] = b[60]
    bd = fenced(b)
    s_all = R.scores64(b, b)
    got = dot_search(bd, bd, 20, exclude_self=True)                   # Q = N = 129, self_base = 0
    assert same(got, R.select(s_all, 20, self_base=0))
    assert not (got[1] == np.arange(129)[:, None]).any()
    assert 100 in got[1][3] and 3 in got[1][100] and 60 in got[1][50] and 50 in got[1][60]
    assert same(dot_search(bd, bd, 128, exclude_self=True), R.select(s_all, 128, self_base=0))      # k = N - 1: everything but the own row
    # a slice of the bank as the queries, and shifted indices
    got = dot_search(bd[40:73], bd, 20, exclude_self=True, self_base=40, index_base=1000)
    want = R.select(s_all[40:73], 20, self_base=40, index_base=1000)
    assert same(got, want) and not (got[1] == 1040 + np.arange(33)[:, None]).any() and got[1].min() >= 1000
    assert 1060 in got[1][10] and 1050 in got[1][20]
    # without the exclusion the own row (or its twin, the smaller index) leads: a row's largest score is with itself or a longer row
    plain = dot_search(bd[40:73], bd, 20, index_base=1000)
    assert same(plain, R.select(s_all[40:73], 20, index_base=1000))


# ---- non-finite scores ------------------------------------------------------------------------------------------------
def test_non_finite_scores_never_enter_a_list():
    rng = np.random.default_rng(11)
    b, q = R.integer_store(rng, 300, 33), R.integer_store(rng, 5, 33)
    q[:, 0] = np.abs(q[:, 0]) + 1                                     # column 0 of every query is non-zero: an inf there gives an inf score
    clean = R.search(q, b, 20)
    bad = b.copy()
    bad[7] = np.nan
    bad[130, 0] = np.inf
    bad[131, 0] = -np.inf
    bad[299, 5] = np.nan
    qn = q.copy()
    qn[2] = np.nan                                                    # a NaN query: no admissible row
    got = dot_search(torch.from_numpy(qn).cuda(), torch.from_numpy(bad).cuda(), 20)
    s = R.scores64(q, b)
    s[:, [7, 130, 131, 299]] = np.nan
    s[2] = np.nan
    want = R.select(s, 20)
    assert same(got, want)
    assert (got[1][2] == -1).all() and np.isneginf(got[0][2]).all()
    assert not np.isin(got[1], [7, 130, 131, 299]).any() and np.isfinite(got[0][[0, 1, 3, 4]]).all()
    keep = ~np.isin(clean[1], [7, 130, 131, 299])                     # the finite rows ranked as without the others
    for r in (0, 1, 3, 4):
        kept = clean[1][r][keep[r]]
        assert np.array_equal(got[1][r][:len(kept)], kept)
    # fewer admissible rows than k: -1 / -inf in the remaining slots
    few = np.full((30, 33), np.nan, np.float32)
    few[[4, 9, 20]] = b[[4, 9, 20]]
    got = dot_search(torch.from_numpy(q).cuda(), torch.from_numpy(few).cuda(), 8)
    s = np.full((5, 30), np.nan)
    s[:, [4, 9, 20]] = R.scores64(q, b[[4, 9, 20]])
    assert same(got, R.select(s, 8)) and (got[1][:, 3:] == -1).all() and np.isneginf(got[0][:, 3:]).all() and (got[1][:, :3] >= 0).all()


# ---- merge -------------------------------------------------------------------------------------------------------------
def test_merge_of_chunks_is_one_search():
    rng = np.random.default_rng(13)
    b, q = R.integer_store(rng, 1000, 33), R.integer_store(rng, 33, 33)
    bd, qd = torch.from_numpy(b).cuda(), torch.from_numpy(q).cuda()
    whole = E.KnnIndex(bd, metric='dot').search(qd, 20)
    parts = [E.KnnIndex(bd[lo:hi], metric='dot').search(qd, min(20, hi - lo), index_base=lo) for lo, hi in ((0, 400), (400, 410), (410, 1000))]
    got = E.knn_merge(parts, 20)
    assert torch.equal(got[0], whole[0]) and torch.equal(got[1], whole[1])
    assert same((got[0].cpu().numpy(), got[1].cpu().numpy()), R.search(q, b, 20))
    # -1 slots are ignored, unsorted lists are merged, a pair that stands twice is taken once, too few pairs end on -1 / -inf
    s = torch.tensor([[1.0, 3.0, -np.inf, 2.0], [5.0, NAN, 5.0, 5.0]]).cuda()
    i = torch.tensor([[4, 9, -1, 6], [8, 2, 1, 8]]).cuda()
    ms, mi = E.knn_merge([(s, i), (s[:, :2], i[:, :2])], 4)
    want = R.merge([(s.cpu().numpy(), i.cpu().numpy()), (s[:, :2].cpu().numpy(), i[:, :2].cpu().numpy())], 4)
    assert mi.cpu().tolist() == [[9, 6, 4, -1], [1, 8, -1, -1]] and np.array_equal(mi.cpu().numpy(), want[1])
    assert np.array_equal(ms.cpu().numpy(), want[0])
    wide = E.knn_merge([E.KnnIndex(bd, metric='dot').search(qd, 256, splits=s_) for s_ in (1, 8)], 256)      # 512 slots per query, each pair twice
    assert same((wide[0].cpu().numpy(), wide[1].cpu().numpy()), R.search(q, b, 256))
    # more than 2 048 slots per query: the merge that reads its input again in every sweep, from knn_merge and inside a search
    parts = [E.KnnIndex(bd, metric='dot').search(qd, 256, splits=s_) for s_ in (1, 2, 3, 4, 5, 6, 7, 8, 1)]
    many = E.knn_merge(parts, 256)
    assert torch.equal(many[0], wide[0]) and torch.equal(many[1], wide[1])
    b2 = R.integer_store(rng, 1300, 33)
    assert same(dot_search(qd, torch.from_numpy(b2).cuda(), 256, splits=11), R.search(q, b2, 256))


# ---- the random store --------------------------------------------------------------------------------------------------
def test_random_store_within_the_f32_chain_bound():
    Q, N, d, k = 64, 1000, 768, 20
    rng = np.random.default_rng(17)
    q, b = rng.standard_normal((Q, d)).astype(np.float32), rng.standard_normal((N, d)).astype(np.float32)
    s64 = R.scores64(q, b)
    tol = (d + 2) * 2.0 ** -24 * (np.abs(q).astype(np.float64) @ np.abs(b).astype(np.float64).T)
    got_s, got_i = dot_search(torch.from_numpy(q).cuda(), torch.from_numpy(b).cuda(), k)
    assert (got_i >= 0).all() and (got_i < N).all() and all(len(set(row)) == k for row in got_i.tolist())
    rows = np.arange(Q)[:, None]
    err = np.abs(got_s.astype(np.float64) - s64[rows, got_i]) / tol[rows, got_i]
    print(f'[knn random store] worst |score - f64| / tol = {err.max():.4f}')
    assert (err <= 1.0).all()                                                                    # (a)
    later = (got_s[:, 1:] < got_s[:, :-1]) | ((got_s[:, 1:] == got_s[:, :-1]) & (got_i[:, 1:] > got_i[:, :-1]))
    assert later.all()                                                                           # (b) sorted under the total order
    # (c) a row that was left out ranks, in f32, at or after every returned row M: s64_out - tol_out <= s32_out <= s32_M <= s64_M + tol_M
    for r in range(Q):
        out = np.setdiff1d(np.arange(N), got_i[r])
        m = got_i[r][np.argmin(s64[r, got_i[r]])]
        assert (s64[r, out] <= s64[r, m] + tol[r, out] + tol[r, m]).all(), r
    print(f'[knn random store] queries whose order is the f64 order: {int((got_i == R.select(s64, k)[1]).all(axis=1).sum())} of {Q}')


# ---- normalise ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('d', [1, 33, 768, 2048])
def test_normalize_within_one_ulp(d):
    rng = np.random.default_rng(d)
    x = (rng.standard_normal((37, d)) * np.exp(rng.uniform(-20, 20, (37, 1)))).astype(np.float32)
    x[5] = 0.0
    got = knn.normalize(fenced(x)).cpu().numpy()
    want = R.normalize(x)
    assert got.shape == x.shape and not np.isnan(got).any()
    ulp = np.spacing(np.abs(want))
    assert (np.abs(got.astype(np.float64) - want.astype(np.float64)) <= ulp).all()
    assert (got[5] == 0).all()
    x[6, 0] = np.nan
    bad = knn.normalize(torch.from_numpy(x).cuda()).cpu().numpy()
    assert np.isnan(bad[6]).all() and np.array_equal(bad[[0, 5, 36]], got[[0, 5, 36]])
    if d == 33:                                                       # the cosine index: normalised rows, then the dot search
        b = rng.standard_normal((200, d)).astype(np.float32)
        s, i = E.knn_search(torch.from_numpy(x[:5]).cuda(), torch.from_numpy(b).cuda(), 10)
        nb = knn.normalize(torch.from_numpy(b).cuda())
        s2, i2 = E.KnnIndex(nb, metric='dot').search(knn.normalize(torch.from_numpy(x[:5]).cuda()), 10)
        assert torch.equal(s, s2) and torch.equal(i, i2) and float(s.max()) <= 1.0 + 1e-6


# ---- vote --------------------------------------------------------------------------------------------------------------
def test_vote():
    rng = np.random.default_rng(23)
    N, K, Q, k = 300, 71, 40, 20
    y = (rng.random((N, K)) < 0.2).astype(np.float32)
    b, q = rng.standard_normal((N, 48)).astype(np.float32), rng.standard_normal((Q, 48)).astype(np.float32)
    index = E.KnnIndex(torch.from_numpy(b).cuda())
    s, i = index.search(torch.from_numpy(q).cuda(), k)
    i[3] = -1                                                         # a query with no neighbour
    i[4, 5:] = -1                                                     # -1 slots are skipped
    i[6, ::2] = -1
    yd = fenced(y, gap=5)
    sn, ni = s.cpu().numpy(), i.cpu().numpy()
    uni = index.vote(s, i, yd, weights='uniform').cpu().numpy()
    assert np.array_equal(uni, R.vote(sn, ni, y, 'uniform')) and (uni[3] == 0).all()
    assert np.array_equal(uni[4], (y[ni[4, :5]].astype(np.float64).sum(0) / 5).astype(np.float32))
    for T in (0.07, 1.0):
        soft = index.vote(s, i, yd, weights='softmax', temperature=T).cpu().numpy()
        ref = R.vote(sn, ni, y, 'softmax', T).astype(np.float64)      # fed the device's own scores
        assert (np.abs(soft - ref) <= 2.0 ** -23 * np.abs(ref) + 1e-30).all(), T
        assert (soft[3] == 0).all() and soft.min() >= 0 and soft.max() <= 1
    assert np.array_equal(index.vote(s[:, :1], i[:, :1], yd, weights='softmax').cpu().numpy()[[0, 1]], y[ni[[0, 1], 0]])     # k = 1: the neighbour's labels
    with pytest.raises(ValueError, match='labels have 299 rows, the bank has 300'):
        index.vote(s, i, yd[:299])


# ---- the refusals that need a device ------------------------------------------------------------------------------------
def test_refusals_on_the_device():
    b, q = torch.zeros(8, 16, device='cuda'), torch.zeros(4, 16, device='cuda')
    index = E.KnnIndex(b)
    with pytest.raises(ValueError, match='queries must be a device tensor'):
        index.search(q.cpu(), 3)
    with pytest.raises(ValueError, match='queries have d = 15'):
        index.search(q[:, :15], 3)
    for k in (0, 9):
        with pytest.raises(ValueError, match='k must be an integer'):
            index.search(q, k)
    with pytest.raises(ValueError, match=r'in \[1, 7\]'):
        index.search(q, 8, exclude_self=True)
    with pytest.raises(ValueError, match='splits'):
        index.search(q, 3, splits=1025)
    with pytest.raises(ValueError, match='queries must be float32'):
        index.search(q.double(), 3)
    s, i = index.search(q, 8)                                         # a zero bank under the cosine metric: zero rows stay zero, scores 0
    assert i.tolist() == [list(range(8))] * 4 and (s == 0).all()


# ---- the probe ---------------------------------------------------------------------------------------------------------
LMAX, PATCH, K = 600, 20, 7


def _model(dtype=torch.bfloat16):
    torch.manual_seed(3)
    conf = E.EcgVitConfig(max_signal_length=LMAX, patch_size=PATCH, hidden_size=128, num_hidden_layers=2, num_attention_heads=2,
                          intermediate_size=256, hidden_dropout_prob=0.1, attention_probs_dropout_prob=0.1)
    return E.EcgVit(num_class=K, config=conf, compute_dtype=dtype).cuda()


def _ragged(x, lengths):
    return torch.cat([x[r, :, :int(n)] for r, n in enumerate(lengths)], dim=1).contiguous()


@pytest.mark.parametrize('form', ['padded', 'lengths', 'ragged'])
def test_knn_probe_is_its_parts_composed_by_hand(form):
    g = torch.Generator().manual_seed(31)
    nb, nq = 24, 8
    xb, xq = torch.randn(nb, 12, LMAX, generator=g).cuda(), torch.randn(nq, 12, LMAX, generator=g).cuda()
    yb, yq = (torch.rand(nb, K, generator=g) < 0.3).float().cuda(), (torch.rand(nq, K, generator=g) < 0.3).float().cuda()
    lb = torch.tensor([PATCH * int(v) for v in torch.randint(1, LMAX // PATCH + 1, (nb,), generator=g)])
    lq = torch.tensor([PATCH * int(v) for v in torch.randint(1, LMAX // PATCH + 1, (nq,), generator=g)])
    lb[0], lq[0] = LMAX, LMAX
    if form == 'padded':
        lb = lq = None
    elif form == 'ragged':
        xb, xq = _ragged(xb, lb), _ragged(xq, lq)
    m = _model().train()
    probe = E.HipKnnProbe(m, k=5, batch_size=7)
    out = probe.evaluate(xb, yb, xq, yq, bank_lengths=lb, query_lengths=lq, return_predictions=True)
    assert m.training                                                 # the flag is as it was
    enc = E.HipEncoder(m, batch_size=7)
    fb, fq = enc.encode(xb, lengths=lb), enc.encode(xq, lengths=lq)
    index = E.KnnIndex(fb)
    s, i = index.search(fq, 5)
    probs = index.vote(s, i, yb, weights='softmax', temperature=0.07)
    want = E.get_accuracy(probs, yq)
    pred = out['predictions']
    assert torch.equal(pred['scores'], s) and torch.equal(pred['indices'], i) and torch.equal(pred['probabilities'], probs) and pred['labels'] is yq
    assert out['metrics'] == {f'knn/{key}': v for key, v in want.items()}
    assert set(out['metrics']) == {'knn/binary_accuracy', 'knn/weighted_binary_accuracy', 'knn/binary_negative_recall', 'knn/binary_positive_recall',
                                   'knn/macro_auc', 'knn/per_class_auc'}
    assert probe.evaluate(xb, yb, xq, yq, bank_lengths=lb, query_lengths=lq) == out['metrics']
    # leave-one-out: the set as its own bank, the own record excluded by index
    loo = probe.leave_one_out(xb, yb, lengths=lb, return_predictions=True)
    s, i = index.search(fb, 5, exclude_self=True)
    probs = index.vote(s, i, yb)
    assert torch.equal(loo['predictions']['indices'], i) and torch.equal(loo['predictions']['scores'], s)
    assert not (i == torch.arange(nb, device='cuda')[:, None]).any()
    assert loo['metrics'] == {f'knn/{key}': v for key, v in E.get_accuracy(probs, yb).items()}
    m.eval()
    assert probe.leave_one_out(xb, yb, lengths=lb) == loo['metrics'] and not m.training
    other = E.HipKnnProbe(m, k=3, weights='uniform', pool='mean', norm=False, batch_size=64).evaluate(xb, yb, xq, yq, bank_lengths=lb, query_lengths=lq)
    assert set(other) == set(out['metrics'])
    with pytest.raises(ValueError, match='bank_y has 23 rows'):
        probe.evaluate(xb, yb[:23], xq, yq, bank_lengths=lb, query_lengths=lq)
