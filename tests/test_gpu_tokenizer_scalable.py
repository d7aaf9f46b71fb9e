"""GPU: the scalable k-means++ seeding kernels (csrc/tok_scalable.hip, ecgvit_tok_scalable_seed) and their route through `EcgTokenizer` against
the numpy restatement (tests/tokenizer_scalable_ref.py), bit for bit: the segments each round appends, the potentials, the truncation counts,
the weights, the chosen indices and the centres.  tests/test_tokenizer_scalable.py holds the restatement itself (sklearn, Python integers).

Stores are the exact stores of tests/test_gpu_tokenizer_seed.py: small integer samples, on which the mean, every distance of the unfused chain
and every weight are exact, so that equality cannot hinge on how the host and the device round -- and equal distances are common, so the tie
rules (the smaller row owns, the smaller trial wins) are exercised throughout.  Three records of 3 001 samples are 13 536 segments at k = 8
(1 128 per lead: a lead crosses the fold's workgroups of 1 024); no store here exceeds 15 000 segments."""
import numpy as np
import pytest
import torch

import ecg_representation_learning_amd as E
from ecg_representation_learning_amd import tok_scalable_abi as A
from ecg_representation_learning_amd.tokenizer import SEED_SPAN
import tokenizer_seed_ref as S
import tokenizer_scalable_ref as P

pytestmark = pytest.mark.gpu
DEV = 'cuda'
V, ELL, ROUNDS, T = 37, 74, 3, 5


def exact_store(rng, k, shape):
    """integer samples in [-20, 20] / [-8, 8] / [-4, 4]: every f32 operation on them is exact, so neither fusion nor order can matter"""
    a = {8: 20, 16: 8, 32: 4}[k]
    return rng.integers(-a, a + 1, shape).astype(np.float32)


def assert_exact(segs32, k):
    """every mean-removed sample is a multiple of 1 / k, and the largest possible distance, in units of 1 / k^2, stays below 2^24: every
    difference, square and partial sum of the chain is an integer f32 holds"""
    s = segs32[np.isfinite(segs32).all(axis=1)].astype(np.float64)
    assert np.array_equal(np.rint(s * k), s * k) and k * (2 * np.abs(s).max()) ** 2 * k * k < 2 ** 24


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def draws(seed, N, n_clusters=V, trials=T, rounds=ROUNDS):
    return E.EcgTokenizer._scalable_draws(np.random.default_rng(seed), N, n_clusters, trials, rounds)


def run_scalable(tok, st, first, keys, u0, U, n_clusters=V, ell=ELL, rounds=ROUNDS, trials=T, cap=None):
    """-> the device's result as the restatement's dict"""
    cap = P.cap_of(ell) if cap is None else cap
    centers, indices, cand_g, weights, info, _ = tok._seed_scalable(st, n_clusters, trials, rounds, ell, cap, first, keys, u0, U)
    torch.cuda.synchronize()
    h = info.cpu().numpy().view(np.uint64)
    H, n_c = A.INFO_HEAD, int(h[0])
    sel, tr = h[H:H + rounds].astype(np.int64), h[H + rounds:H + 2 * rounds].astype(np.int64)
    cg = cand_g.cpu().numpy()
    edges = np.concatenate([[1], 1 + np.cumsum(sel - tr)])
    assert edges[-1] == n_c <= 1 + rounds * cap and int(h[1]) == n_c
    return dict(rounds=[cg[edges[r]:edges[r + 1]] for r in range(rounds)], selected=sel, truncated=tr, pots=h[H + 2 * rounds:H + 3 * rounds].copy(),
                potential=int(h[H + 3 * rounds]), cand_g=cg[:n_c], weights=weights.cpu().numpy()[:n_c], n_c=n_c, indices=indices.cpu().numpy(),
                centers=centers.cpu().numpy())


def assert_same(got, want, n_clusters=V):
    for r, (a, b) in enumerate(zip(got['rounds'], want['rounds'])):
        assert np.array_equal(a, b), f'round {r}: the appended segments differ'
    for name in ('pots', 'selected', 'truncated', 'cand_g', 'weights'):
        assert np.array_equal(got[name], want[name]), name
    assert got['potential'] == want['potential'] and got['n_c'] == want['n_c'] >= n_clusters
    assert np.array_equal(got['indices'], want['indices']) and np.array_equal(bits(got['centers']), bits(want['centers']))


def same_bits(a, b):
    return all(np.array_equal(np.asarray(a[n]), np.asarray(b[n])) for n in ('pots', 'selected', 'truncated', 'cand_g', 'weights', 'indices')) and \
        np.array_equal(bits(a['centers']), bits(b['centers'])) and a['potential'] == b['potential']


# ---- 1. the restatement, every k and pad ------------------------------------------------------------------------
@pytest.mark.parametrize('k,mode', [(8, 'shift'), (8, 'zero'), (16, 'shift'), (16, 'zero'), (32, 'shift'), (32, 'zero')])
def test_three_records_equal_the_restatement(k, mode):
    sig = exact_store(np.random.default_rng(200 + k), k, (3, 12, 3001))
    segs, n_seg = S.segments32(sig, k, mode)
    assert_exact(segs, k)
    first, keys, u0, U = draws(k, len(segs))
    want = P.seed(segs, V, ELL, ROUNDS, T, first, keys, u0, U)
    tok = E.EcgTokenizer(k=k, pad=mode)
    st = tok._record_store(torch.from_numpy(sig).to(DEV), None, None)
    assert st.n_seg == n_seg == 3 * (3001 // k + 1) and (k != 8 or n_seg > SEED_SPAN)
    got = run_scalable(tok, st, first, keys, u0, U)
    print(f'k={k} {mode}: F = {want["F"]}, selected per round {got["selected"].tolist()} (restated {want["selected"].tolist()}), n_c = {got["n_c"]}, '
          f'weights sum {int(got["weights"].sum())} of {len(segs)}, candidates without weight {int((got["weights"] == 0).sum())}')
    assert_same(got, want)
    assert got['weights'].sum() == len(segs) and not got['truncated'].any() and got['selected'].min() > 0
    assert same_bits(run_scalable(tok, st, first, keys, u0, U), got)          # two runs, the same bits


def test_public_call_takes_the_documented_draws():
    k = 8
    sig = exact_store(np.random.default_rng(208), k, (3, 12, 3001))
    segs, _ = S.segments32(sig, k, 'shift')
    first, keys, u0, U = draws(11, len(segs), trials=E.KMeansPlusPlus().trials(V), rounds=5)
    want = P.seed(segs, V, ELL, 5, 5, first, keys, u0, U)
    centers, idx, info = E.EcgTokenizer(k=k).kmeans_parallel(torch.from_numpy(sig).to(DEV), V, random_state=11, return_info=True)
    assert centers.shape == (V, k) and centers.dtype == np.float32 and idx.dtype == np.int64 and sorted(info) == sorted(
        ['cand_g', 'weights', 'selected', 'truncated', 'pots', 'potential'])
    assert np.array_equal(idx, want['indices']) and np.array_equal(bits(centers), bits(segs[idx]))
    for name in ('cand_g', 'weights', 'selected', 'truncated', 'pots'):
        assert np.array_equal(info[name], want[name]), name
    assert info['potential'] == want['potential'] and len(info['pots']) == 5
    pair = E.EcgTokenizer(k=k).kmeans_parallel(torch.from_numpy(sig).to(DEV), V, random_state=11)
    assert len(pair) == 2 and np.array_equal(pair[1], idx)


# ---- 2. store forms -------------------------------------------------------------------------------------------------
def test_rectangle_ragged_and_compact_subset_agree():
    k = 8
    rng = np.random.default_rng(31)
    tok = E.EcgTokenizer(k=k, pad='shift')
    rect = exact_store(rng, k, (3, 12, 3001))
    segs, _ = S.segments32(rect, k, 'shift')
    d = draws(5, len(segs))
    want = P.seed(segs, V, ELL, ROUNDS, T, *d)
    a = run_scalable(tok, tok._record_store(torch.from_numpy(rect).to(DEV), None, None), *d)
    ragged = torch.from_numpy(np.ascontiguousarray(rect.transpose(1, 0, 2)).reshape(12, 3 * 3001)).to(DEV)
    b = run_scalable(tok, tok._record_store(ragged, np.arange(4) * 3001, None), *d)
    assert_same(a, want)
    assert same_bits(a, b)
    # a ragged store of three lengths, two of its records in another order, and the compact copy of those two
    lengths = [3001, 2500, 4017]
    recs = [exact_store(rng, k, (12, l)) for l in lengths]
    off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    store = torch.from_numpy(np.concatenate(recs, axis=1)).to(DEV)
    sel = [2, 0]
    st = tok._record_store(store, off, sel)
    segs, n_seg = S.ragged_segments32([recs[i] for i in sel], k, 'shift')
    assert st.n_seg == n_seg == 503 + 376 and n_seg < SEED_SPAN
    assert_exact(segs, k)
    d = draws(6, len(segs))
    want = P.seed(segs, V, ELL, ROUNDS, T, *d)
    c = run_scalable(tok, st, *d)
    assert_same(c, want)
    compact = torch.from_numpy(np.concatenate([recs[i] for i in sel], axis=1)).to(DEV)
    e = run_scalable(tok, tok._record_store(compact, np.array([0, 4017, 4017 + 3001]), None), *d)
    assert same_bits(c, e)
    whole = tok._record_store(store, off, None)                       # all three: more than one workgroup per lead, record boundaries inside
    assert whole.n_seg == 376 + 313 + 503 > SEED_SPAN
    segs, _ = S.ragged_segments32(recs, k, 'shift')
    d = draws(7, len(segs))
    assert_same(run_scalable(tok, whole, *d), P.seed(segs, V, ELL, ROUNDS, T, *d))


# ---- 3. more rows in a round than one chunk of the fold's row stream ------------------------------------------------
@pytest.mark.parametrize('k', [8, 32])
def test_a_round_longer_than_the_folds_chunk(k):
    ell = 400
    sig = exact_store(np.random.default_rng(300 + k), k, (3, 12, 3001))
    segs, _ = S.segments32(sig, k, 'zero')
    d = draws(k + 1, len(segs), rounds=2)
    want = P.seed(segs, V, ell, 2, T, *d)
    assert (want['selected'] - want['truncated']).max() > A.FOLD_ROWS and P.cap_of(ell) == 560     # on the test's own inputs: a second chunk is streamed
    tok = E.EcgTokenizer(k=k, pad='zero')
    got = run_scalable(tok, tok._record_store(torch.from_numpy(sig).to(DEV), None, None), *d, ell=ell, rounds=2)
    print(f'k={k}: rows appended per round {(got["selected"] - got["truncated"]).tolist()}, n_c = {got["n_c"]}')
    assert_same(got, want)


# ---- 4. edges ---------------------------------------------------------------------------------------------------------
def test_truncation_at_the_cap():
    k = 8
    sig = exact_store(np.random.default_rng(41), k, (3, 12, 3001))
    segs, _ = S.segments32(sig, k, 'shift')
    d = draws(41, len(segs))
    want = P.seed(segs, V, ELL, ROUNDS, T, *d, cap=16)
    assert want['truncated'].min() > 0 and want['n_c'] == 1 + 3 * 16 >= V
    tok = E.EcgTokenizer(k=k)
    x = torch.from_numpy(sig).to(DEV)
    got = run_scalable(tok, tok._record_store(x, None, None), *d, cap=16)
    assert_same(got, want)
    assert all(np.all(np.diff(r) > 0) and len(r) == 16 for r in got['rounds'])       # the round's first 16 in ascending g
    _, idx, info = tok.kmeans_parallel(x, V, random_state=41, n_rounds=ROUNDS, n_local_trials=T, return_info=True, _cap=16)
    assert np.array_equal(idx, want['indices']) and np.array_equal(info['truncated'], want['truncated'])
    with pytest.raises(ValueError, match=r'n_c = 17.*n_clusters = 37.*n_rounds = 1.*oversampling_factor = 2.0'):
        tok.kmeans_parallel(x, V, random_state=41, n_rounds=1, _cap=16)


def test_identical_records_leave_the_later_copy_without_weight():
    k, ell = 8, 400
    rng = np.random.default_rng(51)
    one = exact_store(rng, k, (1, 12, 3001))
    sig = np.concatenate([one, one, exact_store(rng, k, (1, 12, 3001))])
    segs, n_seg = S.segments32(sig, k, 'shift')
    d = draws(51, len(segs), rounds=2)
    want = P.seed(segs, V, ell, 2, T, *d)
    per = n_seg // 3
    lead, pos = np.divmod(want['cand_g'], n_seg)
    row_of = {(int(l), int(p)): j for j, (l, p) in enumerate(zip(lead, pos))}
    later = [j for j, (l, p) in enumerate(zip(lead, pos)) if per <= p < 2 * per and (int(l), int(p) - per) in row_of]      # record 1's copy of a candidate from record 0
    round_of = np.searchsorted(np.concatenate([[1], 1 + np.cumsum(want['selected'])]), np.arange(want['n_c']), side='right') - 1      # -1: row 0
    same_round = [j for j in later if round_of[j] >= 0 and round_of[j] == round_of[row_of[(int(lead[j]), int(pos[j]) - per)]]]
    assert not want['truncated'].any() and len(same_round) >= 5 and not want['weights'][later].any()      # on the restatement: both copies taken in one round, the later one owns nothing
    tok = E.EcgTokenizer(k=k)
    got = run_scalable(tok, tok._record_store(torch.from_numpy(sig).to(DEV), None, None), *d, ell=ell, rounds=2)
    assert_same(got, want)
    assert not got['weights'][later].any() and got['weights'].sum() == len(segs)
    assert not set(got['indices'].tolist()) & set(want['cand_g'][later].tolist())    # a row without weight is never drawn


def test_a_nan_sample_is_never_selected_and_not_counted():
    k = 8
    sig = exact_store(np.random.default_rng(61), k, (3, 12, 3001))
    sig[1, 4, 1003] = np.nan                                            # segment 125 of record 1, lead 4
    segs, n_seg = S.segments32(sig, k, 'shift')
    g_nan = 4 * n_seg + 376 + 125
    assert np.flatnonzero(np.isnan(segs).any(axis=1)).tolist() == [g_nan]
    assert_exact(segs, k)
    first, keys, u0, U = draws(61, len(segs))
    assert first != g_nan
    want = P.seed(segs, V, ELL, ROUNDS, T, first, keys, u0, U)
    tok = E.EcgTokenizer(k=k)
    st = tok._record_store(torch.from_numpy(sig).to(DEV), None, None)
    got = run_scalable(tok, st, first, keys, u0, U)
    assert_same(got, want)
    assert g_nan not in got['cand_g'].tolist() and got['weights'].sum() == len(segs) - 1
    # started on the NaN segment itself, no distance is ever finite: no potential, no candidate, no weight
    got = run_scalable(tok, st, g_nan, keys, u0, np.zeros((0, 1), np.uint64), n_clusters=1, trials=1)
    assert got['n_c'] == 1 and not got['pots'].any() and got['potential'] == 0 and got['weights'].tolist() == [0] and got['indices'].tolist() == [g_nan]


def test_identical_segments_end_the_rounds_at_once():
    tok = E.EcgTokenizer(k=8, pad='shift')
    x = torch.full((2, 12, 100), 0.5, device=DEV)                    # every mean-removed segment is zero: pot == 0 after row 0
    total = 2 * 12 * 13
    centers, idx, info = tok.kmeans_parallel(x, 1, random_state=5, return_info=True)
    first = int(np.random.default_rng(5).integers(total))
    assert idx.tolist() == [first] and not centers.any() and info['cand_g'].tolist() == [first] and info['weights'].tolist() == [total]
    assert not info['pots'].any() and not info['selected'].any() and info['potential'] == 0
    with pytest.raises(ValueError, match=r'n_c = 1 candidates, fewer than n_clusters = 2'):
        tok.kmeans_parallel(x, 2, random_state=5)
    with pytest.raises(ValueError, match=r'n_c = 1 candidates'):
        E.EcgTokenizer(k=8).fit(x, cls_kwargs=dict(n_clusters=2, init=E.ScalableKMeansPlusPlus(), random_state=5))


# ---- 5. through fit -----------------------------------------------------------------------------------------------------
def test_fit_seeded_by_the_scalable_seeding():
    k = 8
    sig = exact_store(np.random.default_rng(71), k, (3, 12, 3001))
    x = torch.from_numpy(sig).to(DEV)
    before = x.clone()
    centers, idx = E.EcgTokenizer(k=k).kmeans_parallel(x, V, random_state=3)
    kw = dict(n_clusters=V, max_iter=6)
    one = E.EcgTokenizer(k=k).fit(x, cls_kwargs=dict(kw, init=E.ScalableKMeansPlusPlus(), n_init=1, random_state=3))
    start = E.EcgTokenizer(k=k).fit(x, cls_kwargs=dict(kw, init=centers))
    assert np.array_equal(one.centers, start.centers) and np.array_equal(one.lens, start.lens) and one.inertia_ == start.inertia_
    assert one.changed_ == start.changed_ and int(one.lens.sum()) == 12 * 3 * 376 and torch.equal(x, before)
    # restarts: the same generator gives the seedings in order, the second one on the kept workspace and its kept maximum
    init = E.ScalableKMeansPlusPlus(n_rounds=2, n_local_trials=2)
    two = E.EcgTokenizer(k=k).fit(x, cls_kwargs=dict(kw, init=init, n_init=2, random_state=4))
    again = E.EcgTokenizer(k=k).fit(x, cls_kwargs=dict(kw, init=init, n_init=2, random_state=4))
    assert np.array_equal(two.centers, again.centers) and np.array_equal(two.lens, again.lens) and two.inertia_ == again.inertia_
    rng = np.random.default_rng(4)
    probe = E.EcgTokenizer(k=k)
    c1, i1 = probe.kmeans_parallel(x, V, random_state=rng, n_rounds=2, n_local_trials=2)
    c2, i2 = probe.kmeans_parallel(x, V, random_state=rng, n_rounds=2, n_local_trials=2)
    assert not np.array_equal(i1, i2)
    f1 = E.EcgTokenizer(k=k).fit(x, cls_kwargs=dict(kw, init=c1))
    f2 = E.EcgTokenizer(k=k).fit(x, cls_kwargs=dict(kw, init=c2))
    better = f1 if f1.inertia_ <= f2.inertia_ else f2
    assert two.inertia_ == better.inertia_ and np.array_equal(two.centers, better.centers) and np.array_equal(two.lens, better.lens)
    with pytest.raises(NotImplementedError, match='random'):           # the string stays refused on the device as on the host
        E.EcgTokenizer(k=k).fit(x, cls_kwargs=dict(n_clusters=V, init='scalable-k-means++'))
