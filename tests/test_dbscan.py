"""CPU: the DBSCAN restatement (tests/dbscan_ref.py) against sklearn.cluster.DBSCAN, and the host contract of `Dbscan`, `EcgTokenizer.segments`,
`EcgTokenizer.dbscan` and `fit(method=Dbscan())`: every refusal that is raised before a device is asked for, the launchers' refusals (a refused
call launches nothing) and the constants the GPU tests build their edge cases from.

Exact-integer stores: samples are integers in -2 .. 2, so a mean-removed sample is a multiple of 1 / k of magnitude at most 4, a squared
distance a multiple of 1 / k^2 below k * 8^2 (in units of 1 / k^2: 32 * 64 * 32^2 = 2^21 < 2^24), and eps a half-integer whose square is
exact: every decision is the same in f32 and f64, and a pair at exactly eps is a neighbour in both."""

import numpy as np
import pytest
import torch

import abi_header
import ecg_representation_learning_amd as E
from ecg_representation_learning_amd import hip, tokenizer
import dbscan_ref as D



def test_restatement_equals_sklearn_on_exact_integer_stores():
    seeds = range(100, 172)
    several = ties = contested = 0
    for seed in seeds:
        k, mode, eps, ms, x = D.integer_case(seed)
        assert x.min() >= -2 and x.max() <= 2 and np.array_equal(x, np.rint(x)) and (2 * eps) % 1 == 0 and 2 <= ms <= 5
        segs, _ = D.segments32(x, k, mode)
        assert np.array_equal(segs * k, np.rint(segs * k))                         # the mean removal was exact
        r = D.run(segs, eps, ms)
        core, labels = D.sklearn_dbscan(segs, eps, ms)
        assert np.array_equal(r['core'], core) and np.array_equal(r['labels'], labels), (seed, k, mode, eps, ms)
        several += r['clusters'] > 1
        ties += r['ties'] > 0
        contested += r['contested'] > 0
    print(f'{len(seeds)} stores: {several} with more than one cluster, {ties} with a pair at exactly eps, {contested} with a border segment two clusters see')
    assert len(seeds) >= 60 and several > 0 and ties > 0 and contested > 0


# (seed, eps): the band of every one is asserted below, on the test's own inputs
WALKS = {(8, 'zero'): (1, 0.06), (8, 'shift'): (1, 0.06), (16, 'zero'): (1, 0.14), (16, 'shift'): (1, 0.14), (32, 'zero'): (1, 0.35), (32, 'shift'): (1, 0.35)}


@pytest.mark.parametrize('k,mode', sorted(WALKS))
def test_restatement_equals_sklearn_on_random_walk_stores(k, mode):
    """general data: no pair lies within 2e-5 of eps (about ten times the f32 chain's bound (k + 2) 2^-24 at k = 32), so the f32 and the f64
    comparison decide every pair alike"""
    seed, eps = WALKS[(k, mode)]
    segs, _ = D.segments32(D.random_walk_store(seed, k), k, mode)
    r = D.run(segs, eps, 5)
    print(f'k={k} {mode}: {len(segs)} segments, band {r["band"]:.3e}, {r["clusters"]} clusters, {len(r["core"])} core, {r["noise"]} noise')
    assert r['band'] > 2e-5
    assert 0 < len(r['core']) < len(segs) and r['clusters'] >= 2 and r['noise'] > 0
    core, labels = D.sklearn_dbscan(segs, eps, 5)
    assert np.array_equal(r['core'], core) and np.array_equal(r['labels'], labels)


def test_restatement_puts_a_non_finite_segment_aside():
    segs, _ = D.segments32(D.random_walk_store(7, 8), 8, 'zero')
    want = D.dbscan(np.delete(segs, 11, axis=0), 0.08, 3)[1]
    segs[11, 3] = np.nan
    core, labels = D.dbscan(segs, 0.08, 3)
    assert labels[11] == -1 and 11 not in core and np.array_equal(np.delete(labels, 11), want)


# ---- the method object and the refusals ---------------------------------------------------------------
def test_method_object_and_exports():
    assert E.Dbscan is tokenizer.Dbscan and 'Dbscan' in E.__all__
    assert repr(E.Dbscan()) == 'Dbscan(min_samples=5)' and repr(E.Dbscan(min_samples=3)) == 'Dbscan(min_samples=3)'
    assert E.Dbscan().min_samples == 5
    for bad in (0, -1, 2.5, None, True):
        with pytest.raises(ValueError, match='min_samples'):
            E.Dbscan(min_samples=bad)
    t = E.EcgTokenizer()
    assert t.n_noise is None and t.labels_ is None


def test_refusals_before_a_device_is_asked_for():
    t = E.EcgTokenizer()
    x = torch.zeros(2, 12, 64)
    with pytest.raises(NotImplementedError, match='kmeans'):                         # the string stays refused: it promises sklearn's arithmetic
        t.fit(x, method='dbscan', cls_kwargs=dict(eps=8e-3))
    for bad in (0, 0.0, -1.0, float('nan'), float('inf'), None, 'a', 1e30):
        with pytest.raises(ValueError, match='eps'):
            t.dbscan(x, bad)
        with pytest.raises(ValueError, match='eps'):
            t.fit(x, method=E.Dbscan(), cls_kwargs=dict(eps=bad))
    with pytest.raises(ValueError, match='eps'):
        t.fit(x, method=E.Dbscan(), cls_kwargs={})
    with pytest.raises(ValueError, match='eps'):
        t.fit(x, method=E.Dbscan())
    for bad in (0, -3, 1.5):
        with pytest.raises(ValueError, match='min_samples'):
            t.dbscan(x, 0.1, min_samples=bad)
        with pytest.raises(ValueError, match='min_samples'):
            t.fit(x, method=E.Dbscan(), cls_kwargs=dict(eps=0.1, min_samples=bad))
    with pytest.raises(ValueError, match='n_clusters'):
        t.fit(x, method=E.Dbscan(), cls_kwargs=dict(eps=0.1, n_clusters=4))
    with pytest.raises(ValueError, match='algorithm'):
        t.fit(x, method=E.Dbscan(), cls_kwargs=dict(eps=0.1, algorithm='brute'))
    for call in (lambda: t.dbscan(x, 0.1), lambda: t.segments(x), lambda: t.fit(x, method=E.Dbscan(), cls_kwargs=dict(eps=0.1)),
                 lambda: t.dbscan(x.numpy(), 0.1)):
        with pytest.raises(ValueError, match='device'):                              # a host tensor: there is no CPU fallback
            call()
    with pytest.raises(ValueError, match='n_pad'):
        t.dbscan(torch.zeros(2, 12, 3), 0.1)
    big = torch.empty((2 ** 20, 12, 2 ** 11), device='meta')                         # 2^20 * 12 * 257 segments, no memory behind them
    for call in (lambda: t.dbscan(big, 0.1), lambda: t.segments(big), lambda: t.fit(big, method=E.Dbscan(), cls_kwargs=dict(eps=0.1))):
        with pytest.raises(ValueError, match=r'2\^31'):
            call()


def test_eps_squared_is_formed_in_f32():
    for eps in (0.1, 8e-3, 1.5, 3):
        e = np.float32(eps)
        assert tokenizer.check_eps(eps) == float(np.float32(e * e)) == float(D.eps_squared(eps))


# ---- ABI ----------------------------------------------------------------------------------------------
ARITY = {'ecgvit_tok_segments': 16, 'ecgvit_tok_dbscan_count': 8, 'ecgvit_tok_dbscan_link': 8, 'ecgvit_tok_dbscan_flatten': 4,
         'ecgvit_tok_dbscan_border': 11, 'ecgvit_tok_dbscan_rows': 1}


def test_symbols_constants_and_abi():
    lib = hip.lib()
    abi_header.held(ARITY, hip.SIGNATURES)                  # declared, with this many arguments, bound with the declaration's types
    for name in ARITY:
        assert hasattr(lib, name)
    assert lib.ecgvit_abi_version() == 6
    assert lib.ecgvit_tok_dbscan_tile() == tokenizer.DBSCAN_TILE
    assert {k: lib.ecgvit_tok_dbscan_rows(k) for k in (8, 16, 32)} == tokenizer.DBSCAN_ROWS and lib.ecgvit_tok_dbscan_rows(12) == 0
    assert tokenizer.DBSCAN_PAIRS_PER_LAUNCH == 1 << 40


def test_row_blocks_hold_the_launch_bound(monkeypatch):
    t = E.EcgTokenizer(k=8)
    rpb = tokenizer.DBSCAN_ROWS[8]
    assert t._row_blocks(5000, 5000) == [(0, 5000)]
    monkeypatch.setattr(tokenizer, 'DBSCAN_PAIRS_PER_LAUNCH', 3 * rpb * 5000)
    assert t._row_blocks(5000, 5000) == [(0, 3 * rpb), (3 * rpb, 5000)]
    monkeypatch.setattr(tokenizer, 'DBSCAN_PAIRS_PER_LAUNCH', 1)                    # never less than one workgroup's rows
    assert t._row_blocks(2 * rpb + 1, 7) == [(0, rpb), (rpb, 2 * rpb), (2 * rpb, 2 * rpb + 1)]
    assert t._row_blocks(1, 1) == [(0, 1)]


P = 0x10000000      # never dereferenced: a refused call launches nothing


def _count(**kw):
    a = dict(segs=P, n=100, k=8, eps2=1.0, row0=0, row1=100, count=P, stream=None)
    a.update(kw)
    return hip.lib().ecgvit_tok_dbscan_count(*a.values())


def _link(**kw):
    a = dict(core=P, m=100, k=8, eps2=1.0, row0=0, row1=100, parent=P, stream=None)
    a.update(kw)
    return hip.lib().ecgvit_tok_dbscan_link(*a.values())


def _border(**kw):
    a = dict(rows=P, nrows=100, core=P, core_label=P, m=50, k=8, eps2=1.0, row0=0, row1=100, label=P, stream=None)
    a.update(kw)
    return hip.lib().ecgvit_tok_dbscan_border(*a.values())


def _segments(**kw):
    a = dict(x=P, src_off=P, lead_stride=64, raw_len=P, seg_cum=P, dst_off=P, dst_stride=9, R=4, C=12, n_seg=36, k=8, pad=1, segs=P, means=P, dst=None,
             stream=None)
    a.update(kw)
    return hip.lib().ecgvit_tok_segments(*a.values())


SWEEP_BAD = [dict(k=12), dict(k=0), dict(k=64), dict(eps2=-1.0), dict(eps2=float('inf')), dict(eps2=float('nan')), dict(row0=-1), dict(row0=100),
             dict(row0=50, row1=50), dict(row1=101)]
ids = lambda d: ','.join(f'{k}={v}' for k, v in d.items())


@pytest.mark.parametrize('bad', SWEEP_BAD + [dict(segs=None), dict(segs=P + 8), dict(n=0), dict(count=None), dict(count=P + 2)], ids=ids)
def test_count_refusals(bad):
    assert _count(**bad) == 1


@pytest.mark.parametrize('bad', SWEEP_BAD + [dict(core=None), dict(core=P + 4), dict(m=0), dict(parent=None), dict(parent=P + 1)], ids=ids)
def test_link_refusals(bad):
    assert _link(**bad) == 1


@pytest.mark.parametrize('bad', SWEEP_BAD + [dict(rows=None), dict(rows=P + 8), dict(core=None), dict(core=P + 8), dict(m=0), dict(nrows=0), dict(core_label=None),
                                             dict(core_label=P + 2), dict(label=None), dict(label=P + 2)], ids=ids)
def test_border_refusals(bad):
    assert _border(**bad) == 1


@pytest.mark.parametrize('bad', [dict(k=12), dict(pad=2), dict(x=None), dict(R=0), dict(C=0), dict(n_seg=0), dict(segs=None), dict(segs=P + 8), dict(means=None),
                                 dict(means=P + 2), dict(dst=P + 4), dict(src_off=None), dict(seg_cum=P + 4), dict(n_seg=2 ** 31 // 12 + 1), dict(C=1, n_seg=2 ** 31)],
                         ids=ids)
def test_segments_refusals(bad):
    assert _segments(**bad) == 1


def test_flatten_refusals():
    f = hip.lib().ecgvit_tok_dbscan_flatten
    assert f(None, 4, P, None) == 1 and f(P, 4, None, None) == 1 and f(P, 0, P, None) == 1 and f(P + 2, 4, P, None) == 1
