"""CPU: the segment tokenizer's restatement (tests/tokenizer_ref.py) against the fixture the reference's own EcgPadder / EcgTokenizer wrote
(tests/golden/tokenizer.npz, tools/make_golden_tokenizer.py), the ABI of csrc/tokenize.hip with every refusal of its launchers (no GPU is
touched: a refused call launches nothing), and the host contract of `EcgTokenizer`."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
import abi_header
import ecg_representation_learning_amd as E
from ecg_representation_learning_amd import hip
import tokenizer_ref as R



@pytest.fixture(scope='module')
def fx():
    z = np.load(os.path.join(GOLDEN, 'tokenizer.npz'))
    return z, json.loads(bytes(z['cases']).decode())


def test_padder_reproduces_the_reference_bit_for_bit(fx):
    z, _ = fx
    for mode in ('zero', 'shift'):
        for l in z['pad_lengths'].tolist():
            x, want = z[f'pad_{mode}_{l}_in'].astype(np.float64), z[f'pad_{mode}_{l}_out']
            got = R.pad(x, 8, mode)
            assert got.shape == want.shape == (2, l + 8 - l % 8) and np.array_equal(got, want), (mode, l)
    assert R.pad(np.zeros((1, 16)), 8, 'zero').shape == (1, 24)      # k divides l: a whole extra segment


def _check_ids(segs, centers, ids_fix, ids_ref):
    """every fixture id is the restatement's argmin; where the two differ (a KDTree and a brute-force search may break an exact tie
    differently) their f64 distances agree to 1e-12 relative"""
    diff = np.flatnonzero(ids_fix != ids_ref)
    if len(diff):
        a, b = R.dist_to(segs[diff], centers, ids_fix[diff]), R.dist_to(segs[diff], centers, ids_ref[diff])
        assert np.all(np.abs(a - b) <= 1e-12 * np.maximum(a, b)), (len(diff), a, b)
    return len(diff)


def test_restatement_reproduces_the_fixture(fx):
    z, cases = fx
    th = int(z['th'])
    for i, (k, V, mode, L) in enumerate(cases):
        sig, centers, lens = z[f'case{i}_sig'], z[f'case{i}_centers'], z[f'case{i}_lens']
        segs, means = R.segments(sig, k, mode)
        T = L // k + 1
        for tag, table in (('', centers), ('_th', centers[lens >= th])):
            ids_fix, means_fix = z[f'case{i}_ids{tag}'], z[f'case{i}_means{tag}']
            assert ids_fix.shape == means_fix.shape == (3, 12, T)
            assert np.all(np.abs(means.reshape(3, 12, T) - means_fix) <= 1e-12 * np.abs(means_fix))
            ids_ref, _ = R.nearest(segs, table)
            assert ids_fix.max() < len(table)
            _check_ids(segs, table, ids_fix.reshape(-1), ids_ref)
            assert np.array_equal(z[f'case{i}_dec{tag}'], table.astype(np.float64)[ids_fix[0, :2]])
        assert 0 < (lens >= th).sum() < V      # the threshold really cuts the table


def test_lloyd_update_of_the_restatement():
    rng = np.random.default_rng(5)
    segs = rng.standard_normal((200, 8))
    ids = rng.integers(0, 5, 200)
    ids[ids == 3] = 0
    init = rng.standard_normal((5, 8))
    c, lens = R.update(segs, ids, init)
    assert lens.tolist() == [int((ids == j).sum()) for j in range(5)] and lens[3] == 0
    assert np.array_equal(c[3], init[3]) and np.allclose(c[1], segs[ids == 1].mean(0), rtol=1e-13)


# ---- ABI ----------------------------------------------------------------------------------------
ARITY = {'ecgvit_tok_assign': 20, 'ecgvit_tok_workspace': 2, 'ecgvit_tok_update': 19, 'ecgvit_tok_decode': 16}


def test_symbols_exist_with_the_declared_arity():
    lib = hip.lib()
    abi_header.held(ARITY, hip.SIGNATURES)                  # declared, with this many arguments, bound with the declaration's types
    for name in ARITY:
        assert hasattr(lib, name)
    assert lib.ecgvit_abi_version() == 6


P = 0x10000000      # never dereferenced: a refused call launches nothing


def _assign(**kw):
    a = dict(x=P, src_off=P, lead_stride=64, raw_len=P, seg_cum=P, dst_off=P, dst_stride=9, R=4, C=12, n_seg=36, k=8, pad=1, centers=P, V=37,
             prev_ids=None, ids=P, means=P, dist=P, changed=None, stream=None)
    a.update(kw)
    return hip.lib().ecgvit_tok_assign(*a.values())


def _update(**kw):
    a = dict(x=P, src_off=P, lead_stride=64, raw_len=P, seg_cum=P, dst_off=P, dst_stride=9, R=4, C=12, n_seg=36, k=8, pad=1, ids=P, centers=P, V=37,
             lens=P, workspace=P, keep_amax=0, stream=None)
    a.update(kw)
    return hip.lib().ecgvit_tok_update(*a.values())


def _decode(**kw):
    a = dict(out=P, src_off=P, lead_stride=64, raw_len=P, seg_cum=P, dst_off=P, dst_stride=9, R=4, C=12, n_seg=36, k=8, ids=P, means=P, centers=P,
             V=37, stream=None)
    a.update(kw)
    return hip.lib().ecgvit_tok_decode(*a.values())


BAD_COMMON = [dict(k=12), dict(k=4), dict(k=64), dict(k=0), dict(V=0), dict(V=65537), dict(V=-1), dict(R=0), dict(R=-3), dict(src_off=None),
              dict(raw_len=None), dict(seg_cum=None), dict(dst_off=None), dict(centers=None), dict(ids=None), dict(src_off=P + 2), dict(raw_len=P + 2),
              dict(seg_cum=P + 4), dict(dst_off=P + 2), dict(centers=P + 2), dict(ids=P + 2), dict(C=0), dict(n_seg=0)]


@pytest.mark.parametrize('bad', BAD_COMMON + [dict(x=None), dict(x=P + 2), dict(pad=2), dict(pad=-1), dict(means=None), dict(means=P + 2), dict(dist=P + 2),
                                              dict(prev_ids=P), dict(changed=P), dict(prev_ids=P + 2, changed=P), dict(prev_ids=P, changed=P + 4)],
                         ids=lambda d: ','.join(f'{k}={v}' for k, v in d.items()))
def test_assign_refusals(bad):
    assert _assign(**bad) == 1


@pytest.mark.parametrize('bad', BAD_COMMON + [dict(x=None), dict(x=P + 2), dict(pad=2), dict(lens=None), dict(lens=P + 4), dict(workspace=None),
                                              dict(workspace=P + 2), dict(keep_amax=2), dict(keep_amax=-1), dict(n_seg=2 ** 32 // 12 + 1), dict(C=1, n_seg=2 ** 32)],
                         ids=lambda d: ','.join(f'{k}={v}' for k, v in d.items()))
def test_update_refusals(bad):
    assert _update(**bad) == 1


@pytest.mark.parametrize('bad', BAD_COMMON + [dict(out=None), dict(out=P + 2), dict(means=None), dict(means=P + 2)],
                         ids=lambda d: ','.join(f'{k}={v}' for k, v in d.items()))
def test_decode_refusals(bad):
    assert _decode(**bad) == 1


def test_workspace_size():
    l = hip.lib()
    assert l.ecgvit_tok_workspace(4096, 8) == (4096 * 8 + 4096 + 2) * 8
    assert l.ecgvit_tok_workspace(0, 8) == 0 and l.ecgvit_tok_workspace(37, 12) == 0 and l.ecgvit_tok_workspace(65537, 8) == 0


# ---- host contract --------------------------------------------------------------------------------
def test_constructor_and_exports():
    assert E.EcgTokenizer is E.tokenizer.EcgTokenizer and 'EcgTokenizer' in E.__all__
    t = E.EcgTokenizer()
    assert (t.k, t.pad) == (8, 'shift') and t.centers is None and t.lens is None and t.fit_method is None and t.n_sig is None and t.cls_th is None
    for k in (8, 16, 32):
        assert E.EcgTokenizer(k=k, pad='zero').k == k
    with pytest.raises(ValueError, match='k = 12'):
        E.EcgTokenizer(k=12)
    with pytest.raises(ValueError):
        E.EcgTokenizer(pad='reflect')


def test_output_shapes_when_k_divides_the_length():
    t = E.EcgTokenizer(k=8)
    assert t.n_segments(16) == 3 and t.n_segments(61) == 8 and t.n_segments(8) == 2 and E.EcgTokenizer(k=16).n_segments(5000) == 313
    segs, means = R.segments(np.ones((2, 3, 16)), 8, 'zero')
    assert segs.shape == (2 * 3 * t.n_segments(16), 8) and means.shape == (18,)


def test_fit_refusals():
    t = E.EcgTokenizer()
    x = torch.zeros(2, 12, 64)
    with pytest.raises(NotImplementedError, match='kmeans'):
        t.fit(x, method='dbscan', cls_kwargs=dict(eps=8e-3))
    for m in ('hierarchical', 'optics', 'birch'):
        with pytest.raises(NotImplementedError):
            t.fit(x, method=m, cls_kwargs={})
    with pytest.raises(ValueError):
        t.fit(x, method='spectral', cls_kwargs={})
    with pytest.raises(NotImplementedError, match='random'):
        t.fit(x, method='kmeans', cls_kwargs=dict(n_clusters=4, init='k-means++'))
    with pytest.raises(ValueError, match='n_clusters'):
        t.fit(x, method='kmeans', cls_kwargs={})
    with pytest.raises(ValueError):
        t.fit(x, method='kmeans', cls_kwargs=dict(n_clusters=0))
    with pytest.raises(ValueError):
        t.fit(x, method='kmeans', cls_kwargs=dict(n_clusters=4, init=np.zeros((4, 7), np.float32)))
    with pytest.raises(ValueError, match='device'):                                   # a host tensor: there is no CPU fallback
        t.fit(x, method='kmeans', cls_kwargs=dict(n_clusters=4))


def test_call_refusals_and_threshold_table():
    rng = np.random.default_rng(0)
    centers, lens = rng.standard_normal((6, 8)).astype(np.float32), np.array([0, 3, 10, 11, 9, 40])
    t = E.EcgTokenizer.from_centers(centers, lens)
    assert t.k == 8 and t.centers.dtype == np.float32 and t.lens.dtype == np.int64
    with pytest.raises(ValueError, match='device'):
        t(torch.zeros(2, 12, 64))
    with pytest.raises(ValueError, match='n_pad'):                                    # l = 3 < n_pad = 5
        t(torch.zeros(2, 12, 3))
    with pytest.raises(ValueError, match='n_pad'):
        t.fit(torch.zeros(2, 12, 3), cls_kwargs=dict(n_clusters=2))
    with pytest.raises(ValueError):
        E.EcgTokenizer.from_centers(centers, lens, pad='zero')(torch.zeros(2, 12, 3))   # passes the padder's rule, stops at the host tensor
    with pytest.raises(RuntimeError):
        E.EcgTokenizer()._rows(None)
    assert np.array_equal(t._rows(10), centers[[2, 3, 5]]) and t._rows(10) is t._rows(10)       # cached per th
    assert np.array_equal(t._rows(0.5), centers[1:])       # the reference compares lens >= th against the RAW fraction: every non-empty cluster stays
    assert np.array_equal(t.decode(np.array([[1, 0]]), th=10), centers[[3, 2]][None])
    assert np.array_equal(t.decode(torch.tensor([5, 0])), centers[[5, 0]])
    with pytest.raises(ValueError):
        t._rows(41)
    t.lens = np.array([0, 3, 10, 11, 9, 5])                  # assigning the vocabulary drops what was derived from the old one
    assert np.array_equal(t._rows(10), centers[[2, 3]])
    t.centers = centers[::-1].copy()
    assert np.array_equal(t._rows(10), centers[::-1][[2, 3]])
    t.centers, t.lens = centers, lens
    with pytest.raises(ValueError):
        t._rows(1.5)
    with pytest.raises(ValueError):
        E.EcgTokenizer.from_centers(centers, lens[:5])
    with pytest.raises(ValueError):
        E.EcgTokenizer.from_centers(rng.standard_normal((6, 12)), lens)
