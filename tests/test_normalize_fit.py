"""CPU: `fit_dynamic_normalize`'s host side -- argument parsing against the reference's forms, the stage-composition algebra against the
fixture with the raw statistics supplied by numpy, every refusal, and the ABI symbols of csrc/fit_stats.hip."""
import ctypes
import math
import os
import re
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT
import abi_header
import ecg_representation_learning_amd as E
from ecg_representation_learning_amd import hip, transform as T
import normalize_cases as NC

sys.path.insert(0, os.path.join(ROOT, 'tools'))


def test_parse_normalize_takes_the_references_forms():
    assert T.parse_normalize('global') == [('global', None)]
    assert T.parse_normalize('none') == [('none', None)]
    assert T.parse_normalize('std') == [('std', 1)] and T.parse_normalize('norm') == [('norm', 2)]          # transform.py:60-61
    assert T.parse_normalize(('std', 3)) == [('std', 3)] and T.parse_normalize(('norm', 2.5)) == [('norm', 2.5)]
    assert T.parse_normalize(('std',)) == [('std', 1)]
    assert T.parse_normalize((('norm', 3), ('std', 1))) == [('norm', 3), ('std', 1)]                         # the default, a tuple of tuples
    assert T.parse_normalize([('norm', 3), 'std', ('global',)]) == [('norm', 3), ('std', 1), ('global', None)]
    assert T.parse_normalize(('global', 7)) == [('global', None)]                                             # the reference drops the arg
    import inspect
    assert inspect.signature(E.fit_dynamic_normalize).parameters['normalize'].default == (('norm', 3), ('std', 1))
    assert E.fit_dynamic_normalize is T.fit_dynamic_normalize and 'fit_dynamic_normalize' in E.__all__


@pytest.mark.parametrize('bad', ['zscore', ('std', '3'), ('std', 1, 2), ['std', 'global'], [('norm', 3), ('minmax',)], (), [], None, 3,
                                 ('std', 0), ('norm', -1), ('std', float('nan')), ('norm', float('inf')), [['norm', 3]]])
def test_parse_normalize_refusals(bad):
    with pytest.raises(ValueError):
        T.parse_normalize(bad)


def test_percentile_of_the_norm_scheme():
    assert abs(T.norm_percentile(1) - 84.1344746068543) < 1e-12 and abs(T.norm_percentile(3) - 99.86501019683699) < 1e-12
    rng = np.random.default_rng(0)
    for n in (1, 2, 3, 10, 1001):
        v = np.sort(rng.standard_normal(n))
        for q in (0.0, 100.0, 50.0, T.norm_percentile(2), 100 - T.norm_percentile(3)):
            lo, hi, g = T.percentile_targets(q, n)
            assert 0 <= lo <= hi <= n - 1 and hi - lo <= 1
            assert T.lerp(v[lo], v[hi], g) == np.percentile(v, q)


def test_order_statistics_plan():
    p3, p2 = T.norm_percentile(3), T.norm_percentile(2)
    assert T.plan_order_stats([('std', 1)]) == []
    assert T.plan_order_stats([('global', None)]) == ['min', 'max']
    assert T.plan_order_stats([('norm', 3), ('std', 1), ('norm', 3), ('norm', 2), ('global', None)]) == \
        ['min', 'max', ('q', 100 - p3), ('q', p3), ('q', 100 - p2), ('q', p2)]


@pytest.mark.parametrize('store', ['rect', 'ragged'])
@pytest.mark.parametrize('tag', ['all', 'idxs'])
def test_stage_composition_against_the_reference(store, tag):
    """the one-sweep algebra: every stage's norm_meta from the RAW statistics (numpy's, in f64) within 1 f32 ulp of what the reference fitted
    stage by stage on the transformed array"""
    z = NC.fixture()
    idxs = None if tag == 'all' else z['idxs']
    leads = NC.lead_samples(z[store], z['offsets'] if store == 'ragged' else None, idxs)
    for k, scheme in enumerate(z['schemes']):
        stages = T.parse_normalize(scheme)
        raw = NC.numpy_raw(leads, T.plan_order_stats(stages))
        st, mean, std = T.compose_stages(stages, raw)
        NC.check_metas(st, z[f'{store}_{tag}_{k}_meta'], (store, tag, scheme))
        assert mean.dtype == np.float32 and std.dtype == np.float32 and (std > 0).all()
        if scheme == 'none':
            assert (mean == 0).all() and (std == 1).all()


def test_composite_affine_is_the_chain():
    z = NC.fixture()
    stages = T.parse_normalize(z['schemes'][5])
    raw = NC.numpy_raw(NC.lead_samples(z['rect']), T.plan_order_stats(stages))
    st, mean, std = T.compose_stages(stages, raw)
    x = z['rect'][:2].astype(np.float64)
    got = (x - mean.astype(np.float64)[None, :, None]) / std.astype(np.float64)[None, :, None]
    ok = ~np.isnan(z['rect_out'])
    assert np.abs(got - z['rect_out'])[ok].max() < 1e-5
    fit = T.DynamicNormalizeFit(st, mean, std, raw)
    xf = fit.to_transform(20, timeout=True, per_record=True)
    assert isinstance(xf, E.FusedInputTransform) and xf.k == 20 and xf.timeout and xf.per_record
    assert torch.equal(xf.mean, torch.from_numpy(mean)) and torch.equal(xf.inv_std, 1.0 / torch.from_numpy(std))


def _raw(**kw):
    d = dict(count=np.full(12, 10), nan_count=np.zeros(12, np.int64), mean=np.zeros(12), std=np.ones(12))
    d.update(kw)
    return T.RawStats(**d)


def test_no_finite_spread_names_the_lead():
    std = np.ones(12); std[7] = 0.0
    with pytest.raises(ValueError, match='lead 7'):
        T.compose_stages([('std', 1)], _raw(std=std))
    lo, hi = -np.ones(12), np.ones(12); hi[3] = -1.0
    with pytest.raises(ValueError, match='lead 3'):
        T.compose_stages([('global', None)], _raw(order={'min': lo, 'max': hi}))
    p = T.norm_percentile(2)
    with pytest.raises(ValueError, match='lead 3'):
        T.compose_stages([('norm', 2)], _raw(order={('q', 100 - p): lo, ('q', p): hi}))
    m = np.zeros(12); m[11] = np.nan
    with pytest.raises(ValueError, match='lead 11'):
        T.compose_stages([('std', 1)], _raw(mean=m))
    hi2 = np.ones(12); hi2[0] = np.inf
    with pytest.raises(ValueError, match='lead 0'):
        T.compose_stages([('global', None)], _raw(order={'min': lo, 'max': hi2}))
    # a later stage is judged after the earlier ones: fine under 'global', constant under the 'std' that follows
    with pytest.raises(ValueError, match='lead 7'):
        T.compose_stages([('global', None), ('std', 1)], _raw(std=std, order={'min': -np.ones(12), 'max': np.ones(12)}))


def test_record_table_refusals():
    x = np.zeros((4, 12, 30), np.float32)
    rag, off = np.zeros((12, 50), np.float32), np.array([0, 20, 50])
    for kw in (dict(records=np.zeros((4, 12), np.float32)), dict(records=np.zeros(7, np.float32)), dict(records=x, offsets=off),
               dict(records=np.zeros((4, 8, 30), np.float32)), dict(records=rag, offsets=np.array([0, 20, 49])), dict(records=rag, offsets=np.array([0, 20, 20, 50])),
               dict(records=rag, offsets=np.array([1, 20, 50])), dict(records=x, idxs=np.array([0, 4])), dict(records=x, idxs=np.array([-1])),
               dict(records=x, idxs=np.array([], np.int64)), dict(records=x, idxs=np.array([True, False, True, True])), dict(records=x, idxs=np.array([0.0, 1.0])),
               dict(records=rag, offsets=off, idxs=np.array([2]))):
        with pytest.raises(ValueError):
            T.fit_dynamic_normalize(normalize='std', **kw)


def test_more_than_sixteen_ranks_are_refused():
    many = [('norm', 1 + 0.25 * i) for i in range(5)]          # 5 distinct args: 20 ranks
    with pytest.raises(ValueError, match='16'):
        T.fit_dynamic_normalize(np.zeros((2, 12, 8), np.float32), normalize=many)
    assert len(T.plan_order_stats(T.parse_normalize(many[:4]))) == 8        # 16 ranks: accepted by the plan


def test_entry_points_declared_bound_and_exported():
    lib = ctypes.CDLL(hip.LIB_PATH)
    arity = {'ecgvit_fit_workspace': 2, 'ecgvit_fit_moments': 10, 'ecgvit_fit_histogram': 11, 'ecgvit_fit_select': 6}
    abi_header.held(arity, hip.SIGNATURES)
    for name in arity:
        assert hasattr(lib, name)
    assert lib.ecgvit_abi_version() == 6 and hip.ABI_VERSION == 6
    l = hip.lib()
    assert l.ecgvit_fit_workspace(0, 12) == 0 and l.ecgvit_fit_workspace(37, 12) == 37 * 12 * 32
    assert l.ecgvit_fit_workspace(10 ** 6, 12) == 512 * 12 * 32          # the record groups per lead are capped
    # argument checks are host logic: nothing is launched on a refusal
    assert l.ecgvit_fit_moments(None, None, 0, None, 1, 12, None, None, None, None) == 1
    assert l.ecgvit_fit_histogram(None, None, 0, None, 1, 12, None, 1, 0, None, None) == 1
    assert l.ecgvit_fit_select(None, None, 12, 1, 0, None) == 1
    assert l.ecgvit_fit_select(0x1000, 0x1000, 12, 17, 0, None) == 1 and l.ecgvit_fit_select(0x1000, 0x1000, 12, 1, 4, None) == 1
    assert l.ecgvit_fit_histogram(0x1000, 0x1000, 8, 0x1000, 1, 12, None, 1, 1, 0x1000, None) == 1      # passes 1..3 need the target table
    assert l.ecgvit_fit_histogram(0x1002, 0x1000, 8, 0x1000, 1, 12, 0x1000, 1, 1, 0x1000, None) == 1    # samples are 4-byte aligned


def test_kernels_spill_free():
    import code_objects
    assert os.path.exists(code_objects.READELF), 'llvm-readelf is needed to read the code object'
    ks = {n: k for n, k in code_objects.kernels(hip.LIB_PATH).items() if re.search(r'fit_(moments|hist|select)', n)}
    assert len(ks) == 7, sorted(ks)
    for n, k in ks.items():
        assert k['vgpr_spill_count'] == 0 and k['sgpr_spill_count'] == 0 and k['private_segment_fixed_size'] == 0, (n, k)
        assert k['group_segment_fixed_size'] <= 32 * 1024, (n, k)
