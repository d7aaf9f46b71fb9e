"""GPU: `fit_dynamic_normalize` and the C-ABI of csrc/fit_stats.hip (moments, radix select) on the smallest inputs at which they can go wrong.
Order statistics, counts and NaN counts are compared BIT FOR BIT with np.sort on the non-NaN samples (ties between -0.0 and +0.0 in key order,
-0.0 first); every stage's norm_meta with the reference's own fit in tests/golden/dynamic_normalize.npz within 1 f32 ulp (both sides are
f64-accurate before the cast to f32, so the casts can differ by one rounding).
"""
import numpy as np
import pytest
import torch

import ecg_representation_learning_amd as E
from ecg_representation_learning_amd import hip, transform as T
from ecg_representation_learning_amd.hip import lib, check, ptr, stream
import normalize_cases as NC

pytestmark = pytest.mark.gpu
P3 = T.norm_percentile(3)
SPECS = ['min', 'max', ('q', 100 - P3), ('q', P3), ('q', 50.0), ('q', T.norm_percentile(1)), ('q', 100 - T.norm_percentile(1)), ('q', 12.5)]   # 14 ranks


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def check_raw(raw, leads, specs=SPECS, want_std=True):
    """a RawStats of the device against numpy on the same samples"""
    want = NC.numpy_raw(leads, specs, want_std)
    assert raw.count.tolist() == want.count.tolist() and raw.nan_count.tolist() == want.nan_count.tolist()
    for c, v in enumerate(leads):
        s = NC.sorted_valid(v)
        got, ref = raw.values[c], s[raw.ranks[c]]
        assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), ref.view(np.uint32)), (c, raw.ranks[c], got, ref)
    for spec in specs:
        assert np.array_equal(raw.order[spec], want.order[spec]), spec            # the same f64 interpolation of the same two samples
    np.testing.assert_allclose(raw.mean, want.mean, rtol=1e-12, atol=1e-300)
    if want_std:
        np.testing.assert_allclose(raw.std, want.std, rtol=1e-11, atol=1e-300)


def fit_raw(x, offsets=None, idxs=None, specs=SPECS, **kw):
    return T.device_raw_stats(x, specs, True, offsets=offsets, idxs=idxs, **kw)


# ------------------------------------------------------------------------------------------------ the fixture
@pytest.mark.parametrize('store', ['rect', 'ragged'])
@pytest.mark.parametrize('tag', ['all', 'idxs'])
def test_fixture_every_scheme(store, tag):
    z = NC.fixture()
    idxs = None if tag == 'all' else z['idxs']
    off = z['offsets'] if store == 'ragged' else None
    leads = NC.lead_samples(z[store], off, idxs)
    x = dev(z[store])
    for k, scheme in enumerate(z['schemes']):
        fit = E.fit_dynamic_normalize(x, scheme, offsets=off, idxs=idxs)
        NC.check_metas(fit.stages, z[f'{store}_{tag}_{k}_meta'], (store, tag, scheme))
        stages = T.parse_normalize(scheme)
        specs = T.plan_order_stats(stages)
        want = NC.numpy_raw(leads, specs)
        assert fit.count.tolist() == want.count.tolist() and fit.nan_count.tolist() == want.nan_count.tolist()
        if specs:
            for c, v in enumerate(leads):
                assert np.array_equal(fit.raw.values[c].view(np.uint32), NC.sorted_valid(v)[fit.raw.ranks[c]].view(np.uint32))
        if scheme == 'global':          # minimum and maximum ARE the metas: bit for bit
            assert np.array_equal(fit.stages[0].norm_meta[0], np.array([np.nanmin(v) for v in leads], np.float32))
            assert np.array_equal(fit.stages[0].norm_meta[1], np.array([np.nanmax(v) for v in leads], np.float32))
    check_raw(fit_raw(x, off, idxs), leads)


def test_chunked_host_input_equals_the_device_fit():
    z = NC.fixture()
    for store, off in (('rect', None), ('ragged', z['offsets'])):
        for idxs in (None, z['idxs'][::-1].copy()):
            one = fit_raw(dev(z[store]), off, idxs)
            for host, chunk in ((z[store], 1), (z[store].astype(np.float64), 3), (torch.from_numpy(z[store]), None)):
                got = fit_raw(host, off, idxs, chunk_records=chunk)
                assert np.array_equal(got.values.view(np.uint32), one.values.view(np.uint32)) and np.array_equal(got.ranks, one.ranks)
                assert got.count.tolist() == one.count.tolist() and got.nan_count.tolist() == one.nan_count.tolist()
                # the chunk order changes the f64 summation order: 1 f32 ulp
                assert NC.ulps(got.mean.astype(np.float32), one.mean.astype(np.float32)).max() <= 1
                assert NC.ulps(got.std.astype(np.float32), one.std.astype(np.float32)).max() <= 1
        a = E.fit_dynamic_normalize(dev(z[store]), offsets=off)
        b = E.fit_dynamic_normalize(z[store], offsets=off, chunk_records=2)
        assert NC.ulps(a.mean, b.mean).max() <= 1 and NC.ulps(a.std, b.std).max() <= 1


def test_two_identical_calls_give_identical_bits():
    rng = np.random.default_rng(5)
    x = dev(rng.standard_normal((37, 12, 1000)).astype(np.float32))
    a, b = fit_raw(x), fit_raw(x)
    assert np.array_equal(a.mean.view(np.uint64), b.mean.view(np.uint64)) and np.array_equal(a.std.view(np.uint64), b.std.view(np.uint64))
    assert np.array_equal(a.values.view(np.uint32), b.values.view(np.uint32)) and a.count.tolist() == b.count.tolist()
    f, g = E.fit_dynamic_normalize(x), E.fit_dynamic_normalize(x)
    assert np.array_equal(f.mean.view(np.uint32), g.mean.view(np.uint32)) and np.array_equal(f.std.view(np.uint32), g.std.view(np.uint32))


# ------------------------------------------------------------------------------------------------ edge cases of the select
def test_one_and_two_valid_samples():
    x = np.full((2, 12, 65), np.nan, np.float32)
    for c in range(12):
        x[c % 2, c, 7 * c % 65] = 0.5 - c                 # one valid sample
        if c >= 6:
            x[1 - c % 2, c, 64 - c] = 3.25 * c            # two: pure interpolation
    leads = NC.lead_samples(x)
    raw = fit_raw(dev(x))
    check_raw(raw, leads)
    assert raw.count.tolist() == [1] * 6 + [2] * 6 and raw.nan_count.tolist() == [129] * 6 + [128] * 6
    for spec in SPECS[2:]:
        assert np.array_equal(raw.order[spec], np.array([np.nanpercentile(v.astype(np.float64), spec[1]) for v in leads]))


def test_ties_shared_last_digits_signed_zeros_and_denormals():
    rng = np.random.default_rng(11)
    n = 4096
    x = np.empty((1, 12, n), np.float32)
    for c in range(12):
        if c < 3:        # 1000 copies of one value straddling both neighbour ranks of the median (and of the 12.5th percentile on lead 2)
            v = np.concatenate([rng.standard_normal(n - 1000).astype(np.float32), np.full(1000, [0.25, -0.125, -1.5][c], np.float32)])
        elif c < 6:      # every digit but the last shared: 1 + k 2^-23
            v = (1.0 + np.arange(n) * 2.0 ** -23).astype(np.float32) * (1 if c < 5 else -1)
        elif c < 9:      # mixed signs, both zeros, denormals, infinities, the largest finite values
            v = rng.standard_normal(n).astype(np.float32)
            v[:600] = 0.0
            v[600:1100] = -0.0
            v[1100:1400] = (rng.integers(1, 1 << 23, 300).astype(np.uint32) | (rng.integers(0, 2, 300).astype(np.uint32) << 31)).view(np.float32)   # denormals
            v[1400:1410] = np.inf
            v[1410:1420] = -np.inf
            v[1420:1424] = [np.finfo(np.float32).max, -np.finfo(np.float32).max, np.finfo(np.float32).tiny, -np.finfo(np.float32).tiny]
            v[1424:1500] = np.nan
        else:            # zeros only, of both signs
            v = np.where(rng.random(n) < 0.5, 0.0, -0.0).astype(np.float32)
        x[0, c] = rng.permutation(v)
    leads = NC.lead_samples(x)
    with np.errstate(invalid='ignore', over='ignore'):
        want = NC.numpy_raw(leads, SPECS)
    raw = fit_raw(dev(x))
    assert raw.count.tolist() == want.count.tolist() and raw.nan_count.tolist() == want.nan_count.tolist()
    for c, v in enumerate(leads):
        got, ref = raw.values[c], NC.sorted_valid(v)[raw.ranks[c]]
        assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), (c, got, ref)
    lo, hi, _ = T.percentile_targets(50.0, n)
    assert raw.values[0][6] == raw.values[0][7] == np.float32(0.25)       # SPECS[4] = the median: entries 6, 7 of the table, both inside the tie
    for c in (0, 1, 2, 3, 4, 5):                                          # finite leads: moments too
        np.testing.assert_allclose(raw.mean[c], want.mean[c], rtol=1e-12)
        np.testing.assert_allclose(raw.std[c], want.std[c], rtol=1e-11)


def test_short_records_at_odd_offsets():
    rng = np.random.default_rng(3)
    lens = [1, 3, 130, 257]
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)          # 0, 1, 4, 134, 391: S_total odd, so every lead starts elsewhere mod 16 B
    x = rng.standard_normal((12, int(off[-1]))).astype(np.float32)
    x[5, 2] = np.nan
    xd = dev(x)
    check_raw(fit_raw(xd, off), NC.lead_samples(x, off))
    check_raw(fit_raw(xd, off, np.array([3, 1])), NC.lead_samples(x, off, [3, 1]))
    check_raw(fit_raw(x, off, chunk_records=3), NC.lead_samples(x, off))
    # the C-ABI on tables of its own: records with gaps between them inside a larger buffer, zero-length entries skipped
    buf = rng.standard_normal(12 * 1001 + 64).astype(np.float32)
    so, rl = np.array([3, 17, 40, 301, 999], np.int64), np.array([1, 3, 130, 257, 0], np.int32)
    bd, sod, rld = dev(buf), dev(so), dev(rl)
    ws = torch.empty(lib().ecgvit_fit_workspace(5, 12) // 8, dtype=torch.float64, device='cuda')
    state = torch.zeros(12, 4, dtype=torch.int64, device='cuda')
    hist = torch.zeros(4, 12, 16, 256, dtype=torch.int64, device='cuda')
    leads = [np.concatenate([buf[c * 1001 + o:c * 1001 + o + l] for o, l in zip(so, rl)]) for c in range(12)]
    ranks = np.array([0, 1, 195, 389, 390, 200], np.int64)
    sel = np.zeros((12, 16, 4), np.int64)
    sel[:, :6, 0] = ranks
    seld = dev(sel)
    for _ in range(2):          # the state accumulates: two launches count everything twice
        check(lib().ecgvit_fit_moments(ptr(bd), ptr(sod), 1001, ptr(rld), 5, 12, None, ptr(ws), ptr(state), stream()), 'fit_moments')
    for p in range(4):
        check(lib().ecgvit_fit_histogram(ptr(bd), ptr(sod), 1001, ptr(rld), 5, 12, ptr(seld), 6, p, ptr(hist[p]), stream()), 'fit_histogram')
        check(lib().ecgvit_fit_select(ptr(hist[p]), ptr(seld), 12, 6, p, stream()), 'fit_select')
    st = state.cpu().numpy()
    assert st[:, 0].tolist() == [2 * 391] * 12 and st[:, 1].tolist() == [0] * 12
    np.testing.assert_allclose(st[:, 2].copy().view(np.float64), [2 * v.astype(np.float64).sum() for v in leads], rtol=1e-12)
    assert hist[0].sum(dim=(1, 2)).tolist() == [391] * 12 and int(hist[0, :, 1:].sum()) == 0
    out = seld.cpu().numpy()
    got = T._key_to_f32(out[:, :6, 1].astype(np.uint64).astype(np.uint32))
    for c in range(12):
        assert np.array_equal(got[c].view(np.uint32), NC.sorted_valid(leads[c])[ranks].view(np.uint32))
    assert (out[:, :6, 3] >= 1).all() and (out[:, :6, 0] < out[:, :6, 3]).all()


def test_several_workgroups_per_lead_and_a_clustered_lead():
    rng = np.random.default_rng(9)
    x = (rng.standard_normal((37, 12, 1000)) * np.linspace(0.1, 3, 12)[None, :, None]).astype(np.float32)
    x[:, 4][rng.random((37, 1000)) < 0.9] = 0.0           # 90 % exact zeros: most percentiles ARE the zero
    x[:, 5][rng.random((37, 1000)) < 0.3] = 0.0
    x[3:9, 6, 100:900] = np.nan
    x[36, :, 990:] = 0.0                                  # a zero-padded tail
    xd = dev(x)
    check_raw(fit_raw(xd), NC.lead_samples(x))
    ids = np.array([36, 0, 17, 5, 22])
    check_raw(fit_raw(xd, idxs=ids), NC.lead_samples(x, idxs=ids))
    fit = E.fit_dynamic_normalize(xd, [('norm', 3), ('std', 1)], idxs=ids)
    assert fit.count.tolist() == [len(ids) * 1000 - (800 if c == 6 else 0) for c in range(12)]


def test_refusals_on_the_device():
    x = np.random.default_rng(2).standard_normal((3, 12, 50)).astype(np.float32)
    x[:, 9] = np.nan
    with pytest.raises(ValueError, match='lead 9'):
        E.fit_dynamic_normalize(dev(x), 'std')
    x[:, 9] = 1.5
    for scheme in ('std', 'global', 'norm', [('none',), ('norm', 3)]):
        with pytest.raises(ValueError, match='lead 9'):
            E.fit_dynamic_normalize(dev(x), scheme)
    assert E.fit_dynamic_normalize(dev(x), 'none').std.tolist() == [1.0] * 12
    with pytest.raises(ValueError, match='float32'):
        E.fit_dynamic_normalize(dev(x).double(), 'std')
    with pytest.raises(ValueError, match='contiguous'):
        E.fit_dynamic_normalize(dev(x).transpose(0, 2).contiguous().transpose(0, 2), 'std')


# ------------------------------------------------------------------------------------------------ the transform the fit hands on
def test_forward_through_the_fitted_transform():
    """`fit.to_transform()` in the patch-load kernel on the two fixture records against the reference's transformed output: its error against
    the f64 evaluation of the reference chain (the fixture's `*_out`) is at most twice the error of the reference's chain evaluated in f32
    (stage by stage with the fixture's f32 norm_meta) against the same -- the factor two covers one affine instead of two.  Both errors are
    computed here from the fixture."""
    z = NC.fixture()
    P = 20
    for store in ('rect', 'ragged'):
        off = z['offsets'] if store == 'ragged' else None
        fit = E.fit_dynamic_normalize(dev(z[store]), offsets=off)
        meta, want = z[f'{store}_all_5_meta'], z[f'{store}_out']
        if store == 'rect':
            recs = [z['rect'][0], z['rect'][1]]
        else:
            recs = [z['ragged'][:, off[i]:off[i + 1]] for i in (0, 1)]
        err_ref = err = 0.0
        xf = fit.to_transform(P)
        mean, inv = xf.device_stats(torch.device('cuda'))
        for i, r in enumerate(recs):
            L = r.shape[1]
            y = r.astype(np.float32)[None]
            for j in range(2):      # the reference's __call__ (transform.py:88-100) in f32
                sub, div = (meta[j, 0], meta[j, 1] - meta[j, 0]) if j == 0 else (meta[j, 0], meta[j, 1])
                y = (y - sub[None, :, None]) / div[None, :, None]
            assert y.dtype == np.float32
            n = xf.padded_length(L) // P
            x = dev(np.nan_to_num(r.astype(np.float32))[None])      # (NaN samples: compared nowhere)
            patches = torch.empty(n, 12 * P, device='cuda')
            check(lib().ecgvit_patch_gather_transform(ptr(x), ptr(patches), 1, 12, L, n * P, P, 12 * P, ptr(mean), ptr(inv), None, None, hip.F32, stream()),
                  'patch_gather_transform')
            got = patches.view(n, P, 12).permute(2, 0, 1).reshape(12, n * P)[:, :L].cpu().numpy()
            ok = ~np.isnan(want[i][:, :L])
            assert ok.sum() > 0.9 * ok.size
            err_ref = max(err_ref, float(np.abs(y[0].astype(np.float64) - want[i][:, :L])[ok].max()))
            err = max(err, float(np.abs(got.astype(np.float64) - want[i][:, :L])[ok].max()))
        print(f'normalize fit forward {store}: max |fitted transform - f64 chain| = {err:.2e}; reference f32 chain {err_ref:.2e}')
        assert err <= 2 * err_ref, (store, err, err_ref)
