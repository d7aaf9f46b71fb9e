"""GPU: the robust LOESS baseline (csrc/denoise.hip, `ecgvit_rloess`) through `rloess` against the numpy f64 restatement `loess_ref.loess_fast`
(parity with the reference's `loess` package is unpinned: include/ecgvit_hip.h).  Every restated element is held to
|device - restatement| <= 2^-24 |restatement| + 1e-8 max |lead| (the f32 store's rounding plus f64 slack: 500 x the two restatements' own
disagreement, a sixth of an f32 ulp at full scale) and the robust iteration counts are equal at every sample: tests/test_loess.py shows that the
restatement takes every outlier decision at these inputs at least 1e-8 from the cut (tests/loess_gpu_cases.py: the inputs and their edges).

Measured on the MI355X, over all 24 cases (480 528 restated elements, baseline and subtract): 0 elements differ from the restatement rounded to
f32 -- the excess over the store's own rounding is 0 against the 1e-8 allowed -- and every iteration count is equal; with the f32 rounding
included the largest |device - restatement| / max |lead| is 4.7e-8 (baseline) and 6.5e-8 (subtract).
"""
import numpy as np
import pytest
import torch

import ecg_representation_learning_amd as E
import loess_ref as R
from loess_gpu_cases import CASES, case_store, case_input

pytestmark = pytest.mark.gpu
_REF = {}


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x, np.float32)).cuda()


def restated(name):
    """{(record, lead): (samples, fit, iters)} of a case, computed once"""
    if name not in _REF:
        c = CASES[name]
        _REF[name] = {key: (y,) + R.loess_fast(y.astype(np.float64), m, c['degree'], c['robust_iters'])[:2] for key, y, m in case_input(c)}
    return _REF[name]


def run(c, store, off, **kw):
    if len(c['lengths']) == 1:
        return E.rloess(dev(store[None]), c['npoints'], c['degree'], c['robust_iters'], **kw)
    return E.rloess(dev(store), c['npoints'], c['degree'], c['robust_iters'], offsets=off, **kw)


@pytest.mark.parametrize('name', list(CASES))
def test_parity_with_the_restatement(name):
    c = CASES[name]
    store, off = case_store(c)
    base, iters = run(c, store, off, return_iters=True)
    sub = run(c, store, off, subtract=True)
    ragged = len(c['lengths']) > 1
    base, iters, sub = base.cpu().numpy(), iters.cpu().numpy(), sub.cpu().numpy()
    assert iters.dtype == np.int8 and iters.shape == (len(c['lengths']), 12, max(c['lengths']))
    worst = worst_sub = 0.0
    differ = total = 0
    for (i, lead), (y, fit, it) in restated(name).items():
        n = len(y)
        got = (base[lead, off[i]:off[i + 1]] if ragged else base[0, lead]).astype(np.float64)
        got_sub = (sub[lead, off[i]:off[i + 1]] if ragged else sub[0, lead]).astype(np.float64)
        amax = float(np.abs(y).max())
        slack = 1e-8 * amax
        diff = y.astype(np.float64) - fit
        worst = max(worst, float(np.abs(got - fit).max()) / amax)
        worst_sub = max(worst_sub, float(np.abs(got_sub - diff).max()) / amax)
        differ += int((got.astype(np.float32) != fit.astype(np.float32)).sum() + (got_sub.astype(np.float32) != diff.astype(np.float32)).sum())
        total += 2 * n
        assert np.all(np.abs(got - fit) <= 2.0 ** -24 * np.abs(fit) + slack), (name, i, lead, np.abs(got - fit).max())
        assert np.all(np.abs(got_sub - diff) <= 2.0 ** -24 * np.abs(diff) + slack), (name, i, lead, np.abs(got_sub - diff).max())
        assert np.array_equal(iters[i, lead, :n], it) and not iters[i, lead, n:].any(), (name, i, lead, np.flatnonzero(iters[i, lead, :n] != it)[:8])
    print(f'{name}: max |device - restatement| / max |lead| = {worst:.2e} (baseline), {worst_sub:.2e} (subtract), the f32 rounding included; '
          f'{differ} of {total} elements differ from the restatement rounded to f32')


# ---- layouts --------------------------------------------------------------------------------------------
L = 161
RAGGED_LENGTHS = [37, L, 64, L, L, 23]       # offsets 37, 198, 262, 423, 584: odd 4-byte addresses
SHARED = [1, 3, 4]                           # where the rectangle's three records sit in the ragged store


@pytest.fixture(scope='module')
def stores():
    recs = [R.signal(50 + i, l) for i, l in enumerate(RAGGED_LENGTHS)]
    rect = np.stack([recs[i] for i in SHARED])
    off = np.concatenate([[0], np.cumsum(RAGGED_LENGTHS)])
    return rect, np.concatenate(recs, axis=1), off


def guarded(shape):
    """-> (flat buffer filled with a pattern, the view of `shape` in its middle)"""
    n = int(np.prod(shape))
    flat = torch.full((n + 512,), -7.25, device='cuda')
    return flat, flat[256:256 + n].view(shape)


@pytest.mark.parametrize('subtract', [False, True])
def test_layouts_give_the_same_bits(stores, subtract):
    rect_h, rag_h, off = stores

    def fn(x, **kw):
        return E.rloess(x, 31, subtract=subtract, **kw)
    rect, rag = dev(rect_h), dev(rag_h)
    base, it_base = E.rloess(rect, 31, subtract=subtract, return_iters=True)
    base, it_base = base.cpu().numpy(), it_base.cpu().numpy()
    assert not np.array_equal(base, rect_h) and np.array_equal(rect.cpu().numpy(), rect_h)     # the input is not modified
    for i in range(3):                                                                         # each record alone
        assert np.array_equal(fn(rect[i:i + 1].contiguous())[0].cpu().numpy(), base[i])
    inpl = rect.clone()                                                                        # in place equals out=
    assert fn(inpl, out=inpl) is inpl and np.array_equal(inpl.cpu().numpy(), base)
    # a subset of the rectangle into a guarded out: the other record and the guard band keep their bits; iters rows come in idxs order
    flat, out = guarded(rect.shape)
    _, it_sub = E.rloess(rect, 31, subtract=subtract, idxs=[2, 0], out=out, return_iters=True)
    o = out.cpu().numpy()
    assert np.array_equal(o[2], base[2]) and np.array_equal(o[0], base[0]) and (o[1] == -7.25).all()
    assert (flat[:256] == -7.25).all() and (flat[-256:] == -7.25).all() and np.array_equal(it_sub.cpu().numpy(), it_base[[2, 0]])
    # the ragged store: every record, then a subset in place (the records between the selected ones are its gaps; samples past raw_len are theirs)
    r_all, it_all = E.rloess(rag, 31, subtract=subtract, offsets=off, return_iters=True)
    r_all, it_all = r_all.cpu().numpy(), it_all.cpu().numpy()
    for j, i in enumerate(SHARED):
        assert np.array_equal(r_all[:, off[i]:off[i + 1]], base[j]) and np.array_equal(it_all[i], it_base[j]), i
    assert not it_all[0, :, 37:].any() and not it_all[5, :, 23:].any()
    flat, out = guarded(rag.shape)
    fn(rag, offsets=off, idxs=[4, 1], out=out)
    o = out.cpu().numpy()
    assert np.array_equal(o[:, off[4]:off[5]], base[2]) and np.array_equal(o[:, off[1]:off[2]], base[0])
    mask = np.ones(rag.shape[1], bool)
    mask[off[4]:off[5]] = mask[off[1]:off[2]] = False
    assert (o[:, mask] == -7.25).all() and (flat[:256] == -7.25).all() and (flat[-256:] == -7.25).all()
    inpl = rag.clone()
    fn(inpl, offsets=off, idxs=[4, 1], out=inpl)
    o = inpl.cpu().numpy()
    assert np.array_equal(o[:, off[4]:off[5]], base[2]) and np.array_equal(o[:, mask], rag_h[:, mask])
    # a host store streams through in chunks and gives the same bits
    h, it_h = E.rloess(rect_h, 31, subtract=subtract, chunk_records=1, return_iters=True)
    assert isinstance(h, np.ndarray) and h.dtype == np.float32 and np.array_equal(h, base) and np.array_equal(it_h, it_base)
    h = fn(rag_h, offsets=off, idxs=[4, 1], chunk_records=1)
    assert np.array_equal(h[:, off[4]:off[5]], base[2]) and np.array_equal(h[:, mask], rag_h[:, mask])
    # beside a long record (another LDS size, another slot count under the fraction form) the record keeps its bits
    long_h = np.concatenate([rect_h[0], R.signal(99, 8300)], axis=1)
    got = fn(dev(long_h), offsets=[0, L, L + 8300])
    assert np.array_equal(got[:, :L].cpu().numpy(), base[0]) and torch.isfinite(got).all()
    f = 32.5 / L                                                   # 31 points for 161 samples, 323 for the 1603 beside it
    assert R.frac_points(L, f) == 31 and R.frac_points(1603, f) == 323
    long_h = np.concatenate([rect_h[0], R.signal(98, 1603)], axis=1)
    got = E.rloess(dev(long_h), f, subtract=subtract, offsets=[0, L, L + 1603])
    assert np.array_equal(got[:, :L].cpu().numpy(), base[0]) and torch.isfinite(got).all()


def test_subtract_is_the_f64_difference_rounded_once(stores):
    rect = dev(stores[0])
    base, sub = E.rloess(rect, 31).double(), E.rloess(rect, 31, subtract=True).double()
    x = rect.double()
    # the baseline tensor is the f64 fit rounded to f32: x - fit lies within half an ulp of the fit around x - baseline, and one rounding more
    assert torch.all((sub - (x - base)).abs() <= 2.0 ** -24 * (base.abs() + (x - base).abs()) * (1 + 2.0 ** -20))
    assert not torch.equal(sub, x)


def test_zero_and_constant_leads():
    x = R.signal(77, 300)
    x[3] = 0.0
    x[7] = 0.625
    x[8] = -1234.5678
    got, iters = E.rloess(dev(x[None]), 64, return_iters=True)
    got, iters = got[0].cpu().numpy(), iters[0].cpu().numpy()
    assert not got[3].any() and not iters[3].any()                       # mad == 0: the distance-weighted fit stands, no robust iteration ran
    for c in (7, 8):
        ulp = np.spacing(np.abs(x[c, 0]))
        assert np.all(np.abs(got[c].astype(np.float64) - np.float64(x[c, 0])) <= 2 * ulp), c
    assert iters[0].min() >= 2 and np.isfinite(got).all()
    sub = E.rloess(dev(x[None]), 64, subtract=True)[0].cpu().numpy()
    assert not sub[3].any() and np.all(np.abs(sub[7]) <= 2 * np.spacing(np.float32(0.625)))


def test_out_aliasing_rules(stores):
    rect = dev(stores[0])
    flat = torch.zeros(rect.numel() + 8, device='cuda')
    a, b = flat[:rect.numel()].view(rect.shape), flat[8:].view(rect.shape)
    with pytest.raises(ValueError, match='overlaps'):
        E.rloess(a, 31, out=b)
    with pytest.raises(ValueError, match='out'):
        E.rloess(rect, 31, out=torch.zeros(3, 12, L - 1, device='cuda'))
    with pytest.raises(ValueError, match='repeats'):
        E.rloess(rect, 31, idxs=[1, 1])
    with pytest.raises(ValueError, match='window of 3'):
        E.rloess(rect, 0.03)


def test_denoiser_with_the_loess_baseline(stores):
    rect_h, rag_h, off = stores
    rect, rag = dev(rect_h), dev(rag_h)
    d = E.EcgDenoiser()
    lp = E.lowpass(rect)
    want = E.nlm(E.rloess(lp, 500, subtract=True))
    got = d(rect, baseline='rloess')
    assert torch.equal(got, want) and not torch.equal(got, d(rect)) and np.array_equal(rect.cpu().numpy(), rect_h)
    # the subtracting sweep is the baseline sweep: lowpass - rloess(lowpass) in f32 differs from it by the extra rounding alone
    two = lp - E.rloess(lp, 500)
    one = E.rloess(lp, 500, subtract=True)
    assert torch.all((one - two).abs() <= 2.0 ** -23 * (lp.abs() + two.abs()))
    d31 = E.EcgDenoiser(fqs=250, loess_points=31, search_width=40, patch_width=5)
    sub = d31(rag, baseline='rloess', offsets=off, idxs=[1, 4])
    lp = E.lowpass(rag, fqs=250, offsets=off, idxs=[1, 4])
    want = E.nlm(E.rloess(lp, 31, subtract=True, offsets=off, idxs=[1, 4]), search_width=40, patch_width=5, offsets=off, idxs=[1, 4])
    assert torch.equal(sub, want) and torch.equal(sub[:, :off[1]], rag[:, :off[1]])
    h = d31(rag_h, baseline='rloess', offsets=off, idxs=[1, 4], chunk_records=1)                 # a host store streams through every stage
    assert isinstance(h, np.ndarray) and np.array_equal(h, sub.cpu().numpy())
