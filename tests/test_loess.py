"""CPU: the two numpy restatements of the robust LOESS baseline against each other (tests/loess_ref.py: `loess_literal`, the algorithm line by
line in the `loess` package's form; `loess_fast`, the kernel's operations in the kernel's order), the margin of every outlier decision at the GPU
tests' inputs, the ABI of `ecgvit_rloess` with every refusal of its launcher (no GPU is touched: a refused call launches nothing) and the host
contract of `rloess` and `EcgDenoiser(baseline=...)`.

A window with exactly degree + 1 samples of positive distance weight (degree 2 at n = 4, n = 5 and npoints = 4) is interpolated: its residuals,
and so its median, are the rounding of the solver, 0 in one restatement and 1e-17 in the other.  The seeds below are such that no window's median
is exactly 0 in either, which is what equal iteration counts need there (the decisions themselves are far from the cut: the three interpolated
samples keep bw >= 0.79, the fourth has bw = 0)."""
import ctypes

import numpy as np
import pytest
import torch

import abi_header
import ecg_representation_learning_amd as E
from ecg_representation_learning_amd import hip, denoise
import loess_ref as R
from loess_gpu_cases import CASES, case_input

SHAPES = [(4, 31), (5, 4), (40, 31), (300, 31), (300, 32), (300, 65), (600, 501)]
SEED = {(4, 31): 1, (5, 4): 3}


@pytest.mark.parametrize('degree', [1, 2])
@pytest.mark.parametrize('n,npoints', SHAPES)
def test_literal_against_fast(n, npoints, degree):
    y = R.signal(SEED.get((n, npoints), 100 + n + npoints), n, 1)[0].astype(np.float64)
    lit, it_l, mg_l = R.loess_literal(y, npoints, degree)
    fast, it_f, mg_f = R.loess_fast(y, npoints, degree)
    tol = 1e-9 * np.abs(y).max()
    print(f'n={n} npoints={npoints} degree={degree}: max |literal - fast| {np.abs(lit - fast).max():.2e}, iters {it_l.min()}..{it_l.max()}, margin {mg_l:.2e}')
    assert np.abs(lit - fast).max() <= tol and np.array_equal(it_l, it_f)
    if npoints & 1 or npoints >= n:           # no tie: the default (unstable) sort selects the same window
        uns, it_u, _ = R.loess_literal(y, npoints, degree, kind=None)
        assert np.abs(uns - lit).max() <= tol and np.array_equal(it_u, it_l)


def test_gpu_inputs_keep_every_decision_clear_of_the_cut():
    """what lets tests/test_gpu_loess.py demand equal iteration counts without exception: at its inputs the restatement takes every decision
    bw < 0.34 at least 1e-8 from the cut, no window's median is 0, and the iteration counts cover 2 and the cap"""
    seen = set()
    for name, case in CASES.items():
        for lead, y, m in case_input(case):
            fit, iters, margin, min_mad = R.loess_fast(y.astype(np.float64), m, case['degree'], case['robust_iters'], return_mad=True)
            assert np.isfinite(fit).all()
            if case['robust_iters']:
                assert margin >= 1e-8 and min_mad > 0, (name, lead, margin, min_mad)
                seen.update(np.unique(iters).tolist())
    assert {2, 10} <= seen and min(seen) >= 1, seen


@pytest.mark.parametrize('degree', [1, 2])
def test_exact_polynomial_and_plain_loess(degree):
    t = np.arange(120, dtype=np.float64)
    y = (0.3 - 0.02 * t + (2e-4 * t * t if degree == 2 else 0.0))
    for iters in (0, 1, 10):
        for fn in (R.loess_fast, R.loess_literal):
            assert np.abs(fn(y, 31, degree, iters)[0] - y).max() <= 1e-9 * np.abs(y).max(), (iters, fn.__name__)
    # robust_iters = 0 on noisy data: a plain tricube-weighted polyfit per window
    y = R.signal(5, 120, 1)[0].astype(np.float64)
    for npoints in (31, 32):
        m, lo, d = R.windows(120, npoints)
        want = np.empty(120)
        for j in range(120):
            x = np.arange(lo[j], lo[j] + m, dtype=np.float64)
            w = (1 - (np.abs(x - j) / d[j]) ** 3) ** 3
            want[j] = np.polyval(np.polyfit(x - j, y[lo[j]:lo[j] + m], degree, w=np.sqrt(w)), 0.0)
        for fn in (R.loess_fast, R.loess_literal):
            fit, iters, _ = fn(y, npoints, degree, 0)
            assert np.abs(fit - want).max() <= 1e-9 * np.abs(y).max() and not iters.any()


def test_fraction_width():
    assert [R.force_odd(x) for x in range(6)] == [1, 1, 3, 3, 5, 5]
    for n, f in ((700, 0.5), (701, 0.25), (37, 0.3), (5000, 0.1), (64, 0.99), (9, 0.1)):
        assert R.frac_points(n, f) == denoise.frac_points(n, f) == 2 * ((int(n * f) - 1) // 2) + 1


# ---- ABI ----------------------------------------------------------------------------------------------
def test_symbol_exists_with_the_declared_arity():
    abi_header.held({'ecgvit_rloess': 16}, hip.SIGNATURES)
    assert hasattr(hip.lib(), 'ecgvit_rloess') and hip.lib().ecgvit_abi_version() == 6
    assert hip.DENOISE_MAX_POINTS == denoise.MAX_POINTS == 1024


P = 0x10000000      # never dereferenced: a refused call launches nothing
IDS = dict(ids=lambda d: ','.join(f'{k}={v}' for k, v in d.items()))


def _rloess(**kw):
    a = dict(x=P, out=P, src_off=P, lead_stride=64, raw_len=P, R=4, C=12, min_len=64, max_len=64, npoints=31, frac=0.0, degree=2, robust_iters=10,
             subtract=0, iters=None, stream=None)
    a.update(kw)
    return hip.lib().ecgvit_rloess(*a.values())


@pytest.mark.parametrize('bad', [dict(x=None), dict(x=P + 2), dict(out=None), dict(out=P + 2), dict(src_off=None), dict(src_off=P + 4), dict(raw_len=None),
                                 dict(raw_len=P + 2), dict(R=0), dict(R=-1), dict(C=0), dict(C=65536), dict(lead_stride=0), dict(lead_stride=-64),
                                 dict(max_len=0), dict(max_len=32769), dict(min_len=65), dict(min_len=3), dict(min_len=2, degree=1), dict(min_len=0),
                                 dict(degree=0), dict(degree=3), dict(robust_iters=-1), dict(robust_iters=11), dict(npoints=3), dict(npoints=2, degree=1),
                                 dict(npoints=1025), dict(npoints=0), dict(frac=-0.1), dict(frac=1.5), dict(frac=float('nan')), dict(frac=float('inf')),
                                 dict(frac=0.05), dict(frac=0.5, min_len=8), dict(frac=0.5, max_len=2100), dict(subtract=2), dict(subtract=-1)], **IDS)
def test_rloess_refusals(bad):
    assert _rloess(**bad) == 1


# ---- host contract ----------------------------------------------------------------------------------------
def test_host_contract():
    assert 'rloess' in E.__all__ and E.rloess is denoise.rloess
    x = torch.zeros(2, 12, 64)
    for bad in (dict(npoints=3), dict(npoints=2, degree=1), dict(npoints=1025), dict(npoints=0.0), dict(npoints=1.0), dict(npoints=1.5), dict(npoints=True),
                dict(npoints='500'), dict(degree=0), dict(degree=3), dict(degree=2.0), dict(robust_iters=-1), dict(robust_iters=11), dict(robust_iters=2.5)):
        with pytest.raises(ValueError, match=next(iter(bad))):
            E.rloess(x, **bad)
    with pytest.raises(ValueError, match='window of 3'):                 # the fraction form: 40 samples * 0.1 -> force_odd(3) = 3 < degree + 2
        E.rloess(np.zeros((12, 90), np.float32), npoints=0.1, degree=2, offsets=[0, 40, 90])
    with pytest.raises(ValueError, match='at most 1024'):
        E.rloess(np.zeros((1, 12, 4100), np.float32), npoints=0.5)
    with pytest.raises(ValueError, match='at least 4'):                  # a record shorter than degree + 2
        E.rloess(np.zeros((1, 12, 3), np.float32))
    with pytest.raises(ValueError, match='at least 3'):
        E.rloess(np.zeros((12, 30), np.float32), degree=1, offsets=[0, 2, 30])
    with pytest.raises(ValueError, match='repeats'):
        E.rloess(x, idxs=[1, 1])
    with pytest.raises(ValueError, match='32768'):
        E.rloess(np.zeros((1, 12, 32769), np.float32))
    with pytest.raises(ValueError, match='12 leads'):
        E.rloess(np.zeros((2, 3, 64), np.float32))
    with pytest.raises(ValueError, match='offsets'):
        E.rloess(np.zeros((12, 64), np.float32))
    with pytest.raises(ValueError, match='idxs'):
        E.rloess(x, idxs=[2])
    with pytest.raises(ValueError, match='float'):
        E.rloess(np.zeros((2, 12, 64), np.int16))
    for out in (np.zeros((2, 12, 64)), np.zeros((2, 12, 63), np.float32), torch.zeros(2, 12, 64)):
        with pytest.raises(ValueError, match='out'):
            E.rloess(x, out=out)
    with pytest.raises(ValueError, match='chunk_records'):
        E.rloess(x, chunk_records=0)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match='no CPU fallback'):
            E.rloess(x)


def test_denoiser_baseline_contract(monkeypatch):
    d = E.EcgDenoiser()
    assert d.loess_points == 500 and E.EcgDenoiser(fqs=250).loess_points == 250 and E.EcgDenoiser(fqs=250, loess_points=125).loess_points == 125
    assert 'loess_points=500' in repr(d)
    for bad in (3, 1025, 2.5, True, '500'):
        with pytest.raises(ValueError, match='loess_points'):
            E.EcgDenoiser(loess_points=bad)
    # the default window, int(fqs), is checked only where the LOESS is asked for: a rate above 1024 Hz still builds and runs the other paths
    fast = E.EcgDenoiser(fqs=2000)
    assert fast.loess_points == 2000 and len(fast.b) == len(E.design_lowpass(2000)[0])
    with pytest.raises(ValueError, match='loess_points = 2000'):
        fast(torch.zeros(2, 12, 64), baseline='rloess')
    with pytest.raises(ValueError, match='loess_points'):
        E.EcgDenoiser(fqs=2000, loess_points=2000)
    x = torch.zeros(2, 12, 64)
    for bad in ('loess', 'RLOESS', ''):
        with pytest.raises(ValueError, match="'rloess'"):
            d(x, baseline=bad)
    with pytest.raises(ValueError, match='baseline'):
        d(x, baseline=np.zeros((2, 12, 63)))
    # which stages run: None and a tensor take the old path, 'rloess' one in-place subtracting sweep between the low-pass and the non-local means
    calls = []
    monkeypatch.setattr(denoise, 'lowpass_taps', lambda rec, *a, **kw: calls.append('lowpass') or np.array(rec, np.float32))
    monkeypatch.setattr(denoise, 'nlm', lambda rec, *a, **kw: calls.append('nlm') or rec)

    def fake_rloess(rec, npoints, **kw):
        calls.append(('rloess', npoints, kw['subtract'], kw['out'] is rec))
        return rec
    monkeypatch.setattr(denoise, 'rloess', fake_rloess)
    h = np.ones((2, 12, 64), np.float32)
    with pytest.raises(ValueError, match='repeats'):                     # the LOESS stage's checks come before the first stage runs
        d(h, baseline='rloess', idxs=[1, 1])
    with pytest.raises(ValueError, match='loess_points = 2000'):
        fast(h, baseline='rloess')
    assert not calls
    assert np.array_equal(fast(h), h) and np.array_equal(fast(h, baseline=0.25 * h), 0.75 * h) and calls == ['lowpass', 'nlm'] * 2
    del calls[:]
    assert np.array_equal(d(h), h) and calls == ['lowpass', 'nlm']
    del calls[:]
    assert np.array_equal(d(h, baseline=0.25 * h), 0.75 * h) and calls == ['lowpass', 'nlm']
    del calls[:]
    d(h, baseline='rloess')
    assert calls == ['lowpass', ('rloess', 500, True, True), 'nlm']
