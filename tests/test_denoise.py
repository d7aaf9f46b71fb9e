"""CPU: the denoiser's restatement (tests/denoise_ref.py) against the fixture the reference's own butterworth_low_pass / est_noise_std / nlm wrote
(tests/golden/denoise.npz, tools/make_golden_denoise.py), the filter design, the ABI of csrc/denoise.hip with every refusal of its launchers
(no GPU is touched: a refused call launches nothing), and the host contract of `denoise`."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
import abi_header
import ecg_representation_learning_amd as E
from ecg_representation_learning_amd import hip, denoise
import denoise_ref as R



@pytest.fixture(scope='module')
def fx():
    z = np.load(os.path.join(GOLDEN, 'denoise.npz'))
    return z, json.loads(bytes(z['nlm_cases']).decode())


# ---- the restatement against the reference's own output ---------------------------------------------
def test_lowpass_restatement_reproduces_the_fixture(fx):
    z, _ = fx
    assert z['lp_lengths'].tolist() == [13, 14, 64, 257]
    for n in z['lp_lengths'].tolist():
        x, want = z[f'lp_{n}_in'].astype(np.float64), z[f'lp_{n}_out']
        got = np.stack([R.filtfilt(z['b_500'], z['a_500'], z['zi_500'], l) for l in x])
        assert got.shape == want.shape == (12, n) and np.abs(got - want).max() <= 1e-12 * np.abs(x).max(), n
    got = np.stack([R.filtfilt(z['b_250'], z['a_250'], z['zi_250'], l) for l in z['lp_64_in'].astype(np.float64)])
    assert np.abs(got - z['lp250_64_out']).max() <= 1e-12 * np.abs(z['lp_64_in']).max()
    with pytest.raises(ValueError, match='padlen'):
        R.filtfilt(z['b_500'], z['a_500'], z['zi_500'], np.zeros(12))


def test_sigma_restatement_reproduces_the_fixture(fx):
    z, _ = fx
    assert z['sg_lengths'].tolist() == [3, 4, 22, 23, 64, 161, 256]
    for n in z['sg_lengths'].tolist():
        got = np.array([R.est_noise_std(l) for l in z[f'sg_{n}_in'].astype(np.float64)])
        want = z[f'sg_{n}_out']
        assert (want > 0).all() and np.all(np.abs(got - want) <= 1e-13 * want), n


def test_nlm_restatement_reproduces_the_fixture(fx):
    z, cases = fx
    assert [tuple(c) for c in cases] == [(21, 10, None), (22, 10, None), (23, 10, None), (64, 3, None), (160, 10, None), (257, 10, None), (257, 10, 40),
                                         (300, 5, 1)]
    for i, (n, p, sw) in enumerate(cases):
        x, sg, want = z[f'nlm{i}_in'].astype(np.float64), z[f'nlm{i}_sigma'], z[f'nlm{i}_out']
        assert np.array_equal(sg, [R.est_noise_std(l) for l in x]) or np.allclose(sg, [R.est_noise_std(l) for l in x], rtol=1e-13, atol=0)
        got = np.stack([R.nlm(l, s, 1.5, p, sw) for l, s in zip(x, sg)])
        assert np.isfinite(want).all() and np.abs(got - want).max() <= 1e-12 * np.abs(x).max(), (n, p, sw, np.abs(got - want).max())
        # the reference's quirks: the first p + 1 and the last p samples are copies, records of n <= 2p + 1 whole
        assert np.array_equal(want[:, :p + 1], x[:, :p + 1]) and np.array_equal(want[:, n - p:], x[:, n - p:])
        changed = (want != x).any(axis=0).sum()
        assert changed == max(0, n - 2 * p - 1), (n, changed)
    const = z['nlmconst_in']
    assert not const[3].any() and R.est_noise_std(const[3].astype(np.float64)) == 0 and np.array_equal(R.nlm(const[3], 0.0), const[3])
    assert 0 < R.est_noise_std(np.full(64, 0.25)) < 1e-9        # a non-zero constant: the in-place recurrence leaves a decaying tail, not zeros


def test_restatement_runs_partition_the_output(fx):
    for n, p in ((23, 10), (36, 10), (37, 10), (160, 10), (64, 3)):
        K = R.n_runs(n, p)
        idx = np.concatenate([R.run_samples(n, p, [k]) for k in range(K)])
        assert np.array_equal(idx, np.arange(p + 1, n - p)), (n, p)
    z, _ = fx
    x, sg = z['nlm4_in'][0].astype(np.float64), z['nlm4_sigma'][0]
    full, part = R.nlm(x, sg), R.nlm(x, sg, runs=[0, 9])
    keep = R.run_samples(160, 10, [0, 9])
    assert np.array_equal(full[keep], part[keep]) and np.array_equal(np.delete(part, keep), np.delete(x, keep))


def test_design_lowpass_reproduces_scipy(fx):
    z, _ = fx
    assert z['band'].tolist() == [50, 60, 1, 2.5] and z['nlm_defaults'].tolist() == [1.5, 10]
    for f in (500, 250):
        b, a, zi = E.design_lowpass(fqs=f)
        assert len(b) == len(a) == int(z[f'ord_{f}']) + 1 == 4 and len(zi) == 3 and a[0] == 1.0
        for got, want in ((b, z[f'b_{f}']), (a, z[f'a_{f}']), (zi, z[f'zi_{f}'])):
            assert got.dtype == np.float64 and np.all(np.abs(got - want) <= 1e-9 * np.abs(want)), (f, got, want)
    assert all(np.array_equal(u, v) for u, v in zip(E.design_lowpass(), E.design_lowpass(500, 50, 60, 1, 2.5)))
    for bad in (dict(passband=60, stopband=50), dict(stopband=250), dict(passband=0), dict(passband_ripple=3), dict(passband_ripple=0),
                dict(passband=50, stopband=50.5)):
        with pytest.raises(ValueError):
            E.design_lowpass(**bad)


# ---- ABI ----------------------------------------------------------------------------------------------
ARITY = {'ecgvit_denoise_workspace': 3, 'ecgvit_filtfilt': 15, 'ecgvit_nlm_sigma': 10, 'ecgvit_nlm_denoise': 13}


def test_symbols_exist_with_the_declared_arity():
    lib = hip.lib()
    abi_header.held(ARITY, hip.SIGNATURES)                  # declared, with this many arguments, bound with the declaration's types
    for name in ARITY:
        assert hasattr(lib, name)
    assert lib.ecgvit_abi_version() == 6 and hip.DENOISE_MAX_LEN == denoise.MAX_LEN == 32768 and hip.DENOISE_MAX_TAPS == denoise.MAX_TAPS == 9


P = 0x10000000      # never dereferenced: a refused call launches nothing
B4 = (ctypes.c_double * 4)(0.1, 0.3, 0.3, 0.1)
A4 = (ctypes.c_double * 4)(1.0, -0.5, 0.2, -0.1)
Z3 = (ctypes.c_double * 3)(0.9, -0.2, 0.1)
IDS = dict(ids=lambda d: ','.join(f'{k}={v if not isinstance(v, ctypes.Array) else list(v)}' for k, v in d.items()))


def _filt(**kw):
    a = dict(x=P, out=P, src_off=P, lead_stride=64, raw_len=P, R=4, C=12, min_len=64, max_len=64, b=B4, a=A4, zi=Z3, ntaps=4, workspace=P, stream=None)
    a.update(kw)
    return hip.lib().ecgvit_filtfilt(*a.values())


def _sigma(**kw):
    a = dict(x=P, src_off=P, lead_stride=64, raw_len=P, R=4, C=12, max_len=64, sigma=P, workspace=P, stream=None)
    a.update(kw)
    return hip.lib().ecgvit_nlm_sigma(*a.values())


def _nlm(**kw):
    a = dict(x=P, out=P, src_off=P, lead_stride=64, raw_len=P, R=4, C=12, max_len=64, sigma=P, scale=1.5, patch_wd=10, sch_wd=0, stream=None)
    a.update(kw)
    return hip.lib().ecgvit_nlm_denoise(*a.values())


BAD_STORE = [dict(x=None), dict(x=P + 2), dict(src_off=None), dict(src_off=P + 4), dict(raw_len=None), dict(raw_len=P + 2), dict(R=0), dict(R=-1), dict(C=0),
             dict(C=65536), dict(max_len=0), dict(max_len=-5), dict(max_len=32769)]


@pytest.mark.parametrize('bad', BAD_STORE + [dict(out=None), dict(out=P + 2), dict(workspace=None), dict(workspace=P + 4), dict(b=None), dict(a=None), dict(zi=None),
                                             dict(ntaps=0), dict(ntaps=10), dict(min_len=12, ntaps=4), dict(min_len=0), dict(min_len=65),
                                             dict(min_len=27, max_len=64, ntaps=9), dict(a=(ctypes.c_double * 4)(2.0, 0, 0, 0)),
                                             dict(b=(ctypes.c_double * 4)(float('nan'), 0, 0, 0)), dict(a=(ctypes.c_double * 4)(1.0, float('inf'), 0, 0)),
                                             dict(zi=(ctypes.c_double * 3)(0, float('nan'), 0))], **IDS)
def test_filtfilt_refusals(bad):
    assert _filt(**bad) == 1


@pytest.mark.parametrize('bad', BAD_STORE + [dict(sigma=None), dict(sigma=P + 4), dict(workspace=None), dict(workspace=P + 4)], **IDS)
def test_sigma_refusals(bad):
    assert _sigma(**bad) == 1


@pytest.mark.parametrize('bad', BAD_STORE + [dict(out=None), dict(out=P + 2), dict(sigma=None), dict(sigma=P + 4), dict(patch_wd=0), dict(patch_wd=-1),
                                             dict(patch_wd=32769), dict(sch_wd=-1), dict(scale=0.0), dict(scale=-1.5), dict(scale=float('nan')),
                                             dict(scale=float('inf'))], **IDS)
def test_nlm_refusals(bad):
    assert _nlm(**bad) == 1


def test_workspace_size():
    l = hip.lib()
    assert l.ecgvit_denoise_workspace(4, 12, 5000) == 4 * 12 * (5000 + 64) * 8
    assert l.ecgvit_denoise_workspace(0, 12, 64) == 0 and l.ecgvit_denoise_workspace(4, 0, 64) == 0 and l.ecgvit_denoise_workspace(4, 12, 32769) == 0
    assert l.ecgvit_denoise_workspace(4, 12, 32768) > 0


# ---- host contract ----------------------------------------------------------------------------------------
def test_exports_and_constructor():
    for name in ('EcgDenoiser', 'design_lowpass', 'lowpass', 'estimate_noise_std', 'nlm', 'denoise'):
        assert name in E.__all__ and hasattr(E, name)
    d = E.EcgDenoiser()
    assert (d.fqs, d.scale, d.search_width, d.patch_width) == (500, 1.5, None, 10) and not hasattr(d, 'zheng')
    assert np.array_equal(d.b, E.design_lowpass(500)[0]) and not np.array_equal(E.EcgDenoiser(fqs=250).b, d.b)
    for bad in (dict(patch_width=0), dict(patch_width=2.5), dict(search_width=0), dict(search_width=-3), dict(scale=0), dict(scale=float('nan'))):
        with pytest.raises(ValueError):
            E.EcgDenoiser(**bad)
    with pytest.raises(ValueError, match='baseline'):
        d(torch.zeros(2, 12, 64), baseline=np.zeros((2, 12, 63)))
    with pytest.raises(ValueError, match='12 leads'):
        d(np.zeros((2, 3, 64), np.float32))


def test_host_api_refusals():
    x = torch.zeros(2, 12, 64)
    for bad in (dict(patch_width=0), dict(patch_width=True + 0.5), dict(search_width=0), dict(search_width=1.5), dict(scale=-1), dict(scale=float('inf'))):
        with pytest.raises(ValueError, match=next(iter(bad))):
            E.nlm(x, **bad)
    for fn in (E.lowpass, E.estimate_noise_std, E.nlm):
        with pytest.raises(ValueError, match='32768'):                   # over the length cap
            fn(np.zeros((1, 12, 32769), np.float32))
        with pytest.raises(ValueError, match='12 leads'):
            fn(np.zeros((2, 3, 64), np.float32))
        with pytest.raises(ValueError, match='offsets'):
            fn(np.zeros((12, 64), np.float32))
        with pytest.raises(ValueError, match='idxs'):
            fn(x, idxs=[2])
        with pytest.raises(ValueError, match='float'):
            fn(np.zeros((2, 12, 64), np.int16))
    with pytest.raises(ValueError, match='at least 13'):                 # length padlen: where scipy raises
        E.lowpass(np.zeros((1, 12, 12), np.float32))
    with pytest.raises(ValueError, match='at least 13'):
        E.lowpass(np.zeros((12, 30), np.float32), offsets=[0, 12, 30])
    with pytest.raises(ValueError, match='a\\[0\\]'):
        denoise.lowpass_taps(x, [1.0, 1.0], [2.0, 1.0])
    with pytest.raises(ValueError, match='taps'):
        denoise.lowpass_taps(x, np.ones(10), np.r_[1.0, np.zeros(9)])
    with pytest.raises(ValueError, match='zi'):
        denoise.lowpass_taps(x, [0.5, 0.5], [1.0, 0.1], zi=[0.0, 0.0])
    with pytest.raises(ValueError, match='finite'):
        denoise.lowpass_taps(x, [0.5, float('nan')], [1.0, 0.1])
    for sg in (np.zeros((2, 11)), np.zeros(24), torch.zeros(2, 12), np.zeros((3, 12))):     # shape, dtype, rows per selected record
        with pytest.raises(ValueError, match='sigma'):
            E.nlm(x, sigma=sg)
    with pytest.raises(ValueError, match='sigma'):
        E.nlm(x, sigma=np.zeros((2, 12)), idxs=[1])
    for out in (np.zeros((2, 12, 64)), np.zeros((2, 12, 63), np.float32), torch.zeros(2, 12, 64)):   # a host store's out: float32 numpy of its shape
        with pytest.raises(ValueError, match='out'):
            E.lowpass(x, out=out)
    with pytest.raises(ValueError, match='chunk_records'):
        E.lowpass(x, chunk_records=0)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match='no CPU fallback'):
            E.lowpass(x)
