"""CPU: the host side of `resample` (the length rule, the plan, the refusals that need no device) and the numpy restatement
tests/resample_ref.py that the GPU tests hold the kernels to.  Parity is pinned at `scipy.signal.resample`; the `wfdb` wrapper around it is not
available, so its length rule int(n * fs_target / fs) is restated, not executed."""
import ctypes
import importlib
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN
import ecg_representation_learning_amd as E
import resample_ref as R

RS = importlib.import_module('ecg_representation_learning_amd.resample')    # (the package's `resample` is the function)
ALL_PAIRS = R.PAIRS + [R.LONG_PAIR]


def test_restatement_equals_scipy():
    """resample_ref against scipy.signal.resample on f64 input, over every length pair of the tests: at most 1e-12 of max |x|.  Measured: 0 at
    every pair but the dense-sized ones scipy transforms by another route (at most 1e-15)."""
    signal = pytest.importorskip('scipy.signal')
    rng = np.random.default_rng(1)
    worst = 0.0
    for n, num in ALL_PAIRS:
        x = rng.standard_normal((2, n))
        err = float(np.abs(R.resample_ref(x, num) - signal.resample(x, num, axis=-1)).max()) / float(np.abs(x).max())
        worst = max(worst, err)
        assert err <= 1e-12, (n, num, err)
    print(f'restatement vs scipy: worst {worst:.3e}')


def test_fixture_matches_restatement():
    z = np.load(os.path.join(GOLDEN, 'resample.npz'))
    cases = json.loads(bytes(z['cases']).decode())
    assert len(cases) >= 3
    for i, (n, num) in enumerate(cases):
        x, y64, y32 = z[f'r{i}_in'], z[f'r{i}_out64'], z[f'r{i}_out32']
        assert x.shape == (12, n) and x.dtype == np.float32 and y64.shape == (12, num) and y64.dtype == np.float64 and y32.dtype == np.float32
        amax = float(np.abs(x).max())
        assert float(np.abs(R.resample_ref(x, num) - y64).max()) <= 1e-12 * amax
        e32 = float(np.abs(y32.astype(np.float64) - y64).max()) / amax          # the single-precision path's own error
        assert 1e-9 < e32 < 1e-5, e32


def test_resampled_length():
    """the reference's expression on the corpus shapes; a length that comes out as 0, and a length of 0, are refused"""
    assert E.resampled_length(462600, 257, 250) == 450000
    assert E.resampled_length(4096, 400, 250) == 2560
    assert E.resampled_length(4999, 500, 250) == 2499
    assert E.resampled_length(1000, 250, 257) == 1028
    assert E.resampled_length(5000, 500, 250) == 2500 and E.resampled_length(115200, 1000, 250) == 28800
    for n, f, g in [(7, 500, 250), (1001, 360, 250), (5, 1000, 250.0)]:
        assert E.resampled_length(n, f, g) == int(n * g / f)
    with pytest.raises(ValueError):
        E.resampled_length(0, 500, 250)
    with pytest.raises(ValueError):
        E.resampled_length(1, 500, 250)
    with pytest.raises(ValueError):
        E.resampled_length(100, 0, 250)


def test_plan_through_the_library():
    """ecgvit_resample_plan is host-only: the product of the radices is n, the same call gives the same plan, a prime is its own plan, 1 has
    the empty plan, built radices come largest first and the generic ones after them"""
    lib = E.hip.lib()
    built = set(RS.BUILT_RADICES)
    for n in sorted({n for pair in ALL_PAIRS for n in pair} | {28800, 115200, 1 << 25, 6, 49, 2 * 3 * 5 * 7 * 11 * 13}):
        p = E.resample_plan(n)
        assert int(np.prod(p, dtype=np.int64)) == n and p == E.resample_plan(n), (n, p)
        head = [r for r in p if r in built]
        assert p[:len(head)] == head == sorted(head, reverse=True) and p[len(head):] == sorted(p[len(head):]), (n, p)
        for r in p[len(head):]:
            assert r > 5 and all(r % q for q in range(2, int(r ** 0.5) + 1)), (n, p)      # what is not built is a prime
    assert E.resample_plan(1) == []
    for prime in (7, 251, 257, 4999):
        assert E.resample_plan(prime) == [prime]
    assert E.resample_plan(5000) == [25, 25, 8] and E.resample_plan(4096) == [16, 16, 16] and E.resample_plan(462600) == [25, 8, 3, 3, 257]
    rad = (ctypes.c_int * 32)()
    assert lib.ecgvit_resample_plan(0, rad, 32) == -1 and lib.ecgvit_resample_plan((1 << 25) + 1, rad, 32) == -1
    assert lib.ecgvit_resample_plan(5000, rad, 2) == -1                                  # more radices than the caller's array holds
    with pytest.raises(ValueError):
        E.resample_plan(0)
    # the workspace query is host-only too: two buffers of R * 6 * max(n) complex f64, 0 for what the launcher refuses
    assert lib.ecgvit_resample_workspace(3, 12, 5000, 2500) == 2 * 16 * 3 * 6 * 5000
    assert lib.ecgvit_resample_workspace(3, 11, 5000, 2500) == 0 and lib.ecgvit_resample_workspace(3, 12, 0, 2500) == 0
    assert lib.ecgvit_resample_workspace(1, 12, 131101, 100) == 0                         # a prime above 65 536: its dense pass is not run
    assert lib.ecgvit_resample_workspace(10923, 12, 8, 4) == 0                            # record x lead pair beyond the grid


def test_refusals_without_a_device():
    with pytest.raises(ValueError, match='ragged'):
        E.resample(np.zeros((12, 100), np.float32), 500, offsets=[0, 40, 100], num=50)
    with pytest.raises(ValueError, match='12 leads'):
        E.resample(np.zeros((2, 11, 100), np.float32), 500)
    with pytest.raises(ValueError, match='resamples to 0'):
        E.resample(np.zeros((2, 12, 1), np.float32), 500)
    with pytest.raises(ValueError, match='prime factor'):
        E.resample(np.zeros((1, 12, 131101), np.float32), 500, num=100)
    with pytest.raises(ValueError, match='num'):
        E.resample(np.zeros((2, 12, 100), np.float32), 500, num=0)


def test_pairing_identity():
    """The kernels resample leads 2p and 2p + 1 as one complex sequence under scipy's complex-input rule: resample_ref_complex(x_a + i x_b)
    against resample_ref(x_a) + i resample_ref(x_b), the error relative to max |record|, over every length pair of the tests, with the pair at
    equal scales and with lead a 1e6 times lead b.  E_pair, the measured maximum: 2.3e-15 (at 462 600 -> 450 000; 9.6e-16 below 5 000 samples); the GPU tests' third
    tolerance term, 1e-12 max |record|, must be at least 50 E_pair."""
    rng = np.random.default_rng(2)
    e_pair = 0.0
    for n, num in ALL_PAIRS:
        t = np.arange(n)        # (the long pair: sines and noise, the record of tests/test_gpu_resample.py; beats cost n^2 / 41 to draw)
        x = R.record(rng, n, 2).astype(np.float64) if n <= 5000 else np.sin(2 * np.pi * t * rng.uniform(0.5, 40, (2, 1)) / 257) + rng.normal(0, 0.05, (2, n))
        for scale in (1.0, 1e-6):
            a, b = x[0], x[1] * scale
            y = R.resample_ref_complex(a + 1j * b, num)
            amax = max(float(np.abs(a).max()), float(np.abs(b).max()))
            err = max(float(np.abs(y.real - R.resample_ref(a, num)).max()), float(np.abs(y.imag - R.resample_ref(b, num)).max())) / amax
            e_pair = max(e_pair, err)
    print(f'E_pair = {e_pair:.3e}')
    assert 50 * e_pair <= 1e-12, e_pair


def test_launcher_refuses_before_launching():
    """ecgvit_resample checks its arguments on the host and returns ECGVIT_EINVAL without a launch (the pointers here are never dereferenced)"""
    lib = E.hip.lib()
    x, out, src, dst, tw_a, tw_b, ws = 0x10000000, 0x20000000, 0x30000000, 0x38000000, 0x40000000, 0x50000000, 0x60000000

    def call(x=x, out=out, src=src, dst=dst, R=2, C=12, n_in=40, n_out=20, tw_a=tw_a, ws=ws, s_stride=40):
        return lib.ecgvit_resample(x, out, src, s_stride, dst, 20, R, C, n_in, n_out, tw_a, tw_b, ws, None)
    assert call(x=None) == 1 and call(out=None) == 1 and call(ws=None) == 1 and call(tw_a=None) == 1
    assert call(C=11) == 1 and call(C=0) == 1 and call(R=0) == 1 and call(R=10923) == 1
    assert call(n_in=0) == 1 and call(n_out=(1 << 25) + 1) == 1 and call(n_in=131101) == 1
    assert call(x=x + 2) == 1 and call(src=src + 4) == 1 and call(ws=ws + 8) == 1 and call(tw_a=tw_a + 8) == 1 and call(s_stride=0) == 1
