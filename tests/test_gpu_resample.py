"""GPU: csrc/resample.hip through `resample` against the numpy f64 restatement of `scipy.signal.resample` (tests/resample_ref.py, which
tests/test_resample.py holds to scipy itself) and against the fixture of scipy's own single-precision output, which is what the reference's
call computes (tests/golden/resample.npz).  Parity is pinned at the scipy call; the `wfdb` wrapper is not available and its length rule is
restated.

Tolerance against the restatement, per element: |out - ref64| <= 2^-24 |ref64| + 1e-8 max |lead| + 1e-12 max |record| -- the f32 store's
rounding; the bound the project's f64 kernels are held to (tests/test_gpu_loess.py); and the partner lead of the pair, which shares the complex
transform: 1e-12 is over 400 E_pair (tests/test_resample.py measures E_pair = 2.3e-15), and an f64 FFT's own error, eps (log2 n + r_max)
sqrt(n) max |x|, stays below 1e-11 at every shape here.  `lead` and `record` are the input's.
Against the fixture's single-precision output: min(1e-4, max(2^-20, 8 E32)) of max |x|, E32 = the fixture's own |f32 path - f64 path| / max |x|.

MEASURED on the MI355X, the largest |out - ref64| as a fraction of the tolerance, per family (the f32 store's rounding alone reaches
0.5 to 1.0 of the first term): radix 0.851; generic 0.809 (7 -> 21: 0.756, 257 -> 250: 0.786, 250 -> 257: 0.809, 251 -> 125: 0.780);
nyquist 0.836 (30 -> 20: 0.795, 20 -> 30: 0.674, 31 -> 17: 0.815, 17 -> 31: 0.826, 32 -> 16 and 16 -> 32: 0.777, 1000 -> 999: 0.783,
999 -> 1000: 0.836); degenerate 0.785 (1 -> 2: 0, the copy of one sample); corpus 0.841 (5000 -> 2500: 0.833, 4096 -> 2560: 0.800,
1028 -> 1000: 0.841, 4999 -> 2499: 0.806); 462 600 -> 450 000: 0.845.
Fixture (E32, bound, kernel error, of max |x|): 257 -> 250: 3.2e-7, 2.5e-6, 2.9e-7; 96 -> 60: 1.2e-7, 9.8e-7, 1.4e-7; 40 -> 64: 1.4e-7, 1.1e-6,
1.6e-7; 31 -> 17: 9.5e-8, 9.5e-7 (the floor 2^-20), 9.4e-8.
Pair independence, lead 1 at 1e-3 beside lead 0 at 1e3: 0.028 (250 -> 257), 0.044 (5000 -> 2500), 0.045 (257 -> 250) of its tolerance; the
swapped pairs 0.79, 0.79, 0.75 of theirs, and not bit-equal to the unswapped outputs at any of the three.
"""
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
import ecg_representation_learning_amd as E
import resample_ref as R

pytestmark = pytest.mark.gpu


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x, np.float32)).cuda()


def excess(got, x, num):
    """got, x: (12, num), (12, n) -> the largest |got - ref64| / tolerance over the record (at most 1 passes)"""
    ref = R.resample_ref(x, num)
    lead = np.abs(x).max(axis=1, keepdims=True).astype(np.float64)
    tol = 2.0 ** -24 * np.abs(ref) + 1e-8 * lead + 1e-12 * float(lead.max())
    assert got.shape == ref.shape and got.dtype == np.float32
    return float((np.abs(got.astype(np.float64) - ref) / tol).max())


FAMILIES = dict(radix=R.RADIX_PAIRS, generic=R.GENERIC_PAIRS, nyquist=R.NYQUIST_PAIRS, degenerate=R.DEGENERATE_PAIRS, corpus=R.CORPUS_PAIRS)


@pytest.mark.parametrize('family', list(FAMILIES))
def test_length_pairs(family):
    """2 records x 12 leads per (n_in, n_out), through num=: every built radix alone and inside a plan, the generic pass as a factor and as
    the dense DFT, every Nyquist branch (N even / odd, down / up), the shortest lengths, the corpus shapes"""
    rng = np.random.default_rng(len(family))
    worst = 0.0
    for n, num in FAMILIES[family]:
        x = np.stack([R.record(rng, n), R.record(rng, n)])
        got = E.resample(dev(x), 500, num=num)
        assert got.shape == (2, 12, num) and got.is_cuda
        got = got.cpu().numpy()
        ex = max(excess(got[0], x[0], num), excess(got[1], x[1], num))
        print(f'{family} {n} -> {num} (plans {E.resample_plan(n)}, {E.resample_plan(num)}): error / tolerance {ex:.3f}')
        worst = max(worst, ex)
        assert ex <= 1.0, (n, num, ex)
    print(f'{family}: worst error / tolerance {worst:.3f}')


def test_copies_are_bit_equal():
    rng = np.random.default_rng(7)
    x = np.stack([R.record(rng, 12), R.record(rng, 12)])
    xd = dev(x)
    for got in (E.resample(xd, 500, num=12), E.resample(xd, 250), E.resample(xd, 360.0, 360)):
        assert got.data_ptr() != xd.data_ptr() and np.array_equal(got.cpu().numpy(), x)
    rag = np.concatenate([R.record(rng, 31), R.record(rng, 40)], axis=1)
    got, off = E.resample(dev(rag), 250, offsets=[0, 31, 71], idxs=[1, 0])
    assert off.tolist() == [0, 40, 71] and np.array_equal(got.cpu().numpy(), np.concatenate([rag[:, 31:], rag[:, :31]], axis=1))


def test_long_record_above_the_resident_cap():
    """one record of INCART's length, 462 600 -> 450 000 at 257 -> 250 Hz: the plan holds the generic radix 257 (and 64-bit record indexing)"""
    n, num = R.LONG_PAIR
    assert 257 in E.resample_plan(n) and E.resampled_length(n, 257, 250) == num
    rng = np.random.default_rng(11)
    t = np.arange(n, dtype=np.float64)
    x = np.stack([np.sin(2 * np.pi * t * rng.uniform(0.5, 40) / 257 + c) * rng.uniform(0.5, 2) + rng.normal(0, 0.05, n) for c in range(12)]).astype(np.float32)
    got = E.resample(dev(x[None]), 257, 250)
    assert got.shape == (1, 12, num)
    ex = excess(got[0].cpu().numpy(), x, num)
    print(f'{n} -> {num}: error / tolerance {ex:.3f}')
    assert ex <= 1.0, ex


def test_fixture_single_precision_path():
    z = np.load(os.path.join(GOLDEN, 'resample.npz'))
    for i, (n, num) in enumerate(json.loads(bytes(z['cases']).decode())):
        x, y64, y32 = z[f'r{i}_in'], z[f'r{i}_out64'], z[f'r{i}_out32']
        amax = float(np.abs(x).max())
        e32 = float(np.abs(y32.astype(np.float64) - y64).max()) / amax
        bound = min(1e-4, max(2.0 ** -20, 8 * e32))
        got = E.resample(dev(x[None]), 500, num=num)[0].cpu().numpy()
        err = float(np.abs(got.astype(np.float64) - y32).max()) / amax
        print(f'fixture {n} -> {num}: E32 {e32:.3e}  bound {bound:.3e}  kernel {err:.3e}')
        assert err <= bound, (n, num, err, bound)
        assert excess(got, x, num) <= 1.0


def test_pair_independence():
    """lead 0 scaled by 1e3 beside lead 1 scaled by 1e-3 in one complex transform: lead 1 keeps the tolerance (its third term, 1e-12 of the
    record's largest sample, is what the partner may leak).  Swapping the two leads of every pair swaps the outputs within the tolerance, not
    bit for bit: the swap is z -> i conj(z), which mirrors the spectrum, and the passes do not treat bin k and bin n - k alike (the table's
    entries k and n - k are not exact conjugates, and the sums run in ascending q either way)."""
    rng = np.random.default_rng(13)
    worst = 0.0
    for n, num in [(250, 257), (5000, 2500), (257, 250)]:
        x = R.record(rng, n)
        x[0] *= np.float32(1e3)
        x[1] *= np.float32(1e-3)
        got = E.resample(dev(x[None]), 500, num=num)[0].cpu().numpy()
        ref = R.resample_ref(x, num)
        tol1 = 2.0 ** -24 * np.abs(ref[1]) + 1e-8 * float(np.abs(x[1]).max()) + 1e-12 * float(np.abs(x).max())
        ex1 = float((np.abs(got[1].astype(np.float64) - ref[1]) / tol1).max())
        swapped = x.reshape(6, 2, n)[:, ::-1].reshape(12, n)
        got_s = E.resample(dev(swapped[None]), 500, num=num)[0].cpu().numpy()
        ex_s = excess(got_s, swapped, num)
        same = np.array_equal(got_s.reshape(6, 2, num)[:, ::-1].reshape(12, num), got)
        print(f'{n} -> {num}: lead 1 beside a 1e6 times larger partner: error / tolerance {ex1:.3f}; swapped {ex_s:.3f}; swap bit-equal: {same}')
        worst = max(worst, ex1, excess(got, x, num), ex_s)
    assert worst <= 1.0, worst


def test_store_forms_are_bit_identical():
    """a ragged store of mixed lengths, the same records as rectangles one by one, a subset with a repeat, a host array one record per chunk,
    a workspace that forces a record group per record: the same bits per record; new offsets = the cumulative resampled_length"""
    rng = np.random.default_rng(17)
    lens = [40, 31, 40, 257, 96, 40]
    recs = [R.record(rng, n) for n in lens]
    rag = np.concatenate(recs, axis=1)
    off = np.concatenate([[0], np.cumsum(lens)])
    want = [E.resample(dev(r[None]), 500, 250)[0].cpu().numpy() for r in recs]
    new = np.concatenate([[0], np.cumsum([E.resampled_length(n, 500, 250) for n in lens])])

    def check(res, ids):
        out, noff = res
        out = out.cpu().numpy() if isinstance(out, torch.Tensor) else out
        assert noff.tolist() == np.concatenate([[0], np.cumsum([want[i].shape[1] for i in ids])]).tolist() and out.shape == (12, noff[-1])
        for k, i in enumerate(ids):
            assert np.array_equal(out[:, noff[k]:noff[k + 1]], want[i]), (k, i)
    res = E.resample(dev(rag), 500, 250, offsets=off)
    assert res[1].tolist() == new.tolist() and res[0].is_cuda
    check(res, range(6))
    check(E.resample(dev(rag), 500, 250, offsets=off, idxs=[3, 0, 3, 5]), [3, 0, 3, 5])
    host = E.resample(rag.astype(np.float64), 500, 250, offsets=off, chunk_records=1)
    assert isinstance(host[0], np.ndarray) and host[0].dtype == np.float32
    check(host, range(6))
    need = E.hip.lib().ecgvit_resample_workspace(1, 12, 40, 20)
    check(E.resample(dev(rag), 500, 250, offsets=off, idxs=[0, 2, 5], workspace_bytes=need), [0, 2, 5])
    # a rectangle: a batch, a subset with a repeat, a host array in chunks, one record per group
    rect = np.stack([recs[0], recs[2], recs[5]])
    one = np.stack([want[0], want[2], want[5]])
    assert np.array_equal(E.resample(dev(rect), 500).cpu().numpy(), one)
    assert np.array_equal(E.resample(dev(rect), 500, idxs=[2, 2, 0]).cpu().numpy(), one[[2, 2, 0]])
    assert np.array_equal(E.resample(rect, 500, chunk_records=2), one)
    assert np.array_equal(E.resample(dev(rect), 500, workspace_bytes=need).cpu().numpy(), one)


def test_refusals():
    x = torch.zeros(2, 12, 40, device='cuda')
    with pytest.raises(ValueError, match='CPU tensor'):
        E.resample(x.cpu(), 500)
    with pytest.raises(ValueError, match='float32'):
        E.resample(x.double(), 500)
    with pytest.raises(ValueError, match='contiguous'):
        E.resample(torch.zeros(2, 12, 80, device='cuda')[..., ::2], 500)
    with pytest.raises(ValueError, match='resamples to 0'):
        E.resample(torch.zeros(2, 12, 1, device='cuda'), 500)
    need = E.hip.lib().ecgvit_resample_workspace(1, 12, 40, 20)
    with pytest.raises(ValueError, match=str(need)):
        E.resample(x, 500, workspace_bytes=need - 1)
    with pytest.raises(ValueError, match='ragged'):
        E.resample(torch.zeros(12, 80, device='cuda'), 500, offsets=[0, 40, 80], num=20)


def test_resample_feeds_the_denoiser_on_one_resident_store():
    rng = np.random.default_rng(19)
    x = dev(np.stack([R.record(rng, 1000), R.record(rng, 1000)]))
    y = E.resample(x, 500)
    out = E.EcgDenoiser(fqs=250)(y)
    assert y.shape == (2, 12, 500) and out.is_cuda and out.shape == y.shape and bool(torch.isfinite(out).all()) and not torch.equal(out, y)
