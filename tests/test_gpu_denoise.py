"""GPU: csrc/denoise.hip through `denoise` against the fixture of the reference's own output (tests/golden/denoise.npz) and the numpy
restatement (tests/denoise_ref.py).

Non-local means tolerance, per case: E32 = max |restatement in f32 - reference| / max |x| on the CPU, bound = 8 E32 clipped to [2^-20, 1e-4]
(the factor covers the hardware exp and a different run length; 1e-4 is the project's f32 parity gate).  Measured on the MI355X (kernel error /
max |x| beside the bound), fixture cases (n, p, sch_wd):
  (21, 10, None): copied through, bit-equal;  (22, 10, None): one sample denoised, E32 2.5e-8, bound 9.5e-7, kernel 4.3e-8;  (23, 10, None): E32 1.8e-7, bound 1.4e-6, kernel 1.8e-7;
  (64, 3, None): E32 2.3e-7, bound 1.9e-6, kernel 2.3e-7;  (160, 10, None): E32 5.6e-7, bound 4.5e-6, kernel 5.6e-7;
  (257, 10, None): E32 1.2e-6, bound 9.2e-6, kernel 1.2e-6;  (257, 10, 40): E32 4.2e-7, bound 3.3e-6, kernel 4.7e-7;
  (300, 5, 1): E32 2.6e-16, bound 9.5e-7 (the floor 2^-20), kernel 2.6e-16.
  Boundary cases (worst lead; kernel against the f32 restatement, bound): M = 1: 4.4e-8 (9.5e-7); 14: 7.6e-8 (2.6e-6); 15: 2.0e-8 (9.5e-7);
  16: 6.2e-8 (1.4e-6); 959: 1.6e-7 (1.3e-5); 960: 1.5e-7 (2.4e-5); 961: 1.2e-7 (1.1e-5); 7679: 1.6e-7 (E32 1.0e-5, bound 8.2e-5);
  7680: 1.6e-7 (E32 9.9e-6, bound 7.9e-5); 7681: 1.7e-7 (E32 1.1e-5, bound 9.1e-5); the cap, n = 32768: 1.4e-7 (E32 3.0e-5, bound 1e-4, the gate).
"""
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
import ecg_representation_learning_amd as E
from ecg_representation_learning_amd import denoise
import denoise_ref as R

pytestmark = pytest.mark.gpu
P = 10


@pytest.fixture(scope='module')
def fx():
    z = np.load(os.path.join(GOLDEN, 'denoise.npz'))
    return z, json.loads(bytes(z['nlm_cases']).decode())


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x, np.float32)).cuda()


def bound(e32):
    return min(1e-4, max(2.0 ** -20, 8 * e32))


def leads(rng, n, C=12):
    """beats, sway and noise, as the fixture's records"""
    t = np.arange(n, dtype=np.float64)
    out = np.empty((C, n), np.float32)
    for c in range(C):
        beats = sum(np.exp(-0.5 * ((t - t0) / 2.5) ** 2) for t0 in np.arange(rng.uniform(0, 41), n + 41, 41))
        out[c] = (rng.uniform(0.5, 1.5) * beats + 0.2 * np.sin(2 * np.pi * t / rng.uniform(150, 400) + rng.uniform(0, 6)) + rng.normal(0, 0.05, n)).astype(np.float32)
    return out


def test_lowpass_fixture(fx):
    z, _ = fx
    for n in z['lp_lengths'].tolist():
        want = z[f'lp_{n}_out']
        got = E.lowpass(dev(z[f'lp_{n}_in'][None]))[0].cpu().numpy().astype(np.float64)
        err = np.abs(got - want).max()
        print(f'lowpass n={n}: max err {err:.3e}, bound {2.0 ** -23 * np.abs(want).max():.3e}')
        assert np.all(np.abs(got - want) <= 2.0 ** -23 * np.abs(want).max()), n
    want = z['lp250_64_out']
    got = E.lowpass(dev(z['lp_64_in'][None]), fqs=250)[0].cpu().numpy().astype(np.float64)
    assert np.all(np.abs(got - want) <= 2.0 ** -23 * np.abs(want).max())
    with pytest.raises(ValueError, match='at least 13'):        # length padlen: where scipy raises
        E.lowpass(torch.zeros(1, 12, 12, device='cuda'))


def test_sigma_fixture(fx):
    z, _ = fx
    for n in z['sg_lengths'].tolist():
        want = z[f'sg_{n}_out']
        got = E.estimate_noise_std(dev(z[f'sg_{n}_in'][None]))
        assert got.shape == (1, 12) and got.dtype == torch.float64
        rel = np.abs(got[0].cpu().numpy() - want) / want
        print(f'sigma n={n}: max rel {rel.max():.3e}')
        assert np.all(rel <= 1e-12), (n, rel)


def test_nlm_fixture_tolerance_and_edges(fx):
    z, cases = fx
    for i, (n, p, sw) in enumerate(cases):
        x, sg, want = z[f'nlm{i}_in'], z[f'nlm{i}_sigma'], z[f'nlm{i}_out']
        amax = float(np.abs(x).max())
        f32 = np.stack([R.nlm(l, s, 1.5, p, sw, dtype=np.float32) for l, s in zip(x, sg)])
        e32 = float(np.abs(f32.astype(np.float64) - want).max()) / amax
        got = E.nlm(dev(x[None]), search_width=sw, patch_width=p)[0].cpu().numpy()
        err = float(np.abs(got.astype(np.float64) - want).max()) / amax
        print(f'nlm ({n}, {p}, {sw}): E32 {e32:.3e}  bound {bound(e32):.3e}  kernel {err:.3e}')
        assert err <= bound(e32), (n, p, sw, err, bound(e32))
        assert np.array_equal(got[:, :p + 1], x[:, :p + 1]) and np.array_equal(got[:, n - p:], x[:, n - p:])      # the copied samples: bit-equal
        if n <= 2 * p + 1:
            assert np.array_equal(got, x)                                                                          # n = 21, 22: copied through
        if (n, p) == (23, 10):
            assert (got != x).any(axis=0).nonzero()[0].tolist() == [11, 12]                                        # exactly two samples denoised
    x = z['nlmconst_in']
    got = E.nlm(dev(x[None]))[0].cpu().numpy()
    assert float(E.estimate_noise_std(dev(x[None]))[0, 3]) == 0.0 and np.array_equal(got[3], x[3]) and not np.array_equal(got[2], x[2])
    assert np.isfinite(got).all()


# output samples M = n - 2p - 1: one; around a lane's run (15), a wave's span (64 x 15), a workgroup's span (512 x 15)
@pytest.mark.parametrize('M', [1, 14, 15, 16, 959, 960, 961, 7679, 7680, 7681])
def test_nlm_boundaries(M):
    n = M + 2 * P + 1
    x = leads(np.random.default_rng(M), n, 12)
    sg = np.array([R.est_noise_std(l.astype(np.float64)) for l in x])
    got = E.nlm(dev(x[None]), sigma=sg[None])[0].cpu().numpy()
    assert np.array_equal(got[:, :P + 1], x[:, :P + 1]) and np.array_equal(got[:, n - P:], x[:, n - P:])
    # up to a wave's span every output sample is held; around a workgroup's span (n = 7700: 9 s per lead in numpy) every 8th run, both ends and the
    # runs on either side of the workgroup's last lane
    K = R.n_runs(n, P)
    runs = None if n < 2000 else sorted(k for k in set(range(0, K, 8)) | {1, 510, 511, 512, 513, K - 2, K - 1} if k < K)
    keep = np.arange(n) if runs is None else R.run_samples(n, P, runs)
    assert np.isfinite(got).all() and (got[:, P + 1:n - P] != x[:, P + 1:n - P]).mean() > 0.99
    for c in ((0, 7) if n < 2000 else (5,)):
        ref, f32 = R.nlm(x[c].astype(np.float64), sg[c], runs=runs), R.nlm(x[c], sg[c], dtype=np.float32, runs=runs)
        amax = float(np.abs(x[c]).max())
        e32 = float(np.abs(f32 - ref).max()) / amax
        err = float(np.abs(got[c][keep] - f32[keep]).max()) / amax
        print(f'nlm boundary M={M} lead {c}: E32 {e32:.3e}  bound {bound(e32):.3e}  kernel vs f32 restatement {err:.3e}  vs f64 {np.abs(got[c][keep] - ref[keep]).max() / amax:.3e}')
        assert err <= bound(e32), (M, c, err, bound(e32))


def test_nlm_length_cap():
    n = denoise.MAX_LEN
    x = leads(np.random.default_rng(7), n, 1).repeat(12, axis=0)
    x[1:] *= np.linspace(0.5, 1.5, 11, dtype=np.float32)[:, None]
    sg = np.array([R.est_noise_std(l.astype(np.float64)) for l in x])
    sg_dev = E.estimate_noise_std(dev(x[None]))[0].cpu().numpy()
    assert np.all(np.abs(sg_dev - sg) <= 1e-12 * sg)
    got = E.nlm(dev(x[None]), sigma=sg[None])[0].cpu().numpy()
    K = R.n_runs(n, P)
    runs = [0, 1, 63, 64, 511, 512, 513, 1301, K - 2, K - 1]         # a strided sample of the runs: both ends, around a wave's and a workgroup's span
    keep = R.run_samples(n, P, runs)
    for c in (0, 11):
        ref, f32 = R.nlm(x[c].astype(np.float64), sg[c], runs=runs), R.nlm(x[c], sg[c], dtype=np.float32, runs=runs)
        amax = float(np.abs(x[c]).max())
        e32 = float(np.abs(f32[keep] - ref[keep]).max()) / amax
        err = float(np.abs(got[c][keep] - f32[keep]).max()) / amax
        print(f'nlm cap n={n} lead {c}: E32 {e32:.3e}  bound {bound(e32):.3e}  kernel vs f32 restatement {err:.3e}')
        assert err <= bound(e32), (c, err, bound(e32))
    assert np.isfinite(got).all() and (got[:, P + 1:n - P] != x[:, P + 1:n - P]).mean() > 0.99
    for fn in (E.nlm, E.lowpass, E.estimate_noise_std):
        with pytest.raises(ValueError, match='32768'):               # a sample over the cap
            fn(torch.zeros(1, 12, n + 1, device='cuda'))


# ---- layouts --------------------------------------------------------------------------------------------
L = 161
RAGGED_LENGTHS = [37, L, 64, L, L, 23]       # offsets 37, 198, 262, 423, 584: odd 4-byte addresses
SHARED = [1, 3, 4]                           # where the rectangle's three records sit in the ragged store


@pytest.fixture(scope='module')
def stores():
    rng = np.random.default_rng(11)
    recs = [leads(rng, l) for l in RAGGED_LENGTHS]
    rect = np.stack([recs[i] for i in SHARED])
    off = np.concatenate([[0], np.cumsum(RAGGED_LENGTHS)])
    return rect, np.concatenate(recs, axis=1), off


def guarded(shape):
    """-> (flat buffer filled with a pattern, the view of `shape` in its middle)"""
    n = int(np.prod(shape))
    flat = torch.full((n + 512,), -7.25, device='cuda')
    return flat, flat[256:256 + n].view(shape)


STAGES = {'lowpass': lambda x, **kw: E.lowpass(x, **kw), 'nlm': lambda x, **kw: E.nlm(x, **kw)}


@pytest.mark.parametrize('stage', ['lowpass', 'nlm'])
def test_layouts_give_the_same_bits(stores, stage):
    rect_h, rag_h, off = stores
    fn = STAGES[stage]
    rect, rag = dev(rect_h), dev(rag_h)
    base = fn(rect).cpu().numpy()                                             # the rectangle, into a new tensor
    assert not np.array_equal(base, rect_h) and np.array_equal(rect.cpu().numpy(), rect_h)     # the input is not modified
    # each record alone
    for i in range(3):
        assert np.array_equal(fn(rect[i:i + 1].contiguous())[0].cpu().numpy(), base[i])
    # in place equals out=
    inpl = rect.clone()
    assert fn(inpl, out=inpl) is inpl and np.array_equal(inpl.cpu().numpy(), base)
    # a subset of the rectangle into a guarded out: the other record and the guard band keep their bits
    flat, out = guarded(rect.shape)
    fn(rect, idxs=[2, 0], out=out)
    o = out.cpu().numpy()
    assert np.array_equal(o[2], base[2]) and np.array_equal(o[0], base[0]) and (o[1] == -7.25).all()
    assert (flat[:256] == -7.25).all() and (flat[-256:] == -7.25).all()
    # the ragged store: every record, then a subset in place (the records between the selected ones are its gaps)
    r_all = fn(rag, offsets=off).cpu().numpy()
    for j, i in enumerate(SHARED):
        assert np.array_equal(r_all[:, off[i]:off[i + 1]], base[j]), i
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
    h = fn(rect_h, chunk_records=2)
    assert isinstance(h, np.ndarray) and h.dtype == np.float32 and np.array_equal(h, base)
    h = fn(rag_h, offsets=off, idxs=[4, 1], chunk_records=1)
    assert np.array_equal(h[:, off[4]:off[5]], base[2]) and np.array_equal(h[:, mask], rag_h[:, mask])


def test_sigma_layouts_give_the_same_bits(stores):
    rect_h, rag_h, off = stores
    rect, rag = dev(rect_h), dev(rag_h)
    base = E.estimate_noise_std(rect).cpu().numpy()
    assert base.shape == (3, 12) and (base > 0).all()
    for i in range(3):
        assert np.array_equal(E.estimate_noise_std(rect[i:i + 1].contiguous())[0].cpu().numpy(), base[i])
    assert np.array_equal(E.estimate_noise_std(rect, idxs=[2, 0]).cpu().numpy(), base[[2, 0]])
    r_all = E.estimate_noise_std(rag, offsets=off).cpu().numpy()
    assert r_all.shape == (6, 12) and np.array_equal(r_all[SHARED], base)
    assert np.array_equal(E.estimate_noise_std(rag, offsets=off, idxs=[4, 1]).cpu().numpy(), base[[2, 0]])
    assert np.array_equal(E.estimate_noise_std(rag_h, offsets=off, chunk_records=4).cpu().numpy(), r_all)
    assert np.array_equal(rect.cpu().numpy(), rect_h)
    # nlm with the table passed equals nlm that estimates it
    assert torch.equal(E.nlm(rect, sigma=torch.from_numpy(base)), E.nlm(rect))


def test_a_passed_sigma_table_follows_the_host_chunks(stores):
    """row `first` of a passed table belongs to the first record of a chunk: the second chunk of a host store reads its own rows"""
    rect_h = stores[0]
    rect = dev(rect_h)
    table = E.estimate_noise_std(rect)
    assert np.array_equal(E.nlm(rect_h, sigma=table, chunk_records=2), E.nlm(rect).cpu().numpy())
    want = E.nlm(rect, idxs=[2, 0]).cpu().numpy()
    for chunk in (2, 1):
        assert np.array_equal(E.nlm(rect_h, sigma=table[[2, 0]], idxs=[2, 0], chunk_records=chunk), want)


@pytest.mark.parametrize('long', [4300, 8300])
def test_a_record_beside_a_long_one_keeps_its_bits(stores, long):
    """the longest record of a launch picks the LDS size of the non-local means (4096 / 8192 / 32768 samples), its workgroup size (64 lanes for
    161 samples, 320 / 512 here) and the workspace pitch of the other two kernels: none of them may reach a record's bits"""
    rect_h = stores[0]
    rect = dev(rect_h[:1])
    rag_h = np.concatenate([rect_h[0], leads(np.random.default_rng(long), long)], axis=1)
    rag, off = dev(rag_h), np.array([0, L, L + long])
    assert torch.equal(E.lowpass(rag, offsets=off)[:, :L], E.lowpass(rect)[0])
    assert torch.equal(E.estimate_noise_std(rag, offsets=off)[0], E.estimate_noise_std(rect)[0])
    got = E.nlm(rag, offsets=off)
    assert torch.equal(got[:, :L], E.nlm(rect)[0]) and torch.isfinite(got).all() and not torch.equal(got[:, L:], rag[:, L:])


def test_out_aliasing_rules(stores):
    rect = dev(stores[0])
    flat = torch.zeros(rect.numel() + 8, device='cuda')
    flat[:rect.numel()] = rect.reshape(-1)
    a, b = flat[:rect.numel()].view(rect.shape), flat[8:].view(rect.shape)
    for fn in (E.lowpass, E.nlm):
        with pytest.raises(ValueError, match='overlaps'):
            fn(a, out=b)
        with pytest.raises(ValueError, match='out'):
            fn(rect, out=torch.zeros(3, 12, L - 1, device='cuda'))
        with pytest.raises(ValueError, match='out'):
            fn(rect, out=torch.zeros(rect.shape, device='cuda', dtype=torch.float64))
        with pytest.raises(ValueError, match='repeats'):
            fn(rect, idxs=[1, 1])


def test_denoiser_is_the_three_stages_in_sequence(stores):
    rect_h, rag_h, off = stores
    rect, rag = dev(rect_h), dev(rag_h)
    d = E.EcgDenoiser()
    want = E.nlm(E.lowpass(rect))
    got = d(rect)
    assert torch.equal(got, want) and torch.equal(d(rect), got) and np.array_equal(rect.cpu().numpy(), rect_h)     # and again: the same bits
    base = dev(0.1 * np.sin(np.arange(L) / 30.0)[None, None, :] * np.ones((3, 12, 1)))
    want_b = E.nlm(E.lowpass(rect) - base)
    assert torch.equal(d(rect, baseline=base), want_b) and not torch.equal(want_b, want)
    sub = d(rect, baseline=base, idxs=[2])
    assert torch.equal(sub[2], want_b[2]) and torch.equal(sub[:2], rect[:2])
    rb = dev(0.1 * np.cos(np.arange(rag.shape[1]) / 25.0)[None, :] * np.ones((12, 1)))
    got = d(rag, baseline=rb, offsets=off, idxs=[1, 5])
    lp = E.lowpass(rag, offsets=off, idxs=[1, 5])
    for i in (1, 5):
        lp[:, off[i]:off[i + 1]] -= rb[:, off[i]:off[i + 1]]
    assert torch.equal(got, E.nlm(lp, offsets=off, idxs=[1, 5]))
    h = d(rect_h, baseline=base.cpu().numpy(), idxs=[2], chunk_records=1)                      # a host store streams through every stage
    assert isinstance(h, np.ndarray) and np.array_equal(h, sub.cpu().numpy())
    d250 = E.EcgDenoiser(fqs=250, search_width=40, patch_width=5)
    assert torch.equal(d250(rect), E.nlm(E.lowpass(rect, fqs=250), search_width=40, patch_width=5))
