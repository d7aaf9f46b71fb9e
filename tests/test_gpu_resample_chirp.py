"""GPU: the chirp route of csrc/resample.hip (Bluestein's algorithm; include/ecgvit_hip.h states it) through `resample(..., chirp=)`,
`ecgvit_resample_chirp` and the tools library's `ecgvit_tools_resample_chirp`, against the numpy f64 restatement of `scipy.signal.resample`
(tests/resample_ref.py) and numpy's FFT.

Tolerance against the restatement, per element: the one tests/test_gpu_resample.py derives, |out - ref64| <= 2^-24 |ref64| + 1e-8 max |lead| +
1e-12 max |record|.  The chirp route's own f64 error (tests/test_resample_chirp.py: at most 5e-15 of max |lead| in numpy) is six orders of
magnitude below the second term, so the chirp route gets no term of its own.
The tools entry returns the chirp DFT in complex f64, before the f32 store hides it: max |X - ref| <= 1e-12 max |ref| against np.fft.fft /
ifft * n, the project's 1e-12 term (the restatement measures about 1e-15; the passes use other radices than numpy's FFT).

MEASURED on the MI355X, the largest |out - ref64| as a fraction of the tolerance (the f32 store's rounding alone reaches 0.5 to 1.0 of the first
term): chirp pairs at chirp=7 0.821 (7 -> 21: 0.815, 13 -> 14: 0.760, 63 -> 13: 0.683, 257 -> 250: 0.782, 250 -> 257: 0.821, 251 -> 125: 0.817,
1028 -> 1000: 0.809, 4999 -> 2499: 0.798); 131 101 -> 65 550 at chirp=True: 0.834 (chirp in; 65 550 = 2 3 25 19 23 stays dense below
CHIRP_DEFAULT = 61; with both sides on the chirp route the same 0.834); 257 -> 250 at chirp=257: 0.781 (and, as it happens, the dense route's
bits after the f32 rounding: not asserted).  Pair independence, lead 1 at 1e-3 beside lead 0 at 1e3: 0.028 (257 -> 250), 0.060 (250 -> 257)
of its tolerance; the swapped pairs 0.68 and 0.75 of theirs.  The tools entry: see test_tools_chirp_dft_in_f64.
"""
import importlib

import numpy as np
import pytest
import torch

import ecg_representation_learning_amd as E
import resample_chirp_ref as CR
import resample_ref as R
from hiputil import tools_lib

pytestmark = pytest.mark.gpu
RS = importlib.import_module('ecg_representation_learning_amd.resample')    # (the package's `resample` is the function)


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x, np.float32)).cuda()


def excess(got, x, num):
    """got, x: (12, num), (12, n) -> the largest |got - ref64| / tolerance over the record (at most 1 passes)"""
    ref = R.resample_ref(x, num)
    lead = np.abs(x).max(axis=1, keepdims=True).astype(np.float64)
    tol = 2.0 ** -24 * np.abs(ref) + 1e-8 * lead + 1e-12 * float(lead.max())
    assert got.shape == ref.shape and got.dtype == np.float32
    return float((np.abs(got.astype(np.float64) - ref) / tol).max())


def test_chirp_pairs():
    """CHIRP_PAIRS at chirp=7, 2 records x 12 leads each: 7 is the smallest admissible length; 13, 14 and 63 have M = 2 n - 1 exactly, where an
    off-by-one in the wrapped filter entries shows; chirp on the input side only, the output side only and both; 1028 = 4 257, a composite with
    one wide factor; 2499 = 3 7 7 17 with several"""
    rng = np.random.default_rng(31)
    worst = 0.0
    sides = set()
    for n, num in CR.CHIRP_PAIRS:
        routes = (E.resample_route(n, 7), E.resample_route(num, 7))
        assert 'chirp' in routes
        sides.add(tuple(r == 'chirp' for r in routes))
        x = np.stack([R.record(rng, n), R.record(rng, n)])
        got = E.resample(dev(x), 500, num=num, chirp=7)
        assert got.shape == (2, 12, num) and got.is_cuda
        got = got.cpu().numpy()
        ex = max(excess(got[0], x[0], num), excess(got[1], x[1], num))
        print(f'{n} -> {num} (routes {routes}, M {E.resample_chirp_length(n)}, {E.resample_chirp_length(num)}): error / tolerance {ex:.3f}')
        worst = max(worst, ex)
        assert ex <= 1.0, (n, num, ex)
    assert sides == {(True, False), (False, True), (True, True)}
    print(f'chirp pairs: worst error / tolerance {worst:.3f}')


def test_the_previously_refused_length():
    """131 101 (a prime above 65 536) -> 65 550 at chirp=True: one record of sines and noise, as the long-record test draws it.  Without chirp=
    the length is refused."""
    n, num = CR.REFUSED_PAIR
    x = CR.sines(np.random.default_rng(11), n)
    with pytest.raises(ValueError, match='prime factor'):
        E.resample(dev(x[None]), 500, num=num)
    assert E.resample_route(n, True) == 'chirp'
    got = E.resample(dev(x[None]), 500, num=num, chirp=True)
    assert got.shape == (1, 12, num)
    ex = excess(got[0].cpu().numpy(), x, num)
    print(f'{n} -> {num} (routes chirp, {E.resample_route(num, True)}): error / tolerance {ex:.3f}')
    assert ex <= 1.0, ex


def test_todays_bits_are_kept():
    """a length below r0 runs today's passes, bit for bit; at r0 = 257 the length 257 changes route and keeps the tolerance"""
    rng = np.random.default_rng(37)
    x = np.stack([R.record(rng, 5000), R.record(rng, 5000)])
    assert torch.equal(E.resample(dev(x), 500, num=2500, chirp=7), E.resample(dev(x), 500, num=2500))
    x = np.stack([R.record(rng, 257), R.record(rng, 257)])
    plain = E.resample(dev(x), 500, num=250)
    assert torch.equal(E.resample(dev(x), 500, num=250, chirp=300), plain)
    got = E.resample(dev(x), 500, num=250, chirp=257).cpu().numpy()
    ex = max(excess(got[0], x[0], 250), excess(got[1], x[1], 250))
    print(f'257 -> 250 at chirp=257: error / tolerance {ex:.3f}; bit-equal to the dense route: {np.array_equal(got, plain.cpu().numpy())}')
    assert ex <= 1.0, ex


def test_store_forms_are_bit_identical():
    """a ragged store at 500 -> 250 with chirp=7 (40 -> 20 and 96 -> 48 plain, 31 -> 15 and 257 -> 128 chirp in, 14 -> 7 chirp on both sides),
    against the same records as rectangles one by one: the whole store, a subset with a repeat, a host array one record per chunk, a workspace of
    exactly one record's chirp need; one byte less raises and names the need"""
    rng = np.random.default_rng(41)
    lens = [40, 31, 14, 257, 96, 40, 14]
    recs = [R.record(rng, n) for n in lens]
    rag = np.concatenate(recs, axis=1)
    off = np.concatenate([[0], np.cumsum(lens)])
    want = [E.resample(dev(r[None]), 500, 250, chirp=7)[0].cpu().numpy() for r in recs]
    for r, w in zip(recs, want):
        assert excess(w, r, w.shape[1]) <= 1.0

    def check(res, ids):
        out, noff = res
        out = out.cpu().numpy() if isinstance(out, torch.Tensor) else out
        assert noff.tolist() == np.concatenate([[0], np.cumsum([want[i].shape[1] for i in ids])]).tolist() and out.shape == (12, noff[-1])
        for k, i in enumerate(ids):
            assert np.array_equal(out[:, noff[k]:noff[k + 1]], want[i]), (k, i)
    check(E.resample(dev(rag), 500, 250, offsets=off, chirp=7), range(7))
    check(E.resample(dev(rag), 500, 250, offsets=off, idxs=[3, 2, 3, 6, 1], chirp=7), [3, 2, 3, 6, 1])
    host = E.resample(rag.astype(np.float64), 500, 250, offsets=off, chunk_records=1, chirp=7)
    assert isinstance(host[0], np.ndarray) and host[0].dtype == np.float32
    check(host, range(7))
    # 257 -> 128 is the largest need of the store: M = 540 on the input side
    need = E.hip.lib().ecgvit_resample_chirp_workspace(1, 12, 257, 128, 1, 0)
    assert need == 2 * 16 * 6 * 540
    check(E.resample(dev(rag), 500, 250, offsets=off, workspace_bytes=need, chirp=7), range(7))
    with pytest.raises(ValueError, match=str(need)):
        E.resample(dev(rag), 500, 250, offsets=off, workspace_bytes=need - 1, chirp=7)
    need14 = E.hip.lib().ecgvit_resample_chirp_workspace(1, 12, 14, 7, 1, 1)
    check(E.resample(dev(rag), 500, 250, offsets=off, idxs=[2, 6, 2], workspace_bytes=need14, chirp=7), [2, 6, 2])


def test_pair_independence():
    """the setup of test_gpu_resample.py's test_pair_independence on the chirp route: lead 0 at 1e3 beside lead 1 at 1e-3 in one complex
    transform; lead 1 keeps its tolerance, and so do the swapped pairs"""
    rng = np.random.default_rng(13)
    worst = 0.0
    for n, num in [(257, 250), (250, 257)]:
        x = R.record(rng, n)
        x[0] *= np.float32(1e3)
        x[1] *= np.float32(1e-3)
        got = E.resample(dev(x[None]), 500, num=num, chirp=7)[0].cpu().numpy()
        ref = R.resample_ref(x, num)
        tol1 = 2.0 ** -24 * np.abs(ref[1]) + 1e-8 * float(np.abs(x[1]).max()) + 1e-12 * float(np.abs(x).max())
        ex1 = float((np.abs(got[1].astype(np.float64) - ref[1]) / tol1).max())
        swapped = x.reshape(6, 2, n)[:, ::-1].reshape(12, n)
        got_s = E.resample(dev(swapped[None]), 500, num=num, chirp=7)[0].cpu().numpy()
        ex_s = excess(got_s, swapped, num)
        print(f'{n} -> {num}: lead 1 beside a 1e6 times larger partner: error / tolerance {ex1:.3f}; swapped {ex_s:.3f}')
        worst = max(worst, ex1, excess(got, x, num), ex_s)
    assert worst <= 1.0, worst


def test_tools_chirp_dft_in_f64():
    """ecgvit_tools_resample_chirp, T = 3 complex f64 sequences of white noise, both signs, against np.fft.fft / ifft * n:
    max |X - ref| <= 1e-12 max |ref|.
    MEASURED on the MI355X, max |X - ref| / max |ref| (sign -1, +1): n = 7: 1.1e-15, 9.0e-16; 13: 1.1e-15, 7.7e-16; 14: 1.2e-15, 8.5e-16;
    63: 7.8e-16, 6.4e-16; 257: 1.9e-15, 1.8e-15; 4 999: 1.5e-15, 1.3e-15; 131 101: 1.7e-15, 2.6e-15.  The largest ratio to the bound: 2.6e-3."""
    lib = E.hip.lib()
    rng = np.random.default_rng(43)
    worst, tools = 0.0, tools_lib()
    for n in CR.DFT_LENGTHS:
        M = E.resample_chirp_length(n)
        z = rng.standard_normal((3, n)) + 1j * rng.standard_normal((3, n))
        zd = torch.from_numpy(z).cuda()
        tw = torch.from_numpy(RS.twiddles(M, -1)).cuda()
        ws = torch.empty((2 * 3 * M, 2), dtype=torch.float64, device='cuda')
        for sign, ref in ((-1, np.fft.fft(z, axis=-1)), (1, np.fft.ifft(z, axis=-1) * n)):
            w = torch.from_numpy(RS.chirp_table(n, sign)).cuda()
            filt = torch.empty((M, 2), dtype=torch.float64, device='cuda')
            E.hip.check(lib.ecgvit_resample_chirp_filter(w.data_ptr(), n, M, tw.data_ptr(), filt.data_ptr(), ws.data_ptr(), None), 'filter')
            ws.fill_(float('nan'))
            out = torch.full((3, n), complex('nan'), dtype=torch.complex128, device='cuda')
            rc = tools.ecgvit_tools_resample_chirp(zd.data_ptr(), out.data_ptr(), w.data_ptr(), filt.data_ptr(), tw.data_ptr(), n, M, 3, ws.data_ptr(), None)
            assert rc == 0, rc
            err = float(np.abs(out.cpu().numpy() - ref).max()) / float(np.abs(ref).max())
            print(f'n = {n} (M = {M}) sign {sign:+d}: max |X - ref| / max |ref| = {err:.3e}')
            worst = max(worst, err)
            assert err <= 1e-12, (n, sign, err)
    print(f'tools chirp DFT: worst {worst:.3e}')


@pytest.mark.parametrize('fill', [float('nan'), 1e300])
def test_workspace_content_is_never_assumed(fill):
    """ecgvit_resample_chirp through ctypes on 13 -> 14 (both sides on the chirp route, M = 25 and 27) with the workspace pre-filled: the same
    bits as resample(..., chirp=7)"""
    lib = E.hip.lib()
    rng = np.random.default_rng(47)
    n, num, Rn = 13, 14, 2
    x = dev(np.stack([R.record(rng, n), R.record(rng, n)]))
    want = E.resample(x, 500, num=num, chirp=7)
    tables = {}
    tw_in, w_in, f_in = RS._side_tables(n, -1, True, tables, x.device)
    tw_out, w_out, f_out = RS._side_tables(num, 1, True, tables, x.device)
    need = lib.ecgvit_resample_chirp_workspace(Rn, 12, n, num, 1, 1)
    assert need == 2 * 16 * Rn * 6 * 27
    ws = torch.full((need // 8,), fill, dtype=torch.float64, device='cuda')
    out = torch.full((Rn, 12, num), float('nan'), device='cuda')
    src = torch.arange(Rn, device='cuda', dtype=torch.int64) * (12 * n)
    dst = torch.arange(Rn, device='cuda', dtype=torch.int64) * (12 * num)
    E.hip.check(lib.ecgvit_resample_chirp(x.data_ptr(), out.data_ptr(), src.data_ptr(), n, dst.data_ptr(), num, Rn, 12, n, num, tw_in.data_ptr(),
                                          tw_out.data_ptr(), w_in.data_ptr(), f_in.data_ptr(), w_out.data_ptr(), f_out.data_ptr(), ws.data_ptr(),
                                          E.hip.stream()), 'ecgvit_resample_chirp')
    assert bool(torch.isfinite(out).all()) and torch.equal(out, want)
