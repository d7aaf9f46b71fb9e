"""CPU: the host side of the chirp route of `resample` (Bluestein's algorithm: `chirp=`, `resample_chirp_length`, `resample_route`, the
refusals of `ecgvit_resample_chirp` and `ecgvit_resample_chirp_filter` that need no device, the workspace query) and the numpy restatement
tests/resample_chirp_ref.py that follows include/ecgvit_hip.h step by step, held here to the existing reference tests/resample_ref.py and to
numpy's FFT."""
import importlib

import numpy as np
import pytest

import ecg_representation_learning_amd as E
import resample_chirp_ref as CR
import resample_ref as R

RS = importlib.import_module('ecg_representation_learning_amd.resample')
ALL_PAIRS = CR.CHIRP_PAIRS + [CR.REFUSED_PAIR]


def test_chirp_lengths():
    """M = the smallest 2^a 3^b 5^c >= 2 n - 1, from the library and from the restatement; its plan holds built radices only"""
    want = {7: 15, 13: 25, 14: 27, 63: 125, 257: 540, 4999: 10000, 131101: 262440, 1 << 24: 1 << 25, (1 << 24) + 1: -1, 0: -1, -5: -1, 1: 1, 2: 3}
    for n, M in want.items():
        assert E.resample_chirp_length(n) == M == CR.chirp_length(n), (n, M, E.resample_chirp_length(n), CR.chirp_length(n))
    built = set(RS.BUILT_RADICES)
    rng = np.random.default_rng(3)
    for n in list(want) + rng.integers(1, 1 << 24, 200).tolist():
        M = E.resample_chirp_length(n)
        if M < 0:
            continue
        assert M == CR.chirp_length(n) and 2 * n - 1 <= M <= 1 << 25 and set(E.resample_plan(M)) <= built, (n, M)
        m = M
        for p in (2, 3, 5):
            while m % p == 0:
                m //= p
        assert m == 1, (n, M)


def test_restatement_equals_the_existing_reference():
    """resample_chirp_ref (both transforms on the chirp route wherever route(., 7) sends them) against resample_ref, per element within the
    GPU tests' tolerance after the rounding to f32: 2^-24 |ref| + 1e-8 max |lead| + 1e-12 max |record|.  Measured: at most 0.84 of the tolerance
    (the f32 rounding itself); in f64 at most 5e-15 of max |lead|."""
    rng = np.random.default_rng(4)
    worst = worst64 = 0.0
    for n, num in ALL_PAIRS:
        x = R.record(rng, n, 2) if n <= 5000 else CR.sines(rng, n, 2)
        ref = R.resample_ref(x, num)
        y = CR.resample_chirp_ref(x[0].astype(np.float64) + 1j * x[1].astype(np.float64), num)
        got64 = np.stack([y.real, y.imag])
        got = got64.astype(np.float32).astype(np.float64)
        lead = np.abs(x).max(axis=1, keepdims=True).astype(np.float64)
        tol = 2.0 ** -24 * np.abs(ref) + 1e-8 * lead + 1e-12 * float(lead.max())
        ex = float((np.abs(got - ref) / tol).max())
        e64 = float((np.abs(got64 - ref) / lead).max())
        print(f'{n} -> {num} (routes {CR.route(n, 7)}, {CR.route(num, 7)}): error / tolerance {ex:.3f}; f64 error / max |lead| {e64:.2e}')
        worst, worst64 = max(worst, ex), max(worst64, e64)
        assert ex <= 1.0, (n, num, ex)
    print(f'worst error / tolerance {worst:.3f}; worst f64 error {worst64:.2e}')


def test_chirp_dft_equals_numpy():
    """the restated chirp DFT against np.fft.fft / ifft * n on complex white noise, both signs.  E_chirp = max |X - ref| / max |ref|, measured:
    at most 1.4e-15 over n = 7 .. 131 101; the GPU test's bound 1e-12 must be at least 50 E_chirp (the pattern of test_pairing_identity)."""
    rng = np.random.default_rng(5)
    e_chirp = 0.0
    for n in CR.DFT_LENGTHS:
        z = rng.standard_normal((3, n)) + 1j * rng.standard_normal((3, n))
        for sign, ref in ((-1, np.fft.fft(z, axis=-1)), (1, np.fft.ifft(z, axis=-1) * n)):
            err = float(np.abs(CR.chirp_dft(z, sign) - ref).max()) / float(np.abs(ref).max())
            print(f'n = {n} sign {sign:+d}: E = {err:.3e}')
            e_chirp = max(e_chirp, err)
    print(f'E_chirp = {e_chirp:.3e}')
    assert 50 * e_chirp <= 1e-12, e_chirp


def test_chirp_table_is_the_restatements():
    for n in (7, 14, 257, 131101):
        for sign in (-1, 1):
            t = RS.chirp_table(n, sign)
            w = CR.chirp(n, sign)
            assert t.shape == (n, 2) and t.dtype == np.float64 and t.flags.c_contiguous
            assert np.array_equal(t[:, 0], w.real) and np.array_equal(t[:, 1], w.imag)
    # the 64-bit reduction: at the cap, j^2 is beyond 2^47 and the angle is still that of (j^2 mod 2 n)
    n = 1 << 24
    j = n - 1
    assert abs(RS.chirp_table(n, 1)[j, 0] - np.cos(np.pi * ((j * j) % (2 * n)) / n)) == 0.0


def test_routes():
    assert E.resample_route(257, None) == 'dense' and E.resample_route(257, 300) == 'dense' and E.resample_route(257, 257) == 'chirp'
    assert E.resample_route(5000, 7) == 'plain' and E.resample_route(1028, 7) == 'chirp'
    assert E.resample_route(257) == 'dense' and E.resample_route(462600, 258) == 'dense' and E.resample_route(462600, 257) == 'chirp'
    assert E.resample_route(131101, None) == 'dense' and E.resample_route(131101, True) == 'chirp'
    assert E.resample_route((1 << 24) + 1, 7) != 'chirp'                       # above the cap of the chirp route
    assert RS.CHIRP_DEFAULT >= 7 and E.resample_route(5000, True) == 'plain'
    for n in sorted({n for pair in ALL_PAIRS for n in pair} | {5000, 4096, 462600}):
        for r0 in (None, 7, 20, 257, 300):
            assert E.resample_route(n, r0) == CR.route(n, r0), (n, r0)


def test_refusals_without_a_device():
    for bad in (3, 6, 0, -1, 7.5, 'yes'):
        with pytest.raises(ValueError, match='chirp'):
            E.resample(np.zeros((1, 12, 100), np.float32), 500, chirp=bad)
        with pytest.raises(ValueError, match='chirp'):
            E.resample_route(257, bad)
    with pytest.raises(ValueError, match='prime factor'):
        E.resample(np.zeros((1, 12, 131101), np.float32), 500, num=100, chirp=None)
    with pytest.raises(ValueError, match='prime factor'):
        E.resample(np.zeros((1, 12, 131101), np.float32), 500, num=100)
    # with chirp set the wide prime factor passes the host checks (what then stops a host array here is the missing device, or nothing)
    RS._check_length(131101, 7)
    RS._check_length(131101, True)
    with pytest.raises(ValueError, match='prime factor'):
        RS._check_length(131101, None)
    # above 1 << 24 samples the chirp route is not taken: 2 * 8 388 617 = 16 777 234 keeps its refusal, and the message says where the limit is
    n = 2 * 8388617
    assert E.resample_plan(n) == [2, 8388617] and n > 1 << 24
    with pytest.raises(ValueError, match=r'1 << 24'):
        RS._check_length(n, 7)


def test_launchers_refuse_before_launching():
    """ecgvit_resample_chirp and ecgvit_resample_chirp_filter check their arguments on the host and return ECGVIT_EINVAL without a launch (the
    pointers here are never dereferenced)"""
    lib = E.hip.lib()
    x, out, src, dst, tw_a, tw_b, ws = 0x10000000, 0x20000000, 0x30000000, 0x38000000, 0x40000000, 0x50000000, 0x60000000
    w_a, f_a, w_b, f_b = 0x70000000, 0x78000000, 0x80000000, 0x88000000

    def call(x=x, out=out, src=src, dst=dst, R=2, C=12, n_in=257, n_out=250, tw_a=tw_a, tw_b=tw_b, w_a=w_a, f_a=f_a, w_b=None, f_b=None, ws=ws, s_stride=257):
        return lib.ecgvit_resample_chirp(x, out, src, s_stride, dst, 250, R, C, n_in, n_out, tw_a, tw_b, w_a, f_a, w_b, f_b, ws, None)
    # a null argument
    assert call(x=None) == 1 and call(out=None) == 1 and call(src=None) == 1 and call(dst=None) == 1 and call(ws=None) == 1
    assert call(tw_a=None) == 1 and call(tw_b=None) == 1
    # a misaligned argument
    assert call(x=x + 2) == 1 and call(src=src + 4) == 1 and call(ws=ws + 8) == 1 and call(tw_a=tw_a + 8) == 1 and call(s_stride=0) == 1
    assert call(w_a=w_a + 8) == 1 and call(f_a=f_a + 8) == 1 and call(w_b=w_b + 8, f_b=f_b) == 1 and call(w_b=w_b, f_b=f_b + 8) == 1
    # half of a chirp / filter pair
    assert call(f_a=None) == 1 and call(w_a=None) == 1 and call(w_b=w_b) == 1 and call(f_b=f_b) == 1
    # a chirp side above 1 << 24 samples; a plain side ecgvit_resample refuses; the shapes it refuses
    assert call(n_in=(1 << 24) + 1) == 1 and call(n_out=(1 << 24) + 1, w_b=w_b, f_b=f_b) == 1
    assert call(n_out=131101) == 1 and call(n_in=131101, w_a=None, f_a=None) == 1 and call(n_in=0) == 1
    assert call(C=11) == 1 and call(C=0) == 1 and call(R=0) == 1 and call(R=10923) == 1

    def filt(w=w_a, n=257, M=540, tw=tw_a, f=f_a, ws=ws):
        return lib.ecgvit_resample_chirp_filter(w, n, M, tw, f, ws, None)
    assert filt(w=None) == 1 and filt(tw=None) == 1 and filt(f=None) == 1 and filt(ws=None) == 1
    assert filt(w=w_a + 8) == 1 and filt(tw=tw_a + 8) == 1 and filt(f=f_a + 8) == 1 and filt(ws=ws + 8) == 1
    assert filt(M=512) == 1 and filt(M=541) == 1 and filt(n=0) == 1 and filt(n=(1 << 24) + 1, M=1 << 25) == 1


def test_workspace_query():
    """two buffers of R * 6 * max(side lengths) complex f64, a chirp side counting its M; 0 for what the launcher refuses"""
    q = E.hip.lib().ecgvit_resample_chirp_workspace
    assert q(3, 12, 5000, 2500, 0, 0) == 2 * 16 * 3 * 6 * 5000 == E.hip.lib().ecgvit_resample_workspace(3, 12, 5000, 2500)
    assert q(1, 12, 13, 14, 1, 1) == 2 * 16 * 6 * 27 and q(1, 12, 13, 14, 1, 0) == 2 * 16 * 6 * 25 and q(1, 12, 13, 14, 0, 1) == 2 * 16 * 6 * 27
    assert q(2, 12, 257, 250, 1, 0) == 2 * 16 * 2 * 6 * 540 and q(2, 12, 250, 257, 0, 1) == 2 * 16 * 2 * 6 * 540
    assert q(2, 12, 257, 1000, 1, 0) == 2 * 16 * 2 * 6 * 1000
    assert q(1, 12, 131101, 65550, 1, 0) == 2 * 16 * 6 * 262440 and q(1, 12, 131101, 65550, 0, 0) == 0
    assert q(1, 12, 1 << 24, 100, 1, 0) == 2 * 16 * 6 * (1 << 25) and q(1, 12, (1 << 24) + 1, 100, 1, 0) == 0
    assert q(1, 12, 100, (1 << 24) + 1, 0, 1) == 0 and q(1, 12, 0, 100, 1, 0) == 0
    assert q(3, 11, 257, 250, 1, 0) == 0 and q(0, 12, 257, 250, 1, 0) == 0 and q(10923, 12, 257, 250, 1, 0) == 0
    # the existing contracts stay: the plain query and the plan know nothing of the chirp route
    assert E.hip.lib().ecgvit_resample_workspace(1, 12, 131101, 100) == 0 and E.resample_plan(131101) == [131101]


def test_chirp_kernels_have_no_spills_or_scratch():
    """tools/code_objects.py over the shipped library: the chirp route's element-wise kernels keep everything in registers"""
    import os
    import sys
    from conftest import ROOT
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import code_objects
    if not os.path.exists(code_objects.READELF):
        pytest.skip('llvm-readelf not in this image')
    ks = {n: k for n, k in code_objects.kernels(E.hip.LIB_PATH).items() if 'rs_' in n and ('chirp' in n or 'rs_scale' in n)}
    assert len(ks) == 6, sorted(ks)
    for name, k in ks.items():
        assert k['vgpr_spill_count'] == 0 and k['private_segment_fixed_size'] == 0 and k['vgpr_count'] <= 32, (name, k)
