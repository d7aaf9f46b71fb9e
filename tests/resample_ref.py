"""numpy f64 restatement of `scipy.signal.resample(x, num)` (Fourier resampling, no window), which is what the reference's
`wfdb.processing.resample_sig` computes per lead (preprocess/data_export.py:202-215).  `resample_ref` is scipy's real-input rule;
`resample_ref_complex` is its complex-input rule, the one the kernels apply to a pair of leads.  PAIRS: the (n_in, n_out) of the tests."""
import numpy as np


def resample_ref(x, num):
    x = np.asarray(x, np.float64)
    n = x.shape[-1]
    X, N = np.fft.rfft(x, axis=-1), min(n, num)
    Y = np.zeros(x.shape[:-1] + (num // 2 + 1,), np.complex128)
    Y[..., :N // 2 + 1] = X[..., :N // 2 + 1]
    if N % 2 == 0 and num != n:
        Y[..., N // 2] *= 2.0 if num < n else 0.5     # real input: the bin at -N/2 is the conjugate of the one at N/2
    return np.fft.irfft(Y, num, axis=-1) * (float(num) / n)


def resample_ref_complex(z, num):
    z = np.asarray(z, np.complex128)
    n = z.shape[-1]
    X, N = np.fft.fft(z, axis=-1), min(n, num)
    Y = np.zeros(z.shape[:-1] + (num,), np.complex128)
    nneg = N - (N // 2 + 1)
    Y[..., :N // 2 + 1] = X[..., :N // 2 + 1]
    if nneg:
        Y[..., num - nneg:] = X[..., n - nneg:]
    if N % 2 == 0 and num < n:
        Y[..., N // 2] += X[..., n - N // 2]
    elif N % 2 == 0 and n < num:
        Y[..., N // 2] *= 0.5
        Y[..., num - N // 2] = Y[..., N // 2]
    return np.fft.ifft(Y, axis=-1) * (float(num) / n)


# every built radix (25, 16, 8, 5, 4, 3, 2) as a whole transform and at a later position of a plan (9 = 3 3, 64 = 16 4, 128 = 16 8, 250 = 25 5 2,
# 256 = 16 16, 625 = 25 25): a chain, each length once forward and once inverse
RADIX_PAIRS = [(2, 3), (3, 4), (4, 5), (5, 8), (8, 16), (16, 25), (25, 9), (9, 64), (64, 256), (256, 625), (625, 128), (128, 250)]
GENERIC_PAIRS = [(7, 21), (257, 250), (250, 257), (251, 125)]             # 7, 257, 251 as a dense pass; 7 as a factor of 21 (1028 = 4 257 below)
NYQUIST_PAIRS = [(30, 20), (20, 30), (31, 17), (17, 31), (32, 16), (16, 32), (1000, 999), (999, 1000)]   # N even / odd, down / up
DEGENERATE_PAIRS = [(1, 2), (2, 1), (3, 2)]
CORPUS_PAIRS = [(5000, 2500), (4096, 2560), (1028, 1000), (4999, 2499)]    # 4999 is prime: the dense pass at its largest here
LONG_PAIR = (462600, 450000)                                             # INCART's 30 minutes at 257 Hz: 462 600 = 25 8 3 3 257
PAIRS = RADIX_PAIRS + GENERIC_PAIRS + NYQUIST_PAIRS + DEGENERATE_PAIRS + CORPUS_PAIRS


def record(rng, n, C=12):
    """12 leads of beats, sway and noise, as the denoiser's fixture draws them"""
    t = np.arange(n, dtype=np.float64)
    out = np.empty((C, n), np.float32)
    for c in range(C):
        beats = sum(np.exp(-0.5 * ((t - t0) / 2.5) ** 2) for t0 in np.arange(rng.uniform(0, 41), n + 41, 41))
        sway = 0.2 * np.sin(2 * np.pi * t / rng.uniform(150, 400) + rng.uniform(0, 6))
        out[c] = (rng.uniform(0.5, 1.5) * beats + sway + rng.normal(0, 0.05, n)).astype(np.float32)
    return out
