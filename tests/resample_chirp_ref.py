"""numpy f64 restatement of the chirp route of include/ecgvit_hip.h (Bluestein's algorithm), step by step as the header states it: the chirp
w, the length M, the operand a, the filter b and its spectrum, c = conj(DFT_M(conj(DFT_M(a) filter))), X = w c.  numpy's FFT stands in for the
passes of the smooth length M only; the length n itself is never handed to it.  `resample_chirp_ref` is the complex-input resample of
tests/resample_ref.py with either transform on that route.  CHIRP_PAIRS: the (n_in, n_out) of the chirp tests."""
import numpy as np

MAX_CHIRP = 1 << 24
BUILT = (25, 16, 8, 5, 4, 3, 2)


def chirp_length(n):
    """the smallest 2^a 3^b 5^c >= 2 n - 1; -1 for n < 1 or n > 1 << 24"""
    if n < 1 or n > MAX_CHIRP:
        return -1
    need, best = 2 * n - 1, 1 << 25
    p5 = 1
    while p5 <= best:
        p3 = p5
        while p3 <= best:
            m = p3
            while m < need:
                m *= 2
            best = min(best, m)
            p3 *= 3
        p5 *= 5
    return best


def chirp(n, sign):
    """w[j] = exp(sign i pi j^2 / n) as cos / sin(pi ((j j) mod 2 n) / n), the square and the reduction in 64-bit integers"""
    j = np.arange(n, dtype=np.int64)
    ang = np.pi * ((j * j) % (2 * n)).astype(np.float64) / n
    return np.cos(ang) + 1j * sign * np.sin(ang)


def chirp_filter(w, M):
    """DFT_M(b) / M, b[j] = conj(w[j]), j < n; b[M - j] = conj(w[j]), 1 <= j < n; 0 elsewhere"""
    n = len(w)
    b = np.zeros(M, np.complex128)
    b[:n] = np.conj(w)
    if n > 1:
        b[M - np.arange(1, n)] = np.conj(w[1:])
    return np.fft.fft(b) / M


def chirp_dft(z, sign):
    """X[k] = sum_j z[j] exp(sign 2 pi i j k / n) over the last axis, by the chirp route"""
    z = np.asarray(z, np.complex128)
    n = z.shape[-1]
    M = chirp_length(n)
    w = chirp(n, sign)
    a = np.zeros(z.shape[:-1] + (M,), np.complex128)
    a[..., :n] = z * w
    c = np.conj(np.fft.fft(np.conj(np.fft.fft(a, axis=-1) * chirp_filter(w, M)), axis=-1))
    return w * c[..., :n]


def generic_radices(n):
    """the prime factors of n outside the built radices (the generic passes of its plan)"""
    for r in BUILT:
        while n % r == 0:
            n //= r
    out, p = [], 7
    while n > 1:
        if p * p > n:
            p = n
        while n % p == 0:
            out.append(p)
            n //= p
        p += 2
    return out


def route(n, r0):
    g = generic_radices(n)
    if not g:
        return 'plain'
    return 'chirp' if r0 is not None and max(g) >= r0 and n <= MAX_CHIRP else 'dense'


def resample_chirp_ref(z, num, r0=7):
    """resample_ref_complex with the transforms of the lengths that route(., r0) sends there done by the chirp route"""
    z = np.asarray(z, np.complex128)
    n = z.shape[-1]
    X = chirp_dft(z, -1) if route(n, r0) == 'chirp' else np.fft.fft(z, axis=-1)
    N = min(n, num)
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
    Y /= n
    return chirp_dft(Y, 1) if route(num, r0) == 'chirp' else np.fft.ifft(Y, axis=-1) * num


# 7: the smallest admissible length; 13, 14, 63: M = 2 n - 1 exactly (25, 27, 125); chirp on the input side only (257 -> 250, 251 -> 125,
# 1028 -> 1000), the output side only (250 -> 257), both (7 -> 21, 13 -> 14, 63 -> 13, 4999 -> 2499); 1028 = 4 257: a composite with one wide
# factor; 2499 = 3 7 7 17: several
CHIRP_PAIRS = [(7, 21), (13, 14), (63, 13), (257, 250), (250, 257), (251, 125), (1028, 1000), (4999, 2499)]
REFUSED_PAIR = (131101, 65550)          # 131 101 is a prime above 65 536: refused without chirp=; 65 550 = 2 3 25 19 23
DFT_LENGTHS = [7, 13, 14, 63, 257, 4999, 131101]


def sines(rng, n, C=12, fs=257):
    """sines and noise, the record of the long-record test (tests/test_gpu_resample.py)"""
    t = np.arange(n, dtype=np.float64)
    return np.stack([np.sin(2 * np.pi * t * rng.uniform(0.5, 40) / fs + c) * rng.uniform(0.5, 2) + rng.normal(0, 0.05, n) for c in range(C)]).astype(np.float32)
