"""numpy restatement of the three stages of the Zheng et al. denoiser (reference preprocess/data_preprocessor.py:48-148), each with a `dtype`.

float64: the reference's arithmetic in another order -- what tests/test_denoise.py holds to the fixture the reference itself wrote
(tests/golden/denoise.npz).  float32 (`nlm` only): the arithmetic of csrc/denoise.hip -- patch distances summed directly from their 2p + 1 terms
at the start of each run of RUN output samples and slid within the run, f32 exp2, shifts added in ascending order -- which prices the kernel's
tolerance without the kernel.  One lead (1-D) per call."""
import math

import numpy as np

RUN = 15            # output samples per lane run in csrc/denoise.hip (NLM_RUN)
EPS = 2.220446049250313e-16


def lfilter(b, a, x, z):
    """direct form II transposed, scipy's order of operations; -> y (z is consumed)"""
    nt, y, z = len(b), np.empty_like(x), z.copy()
    for i, xi in enumerate(x):
        yi = z[0] + b[0] * xi
        for k in range(nt - 2):
            z[k] = z[k + 1] + xi * b[k + 1] - yi * a[k + 1]
        z[nt - 2] = xi * b[nt - 1] - yi * a[nt - 1]
        y[i] = yi
    return y


def filtfilt(b, a, zi, x, dtype=np.float64):
    """scipy.signal.filtfilt(b, a, x) with its defaults: odd extension by 3 * ntaps, forward, backward"""
    b, a, zi, x = (np.asarray(v, dtype) for v in (b, a, zi, x))
    pad = 3 * max(len(a), len(b))
    if len(x) <= pad:
        raise ValueError(f'The length of the input vector x must be greater than padlen, which is {pad}.')
    ext = np.concatenate([2 * x[0] - x[pad:0:-1], x, 2 * x[-1] - x[-2:-pad - 2:-1]])
    y = lfilter(b, a, ext, zi * ext[0])
    y = lfilter(b, a, y[::-1], zi * y[-1])
    return y[::-1][pad:-pad]


def est_noise_std(x, dtype=np.float64):
    res = np.array(x, dtype)
    s6 = dtype(math.sqrt(6))
    for i in range(1, len(res) - 1):
        res[i] = (2 * res[i] - res[i - 1] - res[i + 1]) / s6
    y = dtype(1.4826) * (res - np.median(res))
    return np.median(np.abs(y - np.median(y)))          # scipy.stats.median_abs_deviation


def n_runs(n, p, run=RUN):
    return max(0, -(-(n - 2 * p - 1) // run))


def nlm(x, sigma, scale=1.5, p=10, sch_wd=None, dtype=np.float64, run=RUN, runs=None):
    """DataPreprocessor.nlm.  A lead with n <= 2p + 1 or sigma == 0 comes back unchanged.  runs: the run indices to evaluate (the other
    samples keep their input value); None: all.  Run k stores samples p + 1 + k run ...; the last run ends on sample n - p - 1."""
    x = np.asarray(x, dtype)
    n, out = len(x), np.array(x, dtype)
    M = n - 2 * p - 1
    if M <= 0 or sigma == 0:
        return out
    W = n if sch_wd is None or sch_wd > n else sch_wd
    h = 2.0 * (2 * p + 1) * (scale * float(sigma)) ** 2
    f32 = dtype == np.float32
    cexp = np.float32(-1.4426950408889634 / h)
    K, ln = n_runs(n, p, run), min(M, run)
    t0_all = np.arange(2 - ln, n)
    j = np.arange(ln + 2 * p)
    for k in (range(K) if runs is None else runs):
        first = p + 1 + k * run
        a = n - p - ln if k == K - 1 else first
        t0 = t0_all[np.abs(t0_all - a) <= W - 1]
        ni = t0[:, None] - p + j[None, :]
        df = x[a - p + j][None, :] - x[np.clip(ni, 0, n - 1)]
        e = np.where((ni >= 0) & (ni < n), df * df, dtype(0))
        d = e[:, 0].copy()
        for jj in range(1, 2 * p + 1):
            d = d + e[:, jj]
        for r in range(ln):
            t = t0 + r
            w = np.exp2(d * cexp) if f32 else np.exp(-d / h)
            w = np.where((t > 0) & (t < n), w, dtype(0))
            num = np.cumsum(w * x[np.clip(t, 0, n - 1)], dtype=dtype)[-1]     # cumsum adds in sequence: ascending shifts
            den = np.cumsum(w, dtype=dtype)[-1]
            if a + r >= first:
                out[a + r] = num / (den + dtype(EPS))
            if r + 1 < ln:
                d = (d + e[:, r + 2 * p + 1]) - e[:, r]
    return out


def run_samples(n, p, runs, run=RUN):
    """the sample indices the given runs store"""
    K, ln = n_runs(n, p, run), min(n - 2 * p - 1, run)
    idx = []
    for k in runs:
        first = p + 1 + k * run
        idx += list(range(first, n - p if k == K - 1 else first + ln))
    return np.array(idx)
