"""The robust LOESS baseline (include/ecgvit_hip.h, `ecgvit_rloess`) restated in numpy f64, twice.

`loess_literal` transcribes the algorithm line by line, in the form of the `loess` package's `loess_1d(x, y, degree, npoints)[1]` the reference
calls (the package is not available: parity with it is unpinned): the `npoints` nearest samples by `np.argsort` of the distances, a least-squares
polynomial through `np.linalg.lstsq` on the sqrt(w)-scaled Vandermonde matrix of the raw abscissae, `np.median`.
`loess_fast` does the same through contiguous windows and the normal equations in the centred, scaled abscissa, every sample at once, with the
kernel's operations in the kernel's order (csrc/denoise.hip): what the GPU tests call at real widths.
Both return (fit, iters, margin): the baseline, the robust iterations run at each sample, and the smallest |bw - 0.34| over every outlier
decision taken (how far the stop rule was from going the other way).
"""
import numpy as np

CUT = 0.34          # a robust weight below this marks an outlier


def force_odd(x):
    return 2 * int(np.floor(x / 2)) + 1


def frac_points(n, frac):
    """the reference's `rloess` for a float `n`: force_odd(int(sig.size * n) - 1)"""
    return force_odd(int(n * float(frac)) - 1)


def _polyfit(x, y, degree, w):
    sq = np.sqrt(w)
    a = x[:, None] ** np.arange(degree + 1)
    coeff = np.linalg.lstsq(a * sq[:, None], y * sq, rcond=None)[0]
    return a @ coeff


def loess_literal(y, npoints, degree=2, robust_iters=10, kind='stable'):
    y = np.asarray(y, np.float64)
    n = len(y)
    x = np.arange(n, dtype=np.float64)
    fit, iters, margin = np.empty(n), np.zeros(n, np.int64), np.inf
    for j in range(n):
        dist = np.abs(x - x[j])
        w = np.argsort(dist, kind=kind)[:npoints]
        d = dist[w].max()
        dw = (1 - (dist[w] / d) ** 3) ** 3
        yfit = _polyfit(x[w], y[w], degree, dw)
        bad = None
        for _ in range(robust_iters):
            aerr = np.abs(yfit - y[w])
            mad = np.median(aerr)
            if mad == 0:                     # the reference divides by zero here; the distance-weighted (or last) fit stands
                break
            bw = (1 - np.clip((aerr / (6 * mad)) ** 2, 0, 1)) ** 2
            yfit = _polyfit(x[w], y[w], degree, dw * bw)
            iters[j] += 1
            margin = min(margin, np.abs(bw - CUT).min())
            old, bad = bad, bw < CUT
            if old is not None and np.array_equal(old, bad):
                break
        fit[j] = yfit[0]                     # the nearest sample is j itself
    return fit, iters, margin


def windows(n, npoints):
    """-> (m, lo, d): window width, first sample and largest distance per sample (the even tie goes to the lower index)"""
    m = min(int(npoints), n)
    j = np.arange(n)
    lo = np.clip(j - (m - 1) // 2 if m & 1 else j - m // 2, 0, n - m)
    return m, lo, np.maximum(j - lo, lo + m - 1 - j)


def _wave_sum(a):
    """row sums in the kernel's order: window sample l + 64 v sits in slot v of lane l; a lane adds its slots in ascending order from +0, the
    wave adds lanes by the xor butterfly 32, 16, .. 1 (a slot past the window adds +0)"""
    rows, m = a.shape
    nv = -(-m // 64)
    p = np.zeros((rows, nv * 64))
    p[:, :m] = a
    p = p.reshape(rows, nv, 64)
    acc = 0.0 + p[:, 0, :]
    for v in range(1, nv):
        acc = acc + p[:, v, :]
    for o in (32, 16, 8, 4, 2, 1):
        acc = acc[:, :o] + acc[:, o:2 * o]
    return acc[:, 0]


def _fit(s, y, w, degree):
    """weighted least squares in the scaled abscissa: moment sums, then the normal equations by elimination without pivoting, operation for
    operation as csrc/denoise.hip (which compiles without contraction into fma) -> a0, a1, a2"""
    w1 = w * s
    w2 = w1 * s
    S0, S1, S2, T0, T1 = _wave_sum(w), _wave_sum(w1), _wave_sum(w2), _wave_sum(w * y), _wave_sum(w1 * y)
    r0 = 1.0 / S0
    l1 = S1 * r0
    A11, B1 = S2 - l1 * S1, T1 - l1 * T0
    if degree == 2:
        w3 = w2 * s
        w4 = w3 * s
        S3, S4, T2 = _wave_sum(w3), _wave_sum(w4), _wave_sum(w2 * y)
        l2 = S2 * r0
        A12, A22, B2 = S3 - l1 * S2, S4 - l2 * S2, T2 - l2 * T0
        r1 = 1.0 / A11
        l21 = A12 * r1
        D22, E2 = A22 - l21 * A12, B2 - l21 * B1
        a2 = E2 / D22
        a1 = (B1 - A12 * a2) * r1
        a0 = ((T0 - S1 * a1) - S2 * a2) * r0
    else:
        a2 = np.zeros_like(S0)
        a1 = B1 / A11
        a0 = (T0 - S1 * a1) * r0
    return a0, a1, a2


def _eval(a0, a1, a2, s):
    return a0[:, None] + s * (a1[:, None] + s * a2[:, None])


TINY = np.finfo(np.float64).tiny      # a median below the smallest normal f64 counts as 0 in the kernel


def loess_fast(y, npoints, degree=2, robust_iters=10, return_mad=False):
    y = np.asarray(y, np.float64)
    n = len(y)
    m, lo, d = windows(n, npoints)
    j = np.arange(n)
    idx = lo[:, None] + np.arange(m)[None, :]
    s = (idx - j[:, None]).astype(np.float64) * (1.0 / d.astype(np.float64))[:, None]
    a = np.abs(s)
    u = 1.0 - a * a * a
    dw = u * u * u
    yw = y[idx]
    a0, a1, a2 = _fit(s, yw, dw, degree)
    yfit = _eval(a0, a1, a2, s)
    fit, iters, margin, min_mad = a0.copy(), np.zeros(n, np.int64), np.inf, np.inf
    live = np.arange(n)                      # the samples whose robust loop still runs
    bad = np.zeros((n, m), bool)
    for it in range(robust_iters):
        aerr = np.abs(yfit - yw[live])
        mad = np.median(aerr, axis=1)
        min_mad = min(min_mad, mad.min())
        keep = mad >= TINY
        live, aerr, mad = live[keep], aerr[keep], mad[keep]
        if not len(live):
            break
        q = aerr * (1.0 / (6.0 * mad))[:, None]
        u = 1.0 - np.minimum(q * q, 1.0)
        bw = u * u
        a0, a1, a2 = _fit(s[live], yw[live], dw[live] * bw, degree)
        yfit = _eval(a0, a1, a2, s[live])
        fit[live] = a0
        iters[live] += 1
        margin = min(margin, np.abs(bw - CUT).min())
        now = bw < CUT
        go = (now != bad[live]).any(axis=1) if it else np.ones(len(live), bool)
        bad[live] = now
        live, yfit = live[go], yfit[go]
        if not len(live):
            break
    return (fit, iters, margin, min_mad) if return_mad else (fit, iters, margin)


def signal(seed, n, leads=12, amp=1.0, scaled=False):
    """a seeded test store (leads, n) float32: a smooth wave, Gaussian noise and sparse large spikes, so that the outlier set of a window is
    non-empty and changes between robust iterations.  scaled: lead c is lead 0 times 2^(c - 6): every operation rounds as it does for lead 0, so
    the leads share their decisions (what the exactly determined windows of the shortest records need: see tests/test_loess.py)"""
    if scaled:
        one = signal(seed, n, 1, amp)[0]
        return np.stack([np.ldexp(one, c - 6) for c in range(leads)]).astype(np.float32)
    rng = np.random.default_rng(seed)
    t = np.arange(n, dtype=np.float64)
    out = np.empty((leads, n), np.float32)
    for c in range(leads):
        wave = np.sin(2 * np.pi * t / rng.uniform(90, 400) + rng.uniform(0, 6)) + 0.3 * np.sin(2 * np.pi * t / rng.uniform(25, 60) + rng.uniform(0, 6))
        spikes = np.where(rng.random(n) < 0.04, rng.uniform(1.0, 3.0, n) * rng.choice([-1.0, 1.0], n), 0.0)
        out[c] = (amp * (0.5 * wave + rng.normal(0, 0.08, n) + spikes)).astype(np.float32)
    return out
