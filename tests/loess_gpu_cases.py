"""The inputs of tests/test_gpu_loess.py, shared with the CPU test that checks them (tests/test_loess.py): every store is seeded
(`loess_ref.signal`: a smooth wave, Gaussian noise, sparse large spikes), and each shape is there for an edge of csrc/denoise.hip's rloess_kernel.
The degree-2 cases of 4 and 5 samples hold exactly determined windows (degree + 1 samples of positive distance weight): there the residuals are the
solver's rounding and a median of exactly 0 is common, so their leads are power-of-two multiples of one lead (the same roundings, the same
decisions) and the seed is one at which no window's median is 0.  A case: lengths (one record, or the records of a ragged store), npoints (an int, or the fraction form), degree, robust_iters, the seed, and the
leads the numpy restatement is run for (None: all twelve)."""
import numpy as np

import loess_ref as R


def case(lengths, npoints, degree=2, robust_iters=10, seed=0, leads=None, scaled=False):
    return dict(lengths=[lengths] if isinstance(lengths, int) else list(lengths), npoints=npoints, degree=degree, robust_iters=robust_iters, seed=seed,
                leads=leads, scaled=scaled)


CASES = {
    # the shortest records: degree + 2 samples and one more; npoints above n takes the whole record
    'n4_d1': case(4, 31, 1, seed=1), 'n4_d2': case(4, 31, 2, seed=502, scaled=True), 'n5_m4_d1': case(5, 4, 1, seed=3), 'n5_m4_d2': case(5, 4, 2, seed=304, scaled=True),
    'n5_d2': case(5, 31, 2, seed=5, scaled=True), 'n40_wider': case(40, 63, 2, seed=6),
    # n = npoints and npoints + 1: every window is clamped to an end
    'n31_m31': case(31, 31, 2, seed=7), 'n32_m31': case(32, 31, 2, seed=8), 'n32_m32': case(32, 32, 2, seed=9), 'n33_m32_d1': case(33, 32, 1, seed=10),
    # around one and two slots per lane, odd and even medians
    'm63': case(200, 63, 2, seed=11), 'm64': case(200, 64, 2, seed=12), 'm65': case(200, 65, 2, seed=13), 'm129': case(200, 129, 2, seed=14),
    'm64_d1': case(200, 64, 1, seed=15), 'm129_d1': case(200, 129, 1, seed=16),
    # the plain LOESS and a single robust pass
    'm65_plain': case(200, 65, 2, 0, seed=17), 'm65_one': case(200, 65, 2, 1, seed=18), 'm64_d1_plain': case(200, 64, 1, 0, seed=19),
    # the reference's window at 500 Hz and the widest one (8 and 16 slots per lane)
    'm500': case(1100, 500, 2, seed=20, leads=(0, 5, 11)), 'm1024': case(1100, 1024, 2, seed=21, leads=(0, 5, 11)),
    # the longest record: 128 KiB of LDS (5 points at degree 2 would be interpolated in the interior: degree 1 there, 7 points at degree 2)
    'n32768': case(32768, 5, 1, seed=22, leads=(0, 5, 11)), 'n32768_d2': case(32768, 7, 2, seed=24, leads=(0, 5, 11)),
    # the fraction form on a ragged store: 209, 99 and 19 points
    'frac': case((700, 333, 64), 0.3, 2, seed=23),
}


def case_store(c):
    """-> (store (12, sum of lengths) float32, offsets)"""
    off = np.concatenate([[0], np.cumsum(c['lengths'])])
    return np.concatenate([R.signal(c['seed'] + 1000 * i, n, scaled=c['scaled']) for i, n in enumerate(c['lengths'])], axis=1), off


def case_points(c, n):
    return R.frac_points(n, c['npoints']) if isinstance(c['npoints'], float) else c['npoints']


def case_input(c):
    """-> (record, lead, samples, window width) of every lead the restatement is run for"""
    store, off = case_store(c)
    for i, n in enumerate(c['lengths']):
        for lead in (range(12) if c['leads'] is None else c['leads']):
            yield (i, lead), store[lead, off[i]:off[i + 1]], case_points(c, n)
