"""Restatement of include/ecgvit_hip_pr.h in numpy and Python integers: the walk over the sorted order of tests/rank_ref.py from the highest score
down, tie group by tie group, with unbounded integers for the truncated average-precision terms and the cross-multiplied F comparison.  A plain
module: tests/test_pr_metrics.py holds it to scikit-learn on the CPU, tests/test_gpu_pr_metrics.py holds the kernel to it, integer by integer."""
import numpy as np

import rank_ref as R

Q = 1 << 32


def six(key, y, w=None):
    """[ap_q, wp, wn, f_tp, f_fp, f_pos] of one class, Python integers.  key: the uint32 keys of the records; y: labels; w: integer weights"""
    n = len(key)
    w = np.ones(n, np.int64) if w is None else np.asarray(w, np.int64)
    o = R.order(key)
    s, yy, ww = key[o], np.asarray(y)[o] != 0, w[o]
    wp, wn = int(ww[yy].sum()), int(ww[~yy].sum())
    top = int(np.searchsorted(s, R.NAN_KEY, side='left'))                     # NaN's key is the largest: its records are the tail, never walked
    s, yy, ww = s[:top][::-1], yy[:top][::-1], ww[:top][::-1]                 # descending
    ends = np.flatnonzero(np.r_[s[1:] != s[:-1], True]) if top else np.zeros(0, np.int64)      # the last (lowest) member of every group
    tps, fps = np.cumsum(np.where(yy, ww, 0))[ends].tolist(), np.cumsum(np.where(yy, 0, ww))[ends].tolist()
    ap_q, prev, best = 0, 0, (0, 0, -1)
    for tp, fp, e in zip(tps, fps, ends.tolist()):
        if tp != prev:
            ap_q += (tp - prev) * tp * Q // (tp + fp)
        if tp * (best[0] + best[1] + wp) > best[0] * (tp + fp + wp):          # strictly greater: ties stay with the higher threshold
            best = (tp, fp, top - 1 - e)                                      # the ascending position of the group's lowest member
        prev = tp
    return [ap_q, wp, wn, *best]


def sixes(probs, labels, mult=None):
    """(R, K, 6) int64 for (R, n) multiplicities (None: one row of ones)"""
    n, K = probs.shape
    mult = np.ones((1, n), np.int64) if mult is None else np.asarray(mult)
    ks = [R.keys(probs[:, c]) for c in range(K)]
    return np.array([[six(ks[c], labels[:, c], m) for c in range(K)] for m in mult], np.int64)


def values(v, probs_column=None):
    """(AP, F-max, threshold) in f64 of one six; the threshold is the score at the winning position (None: nothing is predicted)"""
    ap_q, wp, wn, tp, fp, pos = (int(x) for x in v)
    thr = None
    if pos >= 0 and probs_column is not None:
        thr = float(probs_column[R.order(R.keys(probs_column))[pos]])
    return ap_q / (Q * wp), 2 * tp / (tp + fp + wp), thr


# ---- the stores of the GPU tests ----------------------------------------------------------------------------------------------------------
COLUMNS = ('equal', 'distinct', 'grid', 'step_tie', 'lane_tie', 'nan', 'nan_positives', 'no_positive', 'no_negative', 'zeros')


def special_store(rng, n):
    """(n, 10) scores and labels, one column per store of COLUMNS.  The walk runs from the top in steps of 256 positions, four per lane: `step_tie`
    ties the descending ranks 250 .. 261 (across the first step's end), `lane_tie` the ranks 2 .. 5 (across the first lane's end)"""
    K = len(COLUMNS)
    s = np.empty((n, K), np.float32)
    y = (rng.random((n, K)) < 0.3).astype(np.float32)
    if n >= 2:
        y[rng.permutation(n)[:2], :] = np.array([[1], [0]], np.float32)       # both label values wherever a column does not override them
    ranks = lambda: rng.permutation(n).astype(np.float32)                     # noqa: E731  (rank 0 = the lowest score)
    s[:, 0] = 0.25
    s[:, 1] = ranks() - n / 2
    s[:, 2] = rng.integers(0, 9, n) / 8
    for col, (lo, hi) in ((3, (250, 261)), (4, (2, 5))):
        v = ranks()
        desc = n - 1 - v
        v[(desc >= lo) & (desc <= hi)] = n - 1 - hi
        s[:, col] = v
    s[:, 5] = rng.integers(0, 9, n) / 8
    s[rng.random(n) < 0.25, 5] = np.nan
    s[:, 6] = rng.integers(0, 9, n) / 8
    s[y[:, 6] != 0, 6] = np.nan                                               # every positive scores NaN: valid, AP 0, nothing predicted
    s[:, 7] = rng.integers(0, 9, n) / 8
    y[:, 7] = 0
    s[:, 8] = rng.integers(0, 9, n) / 8
    y[:, 8] = 1
    s[:, 9] = rng.choice(np.array([-0.0, 0.0, -1.0, 1.0], np.float32), n)     # -0 and +0: one tie group
    return s, y
