#!/usr/bin/env python3
"""The rank route to AUROC (csrc/rank_metrics.hip) beside the all-pairs kernel and beside scikit-learn on the host, one run on one device.
Shapes: K = 71 classes at n = 2 200 (the PTB-XL test fold), 21 837 (all of PTB-XL) and 350 000 records; scores on a grid of 4 096 values (ties),
label rates 5 % .. 50 %, so that every resample holds both label values of every class and `roc_auc_score` never refuses.
Forms, each warmed up at the shape, then timed in `--reps` rounds that alternate the forms (host clock around a device synchronise; median and
range of the rounds):
  sort        `rank_scores`: keys, four digit passes of three launches, pack
  point       `auroc_counts`: the sort, the confusion counts, one walk with unit weights -- end to end
  all pairs   `eval_counts`: what `get_accuracy` runs today
  bootstrap   `bootstrap_auc(n_boot=1000)`: the sort, the point estimate, 1 000 seeded replicates in chunks of the default workspace, the read-back of
              the (1000, 71, 3) integers and the host's divisions -- end to end
  host        `roc_auc_score` per class on `--host-replicates` resamples (numpy draws; the D2H copy of the scores is not counted), scaled to 1 000
Also: whether the two point estimates hold equal integers at the shape.
Writes profiles/r29_rank_metrics.txt (--out).
usage: python tools/rank_metrics_rate.py [--reps 5] [--host-replicates 20]"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ecg_representation_learning_amd as E  # noqa: E402

K, N_BOOT = 71, 1000
SHAPES = (('the PTB-XL test fold', 2200), ('all of PTB-XL', 21837), ('a 350 000-record corpus', 350000))


def clock(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--host-replicates', type=int, default=20)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r29_rank_metrics.txt'))
    a = ap.parse_args()
    from sklearn.metrics import roc_auc_score
    import bench
    fmt = lambda ts: f'{statistics.median(ts):10.3f} ({min(ts):.3f} .. {max(ts):.3f})'   # noqa: E731
    lines = [f'sources: bench.kernel_source_hash() = {bench.kernel_source_hash()}; {torch.cuda.get_device_name(0)}; torch {torch.__version__}',
             f'K = {K}; grid scores (4 096 values), label rates 5 % .. 50 %; {a.reps} alternating rounds per form after one warm-up of the shape; '
             f'milliseconds, median (min .. max); host clock around a device synchronise',
             f'bootstrap = bootstrap_auc(n_boot={N_BOOT}) end to end; host = roc_auc_score x {K} classes on {a.host_replicates} resamples, scaled to {N_BOOT}']
    rng = np.random.default_rng(29)
    for name, n in SHAPES:
        sc = (rng.integers(0, 4096, (n, K)) / 4096).astype(np.float32)
        yy = (rng.random((n, K)) < np.linspace(0.05, 0.5, K)).astype(np.float32)
        ds, dy = torch.from_numpy(sc).cuda(), torch.from_numpy(yy).cuda()
        forms = (('sort', lambda: E.rank_scores(ds, dy)), ('point', lambda: E.auroc_counts(ds, dy).counts),
                 ('all pairs', lambda: E.eval_counts(ds, dy).counts), ('bootstrap', lambda: E.bootstrap_auc(ds, dy, n_boot=N_BOOT, seed=29)))
        out = {}
        for key, fn in forms:                                        # warm-up of every form at this shape
            out[key] = clock(fn)[1]
        equal = torch.equal(out['point'], out['all pairs'])
        lo, hi = out['bootstrap'].ci()
        ts = {key: [] for key, _ in forms}
        for _ in range(a.reps):
            for key, fn in forms:
                ts[key].append(clock(fn)[0])
        print(f'n = {n}: device rounds done, host replicates running', flush=True)
        t0 = time.perf_counter()
        for b in range(a.host_replicates):
            row = rng.integers(0, n, n)
            s_b, y_b = sc[row], yy[row]
            for c in range(K):
                roc_auc_score(y_b[:, c], s_b[:, c])
        host = (time.perf_counter() - t0) * 1e3 * N_BOOT / a.host_replicates
        med = {key: statistics.median(v) for key, v in ts.items()}
        lines += [f'n = {n} ({name}); point estimates hold equal integers: {equal}; macro AUROC {out["bootstrap"].point["macro_auc"]:.4f}, 95 % interval {lo:.4f} .. {hi:.4f}; '
                  f'replicates per chunk {out["bootstrap"].chunk}']
        lines += [f'    {key:>10s} {fmt(ts[key])}' for key, _ in forms]
        lines += [f'    {"host":>10s} {host:10.1f} (scaled from {a.host_replicates} replicates)',
                  f'    all pairs / point = {med["all pairs"] / med["point"]:.2f}; host / bootstrap = {host / med["bootstrap"]:.1f}; '
                  f'replicate walk visits per second = {N_BOOT * K * n / ((med["bootstrap"] - med["point"]) * 1e-3):.3e} (bootstrap less point)']
        for line in lines[-7:]:
            print(line, flush=True)
        del ds, dy, out
        torch.cuda.empty_cache()
    text = '\n'.join(lines) + '\n'
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as fh:
        fh.write(text)


if __name__ == '__main__':
    main()
