#!/usr/bin/env python3
"""Fitting the per-lead normalisation statistics on the device (`fit_dynamic_normalize`, csrc/fit_stats.hip), one GPU process:
  (a) every pass alone -- moments (count + sum), moments (squared deviations), the four histogram passes of the radix select with the default
      fit's four ranks per lead -- us per launch and GB/s of samples read, on a rectangular 21 837 x 12 x 2 500 f32 store and on a ragged
      (12, S_total) store of the same bytes with record lengths in [50 %, 100 %] of 2 500, each holding a Gaussian input and a clustered one
      (Gaussian, sigma = 0.2, with 30 % exact zeros).  The stores are ten times the 256-MB Infinity Cache: every launch streams from HBM.
      A histogram pass that runs the clustered input at less than half the Gaussian input's rate is FLAGGED in the table;
  (b) the yardsticks of an HBM-bound read, timed in the same run: `ecgvit_pool_records` (f32 rows over the same buffer) and the rectangular
      `ecgvit_patch_gather` (f32 in, bf16 patches out);
  (c) the whole default fit (('norm', 3), ('std', 1)) through `fit_dynamic_normalize`, wall clock with the host's part, beside the same
      statistics by torch on the device (`nanmean`, and a per-lead `sort` for the percentiles; `torch.nanquantile` is tried and its refusal
      noted) and by numpy on the host on a 2 048-record subset, scaled by the record count (stated in the row);
  (d) the two errors tests/test_gpu_normalize_fit.py::test_forward_through_the_fitted_transform measures (run as a child process).
Writes profiles/r18_normalize_fit.txt (--out).
usage: python tools/normalize_fit.py [--reps 5] [--records 21837]"""
import argparse
import os
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ecg_representation_learning_amd as E  # noqa: E402
from ecg_representation_learning_amd import hip, transform as T  # noqa: E402
from ecg_representation_learning_amd.hip import lib, check, ptr, stream  # noqa: E402
from ecg_representation_learning_amd.records import DeviceTables, select_records  # noqa: E402

C, L = 12, 2500


def timed(fn, reps, warmup=1):
    """us per call"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) * 1e3 / reps


def make(n, kind, ragged, seed):
    g = torch.Generator(device='cuda').manual_seed(seed)
    if ragged:
        lens = np.random.default_rng(seed).integers(L // 2, L + 1, size=int(n * L / (0.75 * L)) + 64)
        lens = lens[:int(np.searchsorted(np.cumsum(lens), n * L))]
        off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        shape = (C, int(off[-1]))
    else:
        off, shape = None, (n, C, L)
    x = torch.randn(shape, device='cuda', generator=g)
    if kind == 'clustered':
        x.mul_(0.2)
        x.masked_fill_(torch.rand(shape, device='cuda', generator=g) < 0.3, 0.0)
    return x, off


def passes(x, off, reps):
    """{pass name: us}, the launches exactly as `device_raw_stats` queues them for the default fit"""
    tab = DeviceTables.of(x, select_records(x, off, None))
    R, so, rl, stride = tab.R, tab.src_off, tab.raw_len, tab.stride
    ws = torch.empty(lib().ecgvit_fit_workspace(R, C) // 8, dtype=torch.float64, device='cuda')
    state = torch.zeros(C, 4, dtype=torch.int64, device='cuda')
    hist = torch.zeros(4, C, 16, 256, dtype=torch.int64, device='cuda')
    scratch = torch.zeros(C, 16, 256, dtype=torch.int64, device='cuda')
    mom = lambda mean, st: check(lib().ecgvit_fit_moments(ptr(x), ptr(so), stride, ptr(rl), R, C, ptr(mean), ptr(ws), ptr(st), stream()), 'fit_moments')
    hst = lambda p, seld, h: check(lib().ecgvit_fit_histogram(ptr(x), ptr(so), stride, ptr(rl), R, C, ptr(seld), 4, p, ptr(h), stream()), 'fit_histogram')
    out = {}
    mom(None, state)
    st = state.cpu().numpy()
    count = st[:, 0]
    mean = torch.from_numpy(st[:, 2].copy().view(np.float64) / count).cuda()
    tmp = torch.zeros_like(state)
    out['moments: count, NaN count, sum'] = timed(lambda: mom(None, tmp), reps)
    out['moments: squared deviations'] = timed(lambda: mom(mean, tmp), reps)
    p3 = T.norm_percentile(3)
    hs = np.zeros((C, 16, 4), np.int64)
    for c in range(C):
        lo, hi, _ = T.percentile_targets(100 - p3, int(count[c]))
        lo2, hi2, _ = T.percentile_targets(p3, int(count[c]))
        hs[c, :4, 0] = [lo, hi, lo2, hi2]
    seld = torch.from_numpy(hs).cuda()
    for p in range(4):
        hst(p, seld, hist[p])
        out[f'histogram pass {p} (key bits {31 - 8 * p}..{24 - 8 * p})'] = timed(lambda: hst(p, seld, scratch), reps)
        check(lib().ecgvit_fit_select(ptr(hist[p]), ptr(seld), C, 4, p, stream()), 'fit_select')
    out['select (scan of 4 targets x 12 leads)'] = timed(lambda: check(lib().ecgvit_fit_select(ptr(hist[3]), ptr(seld.clone()), C, 4, 3, stream()), 'fit_select'), reps)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--records', type=int, default=21837)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r18_normalize_fit.txt'))
    a = ap.parse_args()
    import bench
    n = a.records
    nbytes = n * C * L * 4
    lines = [f'sources: bench.kernel_source_hash() = {bench.kernel_source_hash()}; {torch.cuda.get_device_name(0)}',
             f'(a) one pass over the store, us per launch (GB/s of samples read), {a.reps} launches after one warm-up; rectangular {n} x {C} x {L} f32 = {nbytes / 1e9:.2f} GB, '
             f'ragged (12, S_total) of the same bytes with lengths in [{L // 2}, {L}]']
    table, whole = {}, {}
    for ragged in (False, True):
        for kind in ('gaussian', 'clustered'):
            x, off = make(n, kind, ragged, 7)
            gb = x.numel() * 4 / 1e9
            t = passes(x, off, a.reps)
            table[(ragged, kind)] = (t, gb)
            best = None
            for _ in range(3):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fit = E.fit_dynamic_normalize(x, offsets=off)
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                best = dt if best is None else min(best, dt)
            whole[(ragged, kind)] = (best, gb, fit)
            print('ragged' if ragged else 'rect', kind, {k: round(v, 1) for k, v in t.items()}, f'whole fit {best * 1e3:.2f} ms', flush=True)
            if not ragged and kind == 'gaussian':
                xg = x
            else:
                del x
    names = list(table[(False, 'gaussian')][0])
    slow = []
    for ragged in (False, True):
        for nm in names:
            row = f'    {"ragged" if ragged else "rect  "} {nm:42s}'
            for kind in ('gaussian', 'clustered'):
                t, gb = table[(ragged, kind)]
                row += f'  {kind} {t[nm]:9.1f} us' + (f' ({gb / (t[nm] * 1e-6):7.0f} GB/s)' if 'select' not in nm else ' ' * 15)
            tg, tc = table[(ragged, 'gaussian')][0][nm], table[(ragged, 'clustered')][0][nm]
            if nm.startswith('histogram') and tc > 2 * tg:
                row += f'   CLUSTERED INPUT RUNS THIS PASS AT {tg / tc:.2f} OF THE GAUSSIAN RATE (LDS atomic contention)'
                slow.append((ragged, nm, tg / tc))
            lines.append(row)
    lines.append('    no histogram pass runs the clustered input below half the Gaussian rate' if not slow else
                 f'    {len(slow)} histogram pass(es) run the clustered input below half the Gaussian rate: see the flags above')

    # (b) yardsticks on the rectangular Gaussian store
    d = 1000
    rows = xg.numel() // d
    B, N = rows // 30, 30
    pooled = torch.empty(B, d, device='cuda')
    tp = timed(lambda: check(lib().ecgvit_pool_records(ptr(xg), ptr(pooled), None, None, B, N, d, hip.POOL_MEAN, None, None, 1e-5, hip.F32, stream()), 'pool_records'), a.reps)
    Bg = min(n, 4096)
    patches = torch.empty(Bg * (L // 20), C * 20, device='cuda', dtype=torch.bfloat16)
    ring = [xg[i * Bg:(i + 1) * Bg] for i in range(max(1, n // Bg))]
    turn = [0]

    def gather():
        turn[0] += 1
        check(lib().ecgvit_patch_gather(ptr(ring[turn[0] % len(ring)]), ptr(patches), Bg, C, L, 20, C * 20, hip.BF16, stream()), 'patch_gather')
    tg = timed(gather, 2 * len(ring), warmup=2)
    lines.append('(b) yardsticks of an HBM-bound read on the rectangular Gaussian store, same run (GB/s of f32 read)')
    lines.append(f'    ecgvit_pool_records, mean over N = {N} rows of d = {d} f32, B = {B}: {tp:9.1f} us ({B * N * d * 4 / 1e9 / (tp * 1e-6):7.0f} GB/s)')
    lines.append(f'    ecgvit_patch_gather, B = {Bg} of {C} x {L}, P = 20, bf16 patches (writes half the bytes it reads), slices of the store in turn: '
                 f'{tg:9.1f} us ({Bg * C * L * 4 / 1e9 / (tg * 1e-6):7.0f} GB/s)')

    # (c) the whole fit and the same statistics elsewhere
    lines.append("(c) the whole default fit (('norm', 3), ('std', 1)): fit_dynamic_normalize on the device store, wall clock, best of 3 (6 sweeps of the store + select + host algebra)")
    for (ragged, kind), (best, gb, _) in whole.items():
        lines.append(f'    {"ragged" if ragged else "rect  "} {kind:10s} {best * 1e3:9.2f} ms  ({6 * gb / best:7.0f} GB/s over the six sweeps)')
    p3 = T.norm_percentile(3)

    def torch_stats():
        m = xg.nanmean(dim=(0, 2))
        qs = []
        for c in range(C):
            s = xg[:, c, :].reshape(-1).sort().values
            lo, hi, g = T.percentile_targets(p3, s.numel())
            qs.append(s[lo] + (s[hi] - s[lo]) * g)
        return m, torch.stack(qs)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    torch_stats()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    torch_stats()
    torch.cuda.synchronize()
    tt = time.perf_counter() - t0
    lines.append(f'    torch on the device, same rectangular Gaussian store: nanmean over (0, 2) + per lead a contiguous copy and sort (percentiles read off the sorted lead; no nanstd): {tt * 1e3:9.2f} ms '
                 f'= x {tt / whole[(False, "gaussian")][0]:.1f} the fit')
    try:
        torch.nanquantile(xg[:, 0, :].reshape(-1), 0.5)
        lines.append('    torch.nanquantile on one lead of the store: accepted')
    except RuntimeError as e:
        lines.append(f'    torch.nanquantile on one lead of the store ({n * L} samples) refuses: {str(e).splitlines()[0][:160]}')
    sub = min(2048, n)
    xs = xg[:sub].cpu().numpy().astype(np.float64)
    t0 = time.perf_counter()
    lo = np.nanpercentile(xs, 100 - p3, axis=(0, -1), keepdims=True)
    hi_ = np.nanpercentile(xs, p3, axis=(0, -1), keepdims=True)
    ys = (xs - lo) / (hi_ - lo)
    np.nanmean(ys, axis=(0, -1), keepdims=True)
    np.nanstd(ys, axis=(0, -1), keepdims=True)
    tn = time.perf_counter() - t0
    lines.append(f'    numpy on the host as the reference fits it (2 nanpercentile, the stage-1 transform, nanmean, nanstd; f64), {sub} records: {tn:.2f} s; '
                 f'scaled linearly by {n}/{sub} records (the selection inside nanpercentile is linear; a lower bound): {tn * n / sub:.1f} s = x {tn * n / sub / whole[(False, "gaussian")][0]:.0f} the fit')

    # (d) the forward errors of the test
    r = subprocess.run([sys.executable, '-m', 'pytest', '-q', '-s', '-m', 'gpu', os.path.join(ROOT, 'tests', 'test_gpu_normalize_fit.py') + '::test_forward_through_the_fitted_transform'],
                       capture_output=True, text=True, cwd=ROOT)
    lines.append('(d) errors as tests/test_gpu_normalize_fit.py::test_forward_through_the_fitted_transform measures them on the two fixture records (bound: twice the reference f32 chain\'s)')
    lines += ['    ' + l.strip() for l in r.stdout.splitlines() if 'normalize fit forward' in l] or ['    (the test printed nothing: exit code %d)' % r.returncode]
    text = '\n'.join(lines) + '\n'
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as fh:
        fh.write(text)


if __name__ == '__main__':
    main()
