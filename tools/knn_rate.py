#!/usr/bin/env python3
"""The exact k-NN search (csrc/knn.hip, `KnnIndex.search` under the dot metric) beside the cheapest torch form, one run on one device, every
timing by device events after a warm-up of that shape.  Shapes, all at k = 20:
  (1) Q = 2 200 against N = 17 400 at d = 768: the PTB-XL test fold against its training folds;
  (2) leave-one-out at Q = N = 21 837, d = 768;
  (3) Q = 4 096 against N = 800 000, d = 768;
  (4) shape (1) at d = 1 024.
The torch form: `(q[lo:hi] @ bank.T).topk(k)` over chunks of queries sized so that the (chunk, N) temporary stays under 1 GiB (the own row set to
-inf for leave-one-out), the chunks' lists joined -- the merge of a query-chunked search is a concatenation.
Columns: milliseconds; 2 Q N d / t as a share of the 157.3 TF/s f32 matrix peak; peak device memory above the resting allocation (the stores
and the timing events) during one call; the number of queries whose k indices are equal in the two forms (the two sum the products in
different orders: rows whose scores differ by rounding may change places).
Writes profiles/r28_knn.txt (--out).
usage: python tools/knn_rate.py [--reps 3]"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ecg_representation_learning_amd as E  # noqa: E402

PEAK_TF = 157.3
K = 20
SHAPES = (('PTB-XL test fold against its training folds', 2200, 17400, 768, False),
          ('leave-one-out over PTB-XL', 21837, 21837, 768, True),
          ('4 096 queries against a MIMIC-IV-ECG-sized bank', 4096, 800000, 768, False),
          ('the first shape at d = 1 024', 2200, 17400, 1024, False))


def timed(fn, reps):
    """(milliseconds per call by device events after one warm-up, peak bytes above the resting allocation during one call, the last result)"""
    out = fn()
    torch.cuda.synchronize()
    del out
    rest = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - rest
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        out = fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / reps, peak, out


def torch_form(q, bank, k, loo):
    Q, N = q.shape[0], bank.shape[0]
    rows = max(1, min(Q, (1 << 30) // (4 * N)))
    scores, indices = [], []
    for lo in range(0, Q, rows):
        s = q[lo:lo + rows] @ bank.T
        if loo:
            r = torch.arange(s.shape[0], device=s.device)
            s[r, r + lo] = float('-inf')
        top = s.topk(k, dim=1)
        scores.append(top.values)
        indices.append(top.indices)
    return torch.cat(scores), torch.cat(indices)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r28_knn.txt'))
    a = ap.parse_args()
    import bench
    lines = [f'sources: bench.kernel_source_hash() = {bench.kernel_source_hash()}; {torch.cuda.get_device_name(0)}; torch {torch.__version__}',
             f'stores: N(0, 1) f32 rows; k = {K}; {a.reps} run(s) per form after one warm-up of the shape, device events; '
             f'share = 2 Q N d / t of {PEAK_TF} TF/s',
             f'{"shape":>50s} {"Q":>7s} {"N":>7s} {"d":>5s} | {"knn ms":>9s} {"share":>6s} {"peak MiB":>9s} | {"torch ms":>9s} {"share":>6s} {"peak MiB":>9s} | '
             f'{"torch / knn":>11s} {"equal index rows":>17s}']
    g = torch.Generator(device='cuda').manual_seed(28)
    for name, Q, N, d, loo in SHAPES:
        bank = torch.randn((N, d), device='cuda', generator=g)
        q = bank if loo else torch.randn((Q, d), device='cuda', generator=g)
        index = E.KnnIndex(bank, metric='dot')
        t_knn, m_knn, (_, i_knn) = timed(lambda: index.search(q, K, exclude_self=loo), a.reps)
        t_torch, m_torch, (_, i_torch) = timed(lambda: torch_form(q, bank, K, loo), a.reps)
        equal = int((i_knn == i_torch).all(dim=1).sum())
        flop = 2.0 * Q * N * d
        lines.append(f'{name:>50s} {Q:7d} {N:7d} {d:5d} | {t_knn:9.3f} {flop / t_knn / 1e9 / PEAK_TF:6.1%} {m_knn / 2 ** 20:9.1f} | '
                     f'{t_torch:9.3f} {flop / t_torch / 1e9 / PEAK_TF:6.1%} {m_torch / 2 ** 20:9.1f} | {t_torch / t_knn:11.2f} {equal:9d} of {Q}')
        print(lines[-1], flush=True)
        del bank, q, index, i_knn, i_torch
        torch.cuda.empty_cache()
    text = '\n'.join(lines) + '\n'
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as fh:
        fh.write(text)


if __name__ == '__main__':
    main()
