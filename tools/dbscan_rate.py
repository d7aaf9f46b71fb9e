#!/usr/bin/env python3
"""The DBSCAN sweeps (csrc/dbscan.hip) at the sizes an all-pairs method reaches, one GPU process:
  (a) on a random-walk store of about 2^17, 2^19 and 2^21 segments, at k = 8 and k = 16: the count sweep (n^2 pairs), the link sweep over the
      core segments (m (m - 1) / 2 pairs), the border sweep (non-core x core pairs) and a whole `EcgTokenizer.dbscan` (its host reads and
      torch's compaction included): seconds and ns per pair.  eps is the 1 % quantile of the distances among 4 096 sampled segments and
      min_samples = 5, so nearly every segment is a core point: the link sweep at its largest;
  (b) from the same run, the k-means++ seeding's sweep on the largest store -- the same tok_d2 on the vector pipe -- as ns per (segment,
      candidate): a sweep + pick pair from the difference of a 9-centre and a 1-centre seeding, T = 10 candidates;
  (c) `sklearn.cluster.DBSCAN` on the host over the first 2^15 segments (f64; the largest size tried: its neighbourhoods are materialised)
      against the device on the same segments (skipped when sklearn is absent).
Writes profiles/r26_dbscan.txt (--out).
usage: python tools/dbscan_rate.py [--reps 1] [--max-log2 21]"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ecg_representation_learning_amd as E  # noqa: E402
from ecg_representation_learning_amd import tokenizer  # noqa: E402
from ecg_representation_learning_amd.hip import lib, check, ptr, stream  # noqa: E402

C, L = 12, 5000


def timed(fn, reps):
    """seconds per call, after one warm-up"""
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps


def sweeps(tok, segs, eps2, ms, reps):
    """-> (n, m, seconds of count, link, border): the launches of `EcgTokenizer._dbscan`, each sweep timed on its own"""
    Lb, s, k, n = lib(), stream(), tok.k, segs.shape[0]
    count = torch.empty(n, dtype=torch.int32, device=segs.device)

    def do_count():
        for lo, hi in tok._row_blocks(n, n):
            check(Lb.ecgvit_tok_dbscan_count(ptr(segs), n, k, eps2, lo, hi, ptr(count), s), 'count')
    t_count = timed(do_count, reps)
    is_core = count >= ms
    core = is_core.nonzero().view(-1)
    m = int(core.numel())
    if m == 0:
        return n, 0, t_count, 0.0, 0.0
    table = segs.index_select(0, core)
    parent = torch.empty(m, dtype=torch.int32, device=segs.device)

    def do_link():
        parent.copy_(torch.arange(m, dtype=torch.int32, device=segs.device))
        for lo, hi in tok._row_blocks(m, m):
            if hi > 1:
                check(Lb.ecgvit_tok_dbscan_link(ptr(table), m, k, eps2, lo, hi, ptr(parent), s), 'link')
    t_link = timed(do_link, reps)
    roots = torch.empty(m, dtype=torch.int32, device=segs.device)
    check(Lb.ecgvit_tok_dbscan_flatten(ptr(parent), m, ptr(roots), s), 'flatten')
    label = torch.unique(roots, sorted=True, return_inverse=True)[1].to(torch.int32)
    rest = (~is_core).nonzero().view(-1)
    nb, t_border = int(rest.numel()), 0.0
    if nb:
        rows = segs.index_select(0, rest)
        got = torch.empty(nb, dtype=torch.int32, device=segs.device)

        def do_border():
            for lo, hi in tok._row_blocks(nb, m):
                check(Lb.ecgvit_tok_dbscan_border(ptr(rows), nb, ptr(table), ptr(label), m, k, eps2, lo, hi, ptr(got), s), 'border')
        t_border = timed(do_border, reps)
    return n, m, t_count, t_link, t_border


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=1)
    ap.add_argument('--max-log2', type=int, default=21)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r26_dbscan.txt'))
    a = ap.parse_args()
    import bench
    sizes = [s for s in (17, 19, 21) if s <= a.max_log2]
    ms = 5
    lines = [f'sources: bench.kernel_source_hash() = {bench.kernel_source_hash()}; {torch.cuda.get_device_name(0)}',
             f'store: random walks (cumulative sums of N(0, 0.05^2) steps), records of {C} x {L} f32; min_samples = {ms}; {a.reps} run(s) after one warm-up; '
             f'at most 2^{tokenizer.DBSCAN_PAIRS_PER_LAUNCH.bit_length() - 1} pairs per launch']
    g = torch.Generator(device='cuda').manual_seed(26)
    for k in (8, 16):
        tok = E.EcgTokenizer(k=k, pad='shift')
        per = C * (L // k + 1)
        for log2 in sizes:
            R = max(1, round(2 ** log2 / per))
            x = torch.randn((R, C, L), device='cuda', generator=g).mul_(0.05).cumsum_(dim=-1)
            segs, _ = tok.segments(x)
            pick = torch.randint(0, len(segs), (4096,), device='cuda', generator=g)
            eps = float(torch.quantile(torch.pdist(segs[pick].double()).float(), 0.01))
            eps2 = tokenizer.check_eps(eps)
            n, m, t_count, t_link, t_border = sweeps(tok, segs, eps2, ms, a.reps)
            t_fit = timed(lambda: tok.dbscan(x, eps, ms), a.reps)
            lines.append(f'(a) k = {k}: {R} records, n = {n} segments, eps = {eps:.4g}, {m} core')
            lines.append(f'    count    {t_count:9.3f} s  {t_count / (n * n) * 1e9:9.5f} ns per pair ({n * n:.3e} pairs)')
            if m > 1:
                lines.append(f'    link     {t_link:9.3f} s  {t_link / (m * (m - 1) / 2) * 1e9:9.5f} ns per pair ({m * (m - 1) / 2:.3e} pairs)')
            if m and n - m:
                lines.append(f'    border   {t_border:9.3f} s  {t_border / ((n - m) * m) * 1e9:9.5f} ns per pair ({(n - m) * m:.3e} pairs)')
            lines.append(f'    dbscan() {t_fit:9.3f} s  (segments, the sweeps, compaction, flatten, ranks, two host reads, labels to the host)')
            print('\n'.join(lines[-5:]), flush=True)
            if log2 == sizes[-1]:                       # (b) the seeding's sweep on the same store
                st = tok._record_store(x, None, None)
                T, nseg = 10, st.C * st.n_seg
                rng = np.random.default_rng(26)

                def seeding(v):
                    first, u53 = tok._seed_draws(rng, nseg, v, T)
                    tok._seed(st, v, T, first, u53)
                pair = (timed(lambda: seeding(9), a.reps) - timed(lambda: seeding(1), a.reps)) / 8
                lines.append(f'(b) k = {k}: k-means++ sweep + pick, T = {T}, {nseg} segments: {pair * 1e3:9.3f} ms = {pair / (nseg * T) * 1e9:9.5f} ns per (segment, candidate); '
                             f'count = x {t_count / (n * n) / (pair / (nseg * T)):.2f} of it per pair')
                print(lines[-1], flush=True)
            if k == 8 and log2 == sizes[0]:             # (c) the host's route, at a size the host finishes
                sub = segs[:2 ** 15].contiguous()
                t_dev = timed(lambda: tok._dbscan(sub, eps2, ms)[1].cpu(), a.reps)
                try:
                    from sklearn.cluster import DBSCAN
                    host = sub.cpu().numpy().astype(np.float64)
                    t0 = time.perf_counter()
                    sk = DBSCAN(eps=eps, min_samples=ms).fit(host)
                    t_host = time.perf_counter() - t0
                    same = bool(np.array_equal(sk.labels_, tok._dbscan(sub, eps2, ms)[1].cpu().numpy()))
                    lines.append(f'(c) k = {k}: sklearn.cluster.DBSCAN on the host, {len(host)} segments (f64): {t_host:8.2f} s; the device on the same segments: '
                                 f'{t_dev * 1e3:8.2f} ms = x {t_host / t_dev:.0f}; labels equal: {same} (a pair within f32 rounding of eps may differ)')
                except ImportError:
                    lines.append(f'(c) sklearn is not installed here: no host row (the device, {len(sub)} segments: {t_dev * 1e3:8.2f} ms)')
                print(lines[-1], flush=True)
            del x, segs
    text = '\n'.join(lines) + '\n'
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as fh:
        fh.write(text)


if __name__ == '__main__':
    main()
