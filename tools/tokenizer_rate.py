#!/usr/bin/env python3
"""The segment tokenizer's kernels (csrc/tokenize.hip) at corpus size, one GPU process:
  (a) assign, update and one full Lloyd iteration (assign with the changed counter, its 8-byte read, update) on a resident
      21 837 x 12 x 5 000 f32 store, at k = 8, V = 4 096 and at k = 16, V = 1 024: ms per launch, segments/s, and for assign the rate of the
      score product alone (2 k FLOP per score) beside the board's f32 matrix peak -- the expectation to check is that assign is bound by that
      rate, not by the running argmin;
  (b) in the same process, a chunked `torch.cdist(...).argmin` on the same device over the same store and the same table: every whole
      segment of every run (the padded last one of each run is left out, the time is scaled by the segment count; the mean is removed by
      torch beforehand and not timed), and the share of those segments on which it agrees with assign's ids;
  (c) sklearn's `KDTree.query` on the host over a 1 % sample of the segments, scaled by 100 (stated in the row; skipped when sklearn is absent).
Writes profiles/r19_tokenizer.txt (--out).
--seed: the k-means++ seeding (ecgvit_tok_seed) instead, on the same store at the same two shapes with sklearn's default number of trials T:
  (d) a whole seeding; a sweep + pick pair, as the difference of a 9-centre and a 1-centre seeding over 8; the sweep and the pick apart, from
      the kernel durations torch.profiler records for one 9-centre seeding (left out where the profiler reports no kernels);
  (e) beside it `ecgvit_tok_assign` with a (T + 1)-row table on the same store, which reads the same bytes;
  (f) `sklearn.cluster.kmeans_plusplus` on the host at a size the host finishes (2 M segments, V = 256, f64) against the device on the same
      segments (skipped when sklearn is absent).
Writes profiles/r25_tokenizer_seed.txt (--out).
--scalable: the scalable k-means++ seeding (ecgvit_tok_scalable_seed, csrc/tok_scalable.hip) on the same store at the same two shapes, with the
  defaults of `ScalableKMeansPlusPlus` (oversampling factor 2, five rounds, sklearn's T):
  (g) a whole seeding (event-timed, the sweep for the maximum included), and the time of its folds, selections (count, scan, scatter), weights
      pass and recluster from the kernel durations torch.profiler records for that run;
  (h) the `KMeansPlusPlus` seeding re-measured in the same run, on the same store with the same T;
  (i) the full-store potential of each seeding (the sum of the f32 distances `ecgvit_tok_assign` reports under its centres) and the inertia
      after ten Lloyd iterations from each.
Writes profiles/r27_tokenizer_scalable.txt (--out).
usage: python tools/tokenizer_rate.py [--reps 3] [--records 21837] [--seed | --scalable]"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ecg_representation_learning_amd as E  # noqa: E402
from ecg_representation_learning_amd.hip import lib  # noqa: E402

C, L = 12, 5000
F32_MATRIX_PEAK = 157.3e12      # FLOP/s, v_mfma_f32_32x32x2_f32 at the board's spec clock


def timed(fn, reps, warmup=1):
    """ms per call"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / reps


def kernel_split(fn):
    """us per launch of the seeding's two kernels over one call of fn, from torch.profiler's device events; {} where it records none"""
    from torch.profiler import profile, ProfilerActivity
    try:
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        out = {}
        for ev in prof.key_averages():
            for name in ('tok_seed_sweep_kernel', 'tok_seed_pick_kernel'):
                total = getattr(ev, 'device_time_total', 0) or getattr(ev, 'cuda_time_total', 0)
                if name in ev.key and ev.count and total:
                    n, t = out.get(name, (0, 0.0))
                    out[name] = (n + ev.count, t + total)
        return {k: t / n for k, (n, t) in out.items()}
    except Exception as e:          # a profiler that cannot attach is no reason to lose the table
        print(f'torch.profiler: {e!r}', flush=True)
        return {}


def kernel_totals(fn, groups):
    """{group: (launches, ms in all)} over one call of fn for {group: kernel-name stems}, from torch.profiler's device events; {} where it
    records none"""
    from torch.profiler import profile, ProfilerActivity
    try:
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        out = {}
        for ev in prof.key_averages():
            total = getattr(ev, 'device_time_total', 0) or getattr(ev, 'cuda_time_total', 0)
            for group, stems in groups.items():
                if any(stem in ev.key for stem in stems) and ev.count and total:
                    n, t = out.get(group, (0, 0.0))
                    out[group] = (n + ev.count, t + total / 1e3)
        return out
    except Exception as e:          # a profiler that cannot attach is no reason to lose the table
        print(f'torch.profiler: {e!r}', flush=True)
        return {}


def scalable_table(a, x, lines):
    groups = dict(fold=('kmpar_fold_kernel', 'kmpar_pot_kernel'), select=('kmpar_select_',), weights=('kmpar_weights_kernel',),
                  recluster=('kmpar_recluster_kernel',), maximum=('tok_amax_kernel', 'kmpar_init_kernel'))
    for k, V in ((8, 4096), (16, 1024)):
        tok = E.EcgTokenizer(k=k, pad='shift')
        st = tok._record_store(x, None, None)
        nseg = st.C * st.n_seg
        init = E.ScalableKMeansPlusPlus()
        T, R, ell, cap = init.plan(V)
        ids, means, dist = st.new(torch.int32), st.new(torch.float32), st.new(torch.float32)
        ws = torch.empty(lib().ecgvit_tok_workspace(V, k) // 8, dtype=torch.int64, device='cuda')
        got = {}

        def scalable():
            first, keys, u0, u53 = tok._scalable_draws(np.random.default_rng(27), nseg, V, T, R)
            got['s'] = tok._seed_scalable(st, V, T, R, ell, cap, first, keys, u0, u53)

        def plus():
            first, u53 = tok._seed_draws(np.random.default_rng(27), nseg, V, T)
            got['p'] = tok._seed(st, V, T, first, u53)

        def quality(table):
            """-> (the seeding's full-store potential, the inertia after ten Lloyd iterations from it)"""
            tok._assign(st, table, ids, means, dist=dist)
            pot = float(dist.sum(dtype=torch.float64))
            table, _, _, _ = tok._lloyd(st, table.clone(), 10, ws, dict(amax=False))
            tok._assign(st, table, ids, means, dist=dist)
            return pot, float(dist.sum(dtype=torch.float64))
        small = tok._record_store(x[:64], None, None)                 # warm-up: every kernel of both seedings once, at a small size
        f_, k_, u0_, u_ = tok._scalable_draws(np.random.default_rng(1), small.C * small.n_seg, 64, 6, R)
        tok._seed_scalable(small, 64, 6, R, 128, 224, f_, k_, u0_, u_)
        tok._seed(small, 64, 6, *tok._seed_draws(np.random.default_rng(1), small.C * small.n_seg, 64, 6))
        t_runs = [timed(scalable, 1, warmup=0) for _ in range(2)]      # twice: the spread of a run beside the difference the table reports
        t_s = min(t_runs)
        n_c, selected, truncated, _ = tok._scalable_info(got['s'][4], init, V)
        split = kernel_totals(scalable, groups)
        t_p = timed(plus, 1, warmup=0)
        pot_s, inertia_s = quality(got['s'][0])
        pot_p, inertia_p = quality(got['p'][0])
        lines.append(f'(g) k = {k}, V = {V}, T = {T}, ell = {ell}, {R} rounds, cap {cap}: {nseg} segments')
        lines.append(f'    scalable seeding, whole  {t_s / 1e3:10.3f} s   (the faster of two runs: {", ".join(f"{t / 1e3:.3f}" for t in t_runs)} s; selected per round {selected.tolist()}, dropped at the cap {truncated.tolist()}, '
                     f'{n_c} candidates)')
        if split:
            lines.append('    its kernels (torch.profiler, a second run): ' + ', '.join(
                f'{g} {split[g][1] / 1e3:.3f} s in {split[g][0]} launches' for g in groups if g in split))
        else:
            lines.append('    its kernels              not taken: torch.profiler recorded no kernel of the seeding')
        lines.append(f'(h) KMeansPlusPlus seeding   {t_p / 1e3:10.3f} s   = {t_p / V:8.3f} ms per centre (one run, the same store and T); scalable = x {t_s / t_p:.3f} of it')
        lines.append(f'(i) full-store potential     scalable {pot_s:.6e}, k-means++ {pot_p:.6e} (ratio {pot_s / pot_p:.4f}); inertia after ten Lloyd iterations '
                     f'scalable {inertia_s:.6e}, k-means++ {inertia_p:.6e} (ratio {inertia_s / inertia_p:.4f})')
        print('\n'.join(lines[-5:]), flush=True)
        del ids, means, dist, got


def seed_table(a, x, lines):
    for k, V in ((8, 4096), (16, 1024)):
        tok = E.EcgTokenizer(k=k, pad='shift')
        st = tok._record_store(x, None, None)
        nseg = st.C * st.n_seg
        T = E.KMeansPlusPlus().trials(V)
        rng = np.random.default_rng(25)

        def seeding(v):
            first, u53 = tok._seed_draws(rng, nseg, v, T)
            tok._seed(st, v, T, first, u53)
        t_whole = timed(lambda: seeding(V), 1, warmup=0)
        t1, t9 = timed(lambda: seeding(1), a.reps), timed(lambda: seeding(9), a.reps)
        pair = (t9 - t1) / 8
        split = kernel_split(lambda: seeding(9))
        table = tok._random_init(st, T + 1, np.random.default_rng(25))
        ids, means = st.new(torch.int32), st.new(torch.float32)
        t_assign = timed(lambda: tok._assign(st, table, ids, means), a.reps)
        lines.append(f'(d) k = {k}, V = {V}, T = {T}: {nseg} segments')
        lines.append(f'    whole seeding            {t_whole / 1e3:10.2f} s   = {t_whole / V:8.3f} ms per centre (one run, the sweep for the maximum included)')
        lines.append(f'    sweep + pick             {pair:10.3f} ms  {nseg / pair / 1e3:9.1f} M segments/s  ({(x.numel() * 4 + 8 * nseg) / 1e9 / (pair * 1e-3):7.0f} GB/s over the store and closest)')
        if split:
            lines.append('    apart (torch.profiler)   ' + ', '.join(f'{name} {us / 1e3:.3f} ms' for name, us in sorted(split.items())))
        else:
            lines.append('    apart                    not taken: torch.profiler recorded no kernel of the seeding')
        lines.append(f'(e) ecgvit_tok_assign, a {T + 1}-row table, the same store: {t_assign:10.3f} ms; sweep + pick = x {pair / t_assign:.2f} of it')
        print('\n'.join(lines[-5:]), flush=True)
        del ids, means
    # (f) the host's route, at a size the host finishes
    k, V, rec = 8, 256, 267                      # 267 x 12 x 626 = 2 005 704 segments
    tok = E.EcgTokenizer(k=k, pad='shift')
    sub = x[:rec].contiguous()
    st = tok._record_store(sub, None, None)
    T = E.KMeansPlusPlus().trials(V)

    def small():
        first, u53 = tok._seed_draws(np.random.default_rng(25), st.C * st.n_seg, V, T)
        tok._seed(st, V, T, first, u53)
    t_dev = timed(small, a.reps)
    try:
        from sklearn.cluster import kmeans_plusplus
        T_ = sub.shape[-1] // k
        host = sub[..., :T_ * k].reshape(-1, k)
        host = (host - host.mean(dim=1, keepdim=True)).cpu().numpy().astype(np.float64)
        t0 = time.perf_counter()
        kmeans_plusplus(host, V, random_state=25)
        t_host = (time.perf_counter() - t0) * 1e3
        lines.append(f'(f) k = {k}, V = {V}, T = {T}: sklearn.cluster.kmeans_plusplus on the host, {len(host)} whole segments (f64): {t_host / 1e3:8.2f} s; '
                     f'the device, {st.C * st.n_seg} segments: {t_dev:8.2f} ms = x {t_host / t_dev:.0f}')
    except ImportError:
        lines.append(f'(f) sklearn is not installed here: no host row (the device, {st.C * st.n_seg} segments, V = {V}: {t_dev:8.2f} ms)')
    print(lines[-1], flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--records', type=int, default=21837)
    ap.add_argument('--seed', action='store_true', help='time the k-means++ seeding instead (profiles/r25_tokenizer_seed.txt)')
    ap.add_argument('--scalable', action='store_true', help='time the scalable k-means++ seeding instead (profiles/r27_tokenizer_scalable.txt)')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if a.seed and a.scalable:
        ap.error('--seed and --scalable are tables of their own: one at a time')
    a.out = a.out or os.path.join(ROOT, 'profiles', 'r27_tokenizer_scalable.txt' if a.scalable else 'r25_tokenizer_seed.txt' if a.seed else 'r19_tokenizer.txt')
    import bench
    n = a.records
    g = torch.Generator(device='cuda').manual_seed(19)
    x = torch.randn((n, C, L), device='cuda', generator=g).mul_(0.7).add_(0.3)
    lines = [f'sources: bench.kernel_source_hash() = {bench.kernel_source_hash()}; {torch.cuda.get_device_name(0)}',
             f'store: {n} x {C} x {L} f32 = {x.numel() * 4 / 1e9:.2f} GB, N(0.3, 0.7^2); {a.reps} launches after one warm-up']
    if a.seed:
        seed_table(a, x, lines)
    if a.scalable:
        lines[-1] = lines[-1].replace(f'{a.reps} launches after one warm-up', 'every seeding timed once, after a warm-up of its kernels on 64 records')
        scalable_table(a, x, lines)
    for k, V in (() if a.seed or a.scalable else ((8, 4096), (16, 1024))):
        tok = E.EcgTokenizer(k=k, pad='shift')
        st = tok._record_store(x, None, None)
        nseg = st.C * st.n_seg
        table = tok._random_init(st, V, np.random.default_rng(19))
        ids, means, dist = st.new(torch.int32), st.new(torch.float32), st.new(torch.float32)
        changed = torch.zeros(1, dtype=torch.int64, device='cuda')
        lens = torch.zeros(V, dtype=torch.int64, device='cuda')
        ws = torch.empty(lib().ecgvit_tok_workspace(V, k) // 8, dtype=torch.int64, device='cuda')
        work = table.clone()
        t_assign = timed(lambda: tok._assign(st, table, ids, means), a.reps)
        # (b) torch on the same device, same store, same table -- compared before anything below overwrites ids
        T = st.dst_stride
        segs = x[..., :(T - 1) * k].reshape(-1, k)
        segs = (segs - segs.mean(dim=1, keepdim=True)).contiguous()
        chunk = 65536
        out = torch.empty(len(segs), dtype=torch.int64, device='cuda')

        def by_torch():
            for i in range(0, len(segs), chunk):
                out[i:i + chunk] = torch.cdist(segs[i:i + chunk], table).argmin(dim=1)
        t_torch = timed(by_torch, 1, warmup=0) * nseg / len(segs)
        agree = float((out.view(n, C, T - 1) == ids[..., :T - 1]).float().mean())
        t_update = timed(lambda: tok._update(st, ids, work, lens, ws), a.reps)
        t_update_kept = timed(lambda: tok._update(st, ids, work, lens, ws, keep_amax=True), a.reps)

        def lloyd():
            tok._assign(st, work, ids, means, dist=dist, prev_ids=ids, changed=changed)
            changed.item()
            tok._update(st, ids, work, lens, ws, keep_amax=True)
        t_lloyd = timed(lloyd, a.reps)
        flops = 2.0 * k * V * nseg
        lines.append(f'(a) k = {k}, V = {V}: {nseg} segments')
        lines.append(f'    assign                   {t_assign:10.2f} ms  {nseg / t_assign / 1e3:9.1f} M segments/s  score product {flops / t_assign / 1e9:7.1f} TFLOP/s '
                     f'= {flops / (t_assign * 1e-3) / F32_MATRIX_PEAK:.2f} of the f32 matrix peak')
        lines.append(f'    update                   {t_update:10.2f} ms  {nseg / t_update / 1e3:9.1f} M segments/s  ({2 * x.numel() * 4 / 1e9 / (t_update * 1e-3):7.0f} GB/s over its two sweeps)')
        lines.append(f'    update, maximum kept     {t_update_kept:10.2f} ms  {nseg / t_update_kept / 1e3:9.1f} M segments/s  (one sweep; what every update of a fit after the first costs)')
        lines.append(f'    Lloyd iteration          {t_lloyd:10.2f} ms  (assign with dist and the changed counter + 8-byte read + update, maximum kept)')
        print('\n'.join(lines[-7:]), flush=True)
        lines.append(f'(b) torch.cdist(...).argmin, chunks of {chunk} segments, {len(segs)} whole segments scaled to {nseg}: {t_torch:10.2f} ms = x {t_torch / t_assign:.1f} assign')
        lines.append(f'    (same ids as assign against the same table on {agree:.6f} of those segments)')
        # (c) the reference's route on the host
        try:
            from sklearn.neighbors import KDTree
            host = segs[:max(1, nseg // 100)].cpu().numpy().astype(np.float64)
            tree = KDTree(table.cpu().numpy().astype(np.float64))
            t0 = time.perf_counter()
            tree.query(host, k=1, return_distance=True)
            t_kd = (time.perf_counter() - t0) * 1e3 * nseg / len(host)
            lines.append(f'(c) sklearn KDTree.query on the host, {len(host)} segments (f64) scaled to {nseg}: {t_kd / 1e3:10.1f} s = x {t_kd / t_assign:.0f} assign')
        except ImportError:
            lines.append('(c) sklearn is not installed here: no host row')
        print(lines[-1], flush=True)
        del ids, means, dist, segs, out
    text = '\n'.join(lines) + '\n'
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as fh:
        fh.write(text)


if __name__ == '__main__':
    main()
