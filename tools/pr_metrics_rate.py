#!/usr/bin/env python3
"""The precision-recall walk (csrc/pr_metrics.hip) beside the AUROC walk (csrc/rank_metrics.hip) at the same shape in the same run, and beside
scikit-learn's `average_precision_score` on the host.  Shapes: those of tools/rank_metrics_rate.py -- K = 71 classes at n = 2 200 (the PTB-XL test
fold), 21 837 (all of PTB-XL) and 350 000 records; scores on a grid of 4 096 values (ties), label rates 5 % .. 50 %.
Forms, each warmed up at the shape, then timed in `--reps` rounds that alternate the forms (host clock around a device synchronise; median and range
of the rounds).  The sort and the multiplicities are made once per shape, outside the clock: a walk is one launch.
  pr point      `ecgvit_pr_walk`, unit weights, one replicate
  auc point     `ecgvit_rank_walk`, unit weights, one replicate
  pr 1000       `ecgvit_pr_walk` over 1 000 seeded replicates, in the chunks `bootstrap_pr` would take (the multiplicities of every chunk are resident)
  auc 1000      `ecgvit_rank_walk` over the same multiplicities
  bootstrap_pr  `bootstrap_pr(n_boot=1000)` end to end: the sort, the point estimate, the fills, the walks, the read-back, the host's divisions
  host          `average_precision_score` per class on `--host-replicates` resamples (numpy draws), scaled to 1 000
Writes profiles/r30_pr_metrics.txt (--out).
--against LIB.so: the A/B of the four walk forms against another build of the library (`make prev` on the parent commit keeps one as
csrc/build/libecgvit_hip_prev.so), nothing else timed.  Both libraries walk the same resident sort and multiplicities into buffers of their own,
which must hold the same integers.  `--reps` + 1 rounds, the two libraries alternating within each round and taking turns to go first, the first
round discarded; a timing is HIP events around enough launches to fill about 20 ms.  A row passes when the shipped library's median is at most the
other's median plus the other's own spread (max - min over its rounds), the rule of tools/ln_ab.py.  Writes profiles/r33_walk_skeleton.txt (--out)
with both builds' register budgets; exit status 1 when a row is slower.
usage: python tools/pr_metrics_rate.py [--reps 5] [--host-replicates 5] [--against LIB.so]"""
import argparse
import ctypes
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ecg_representation_learning_amd as E  # noqa: E402
from ecg_representation_learning_amd import hip, pr_abi, pr_metrics, rank_abi, rank_metrics  # noqa: E402
from ecg_representation_learning_amd.hip import ptr, stream  # noqa: E402

K, N_BOOT = 71, 1000
SHAPES = (('the PTB-XL test fold', 2200), ('all of PTB-XL', 21837), ('a 350 000-record corpus', 350000))


def clock(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def walkers(path):
    """the two walks of the library at `path` as fn(ranked, mult, R, out), each launch checked"""
    lib = ctypes.CDLL(path)
    fns = {}
    for name, table in (('ecgvit_rank_walk', rank_abi.SIGNATURES), ('ecgvit_pr_walk', pr_abi.SIGNATURES)):
        fns[name] = getattr(lib, name)
        fns[name].restype, fns[name].argtypes = table[name]

    def auc(ranked, mult, R, out):
        assert fns['ecgvit_rank_walk'](ptr(ranked.packed), ptr(ranked.first_nan), ranked.n, ranked.K, ptr(mult), R, ptr(out), None, stream()) == 0

    def pr(ranked, mult, R, out):
        assert fns['ecgvit_pr_walk'](ptr(ranked.packed), ptr(ranked.first_nan), ranked.n, ranked.K, ptr(mult), R, ptr(out), stream()) == 0
    return dict(auc=auc, pr=pr)


def budgets(path):
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import code_objects
    return [f'    {name}: {k["vgpr_count"]} VGPRs, {k["agpr_count"]} AGPRs, {k["sgpr_count"]} SGPRs, spilled {k["vgpr_spill_count"]} + {k["sgpr_spill_count"]}, '
            f'scratch {k["private_segment_fixed_size"]}, LDS {k["group_segment_fixed_size"]}'
            for name, k in sorted(code_objects.kernels(path).items()) if 'walk_kernel' in name]


def against(builds, ranked, mults, reps):
    """builds: [(label, walkers)], the baseline first -> (the table's lines, whether every row passes)"""
    lines, ok = [], True
    for key, slots in (('pr', 6), ('auc', 3)):
        for form, chunks in (('point', [(0, 1, None)]), ('1000', mults)):
            R = chunks[-1][0] + chunks[-1][1]
            outs = [torch.full((R, ranked.K, slots), -7, dtype=torch.int64, device='cuda') for _ in builds]

            def run(i, out):
                for r0, rows, m in chunks:
                    builds[i][1][key](ranked, m, rows, out[r0:r0 + rows])
            once = max(clock(lambda: run(i, outs[i]))[0] for i in (0, 1))   # the warm-up of both builds at this shape, and the size of a launch
            assert torch.equal(outs[0], outs[1]) and int(outs[0][..., 1].min()) >= 0, f'{key} {form}: the two libraries\' integers differ'
            iters = max(1, min(50, int(20.0 / once)))
            ts = [[], []]
            for rnd in range(reps + 1):
                for i in ((0, 1) if rnd % 2 == 0 else (1, 0)):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(iters):
                        run(i, outs[0])                            # one buffer for both: two sit on different pages and channels (tools/ln_ab.py)
                    e1.record()
                    torch.cuda.synchronize()
                    ts[i].append(e0.elapsed_time(e1) / iters)
            v = [x[1:] for x in ts]
            med, spread = [statistics.median(x) for x in v], max(v[0]) - min(v[0])
            good = med[1] <= med[0] + spread
            ok &= good
            lines.append(f'    {key + " " + form:>12s} ' + '   '.join(f'{builds[i][0]} {med[i]:9.4f} ({min(v[i]):.4f} .. {max(v[i]):.4f})' for i in (0, 1)) +
                         f'   {iters:2d} launches a timing; difference {med[1] - med[0]:+.4f}, {builds[0][0]}\'s spread {spread:.4f}: {"ok" if good else "SLOWER"}; integers equal')
    return lines, ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--host-replicates', type=int, default=5)
    ap.add_argument('--against', metavar='LIB.so')
    ap.add_argument('--out')
    a = ap.parse_args()
    a.out = a.out or os.path.join(ROOT, 'profiles', 'r33_walk_skeleton.txt' if a.against else 'r30_pr_metrics.txt')
    import bench
    ok = True
    if a.against:
        builds = [('other', walkers(a.against)), ('shipped', walkers(hip.LIB_PATH))]
    else:
        from sklearn.metrics import average_precision_score
    fmt = lambda ts: f'{statistics.median(ts):10.3f} ({min(ts):.3f} .. {max(ts):.3f})'   # noqa: E731
    lines = [f'sources: bench.kernel_source_hash() = {bench.kernel_source_hash()}; {torch.cuda.get_device_name(0)}; torch {torch.__version__}',
             f'K = {K}; grid scores (4 096 values), label rates 5 % .. 50 %; {a.reps} alternating rounds per form after one warm-up of the shape; '
             f'milliseconds, median (min .. max); host clock around a device synchronise',
             f'walks: one launch each over resident sort and multiplicities; bootstrap_pr = bootstrap_pr(n_boot={N_BOOT}) end to end; '
             f'host = average_precision_score x {K} classes on {a.host_replicates} resamples, scaled to {N_BOOT}']
    if a.against:
        lines = [lines[0], f'K = {K}; grid scores (4 096 values), label rates 5 % .. 50 %; other = {os.path.relpath(a.against, ROOT)}, shipped = the package\'s library; '
                 f'one launch per walk (one per chunk of replicates) over resident sort and multiplicities; milliseconds per walk, median (min .. max) of '
                 f'{a.reps} rounds, the builds interleaved, after one round discarded; HIP events', 'other:'] + budgets(a.against) + ['shipped:'] + budgets(hip.LIB_PATH)
    rng = np.random.default_rng(30)
    for name, n in SHAPES:
        sc = (rng.integers(0, 4096, (n, K)) / 4096).astype(np.float32)
        yy = (rng.random((n, K)) < np.linspace(0.05, 0.5, K)).astype(np.float32)
        ds, dy = torch.from_numpy(sc).cuda(), torch.from_numpy(yy).cuda()
        ranked = E.rank_scores(ds, dy)
        quad = rank_abi.lib().ecgvit_rank_workspace(n, K, 4)
        chunk = max(1, min(N_BOOT, rank_metrics.DEFAULT_WORKSPACE_BYTES // quad * 4))
        mults = []
        for r0 in range(0, N_BOOT, chunk):
            rows = min(chunk, N_BOOT - r0)
            m = torch.empty(n, rank_metrics.pad4(rows), dtype=torch.int32, device='cuda')
            rank_abi.run.ecgvit_rank_multiplicities_seeded(30, r0, rows, n, ptr(m), stream())
            mults.append((r0, rows, m))
        if a.against:
            rows, good = against(builds, ranked, mults, a.reps)
            ok &= good
            lines += [f'n = {n} ({name}); replicates per chunk {chunk}'] + rows
            for line in lines[-5:]:
                print(line, flush=True)
            del ds, dy, ranked, mults
            torch.cuda.empty_cache()
            continue
        sixes = torch.empty(N_BOOT, K, 6, dtype=torch.int64, device='cuda')
        triples = torch.empty(N_BOOT, K, 3, dtype=torch.int64, device='cuda')

        def pr_all():
            for r0, rows, m in mults:
                pr_metrics._walk(ranked, m, rows, sixes[r0:r0 + rows])

        def auc_all():
            for r0, rows, m in mults:
                ranked._walk(m, rows, triples[r0:r0 + rows])
        forms = (('pr point', lambda: pr_metrics._walk(ranked, None, 1, sixes[:1])), ('auc point', lambda: ranked._walk(None, 1, triples[:1])),
                 ('pr 1000', pr_all), ('auc 1000', auc_all), ('bootstrap_pr', lambda: E.bootstrap_pr(ds, dy, n_boot=N_BOOT, seed=30)))
        out = {}
        for key, fn in forms:                                        # warm-up of every form at this shape
            out[key] = clock(fn)[1]
        res = out['bootstrap_pr']
        same = bool(np.array_equal(res.sixes, sixes.cpu().numpy()))
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
                average_precision_score(y_b[:, c], s_b[:, c])
        host = (time.perf_counter() - t0) * 1e3 * N_BOOT / a.host_replicates
        med = {key: statistics.median(v) for key, v in ts.items()}
        (alo, ahi), (flo, fhi) = res.ci('ap'), res.ci('fmax')
        lines += [f'n = {n} ({name}); macro AP {res.point["macro_ap"]:.4f}, 95 % interval {alo:.4f} .. {ahi:.4f}; macro F-max {res.point["macro_fmax"]:.4f}, '
                  f'95 % interval {flo:.4f} .. {fhi:.4f}; replicates per chunk {res.chunk}; the timed walks hold bootstrap_pr\'s integers: {same}']
        lines += [f'    {key:>12s} {fmt(ts[key])}' for key, _ in forms]
        lines += [f'    {"host":>12s} {host:10.1f} (scaled from {a.host_replicates} replicates)',
                  f'    pr point / auc point = {med["pr point"] / med["auc point"]:.2f}; pr 1000 / auc 1000 = {med["pr 1000"] / med["auc 1000"]:.2f}; '
                  f'host / bootstrap_pr = {host / med["bootstrap_pr"]:.1f}; pr walk visits per second = {N_BOOT * K * n / (med["pr 1000"] * 1e-3):.3e}']
        for line in lines[-8:]:
            print(line, flush=True)
        del ds, dy, ranked, mults, sixes, triples, out, res
        torch.cuda.empty_cache()
    text = '\n'.join(lines) + '\n'
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as fh:
        fh.write(text)
    sys.exit(0 if ok else 1)


if __name__ == '__main__':
    main()
