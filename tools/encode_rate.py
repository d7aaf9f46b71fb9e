#!/usr/bin/env python3
"""Pooled representations and the probe on cached features, one GPU process:
  (a) `ecgvit_pool_records` (mean pool) against torch's own `x.view(B, N, d).float().mean(1)` on the same tensor, us per launch and the
      fraction of bytes read / 8 TB/s, at the base shape (B = 512, N = 251, d = 768, bf16) and at few long records (B = 16, N = 2049,
      d = 1024, bf16), every launch on another tensor of a ring larger than the Infinity Cache.  The kernel must not be slower than the
      torch expression at either shape (the tool exits non-zero if it is);
  (b) `EcgVit.encode` records/s, EcgVit-base, bf16, B = 512 records of 5000 samples: pool='cls' (pruned last block) and pool='mean' (full last
      block), beside `HipEvaluator`'s forward over the same batch;
  (c) `HipProbeStep` on cached features, B = 512, records/s, beside the existing linear probe (`HipTrainStep` with every parameter but the
      head frozen, re-measured in the same run), and the one-off cost of the encode pass the cached features presuppose.
Writes profiles/r16_encode.txt (--out).
usage: python tools/encode_rate.py [--runs 3] [--steps 10] [--warmup 3]"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ecg_representation_learning_amd as E  # noqa: E402
from ecg_representation_learning_amd import hip  # noqa: E402
from ecg_representation_learning_amd.hip import lib, check, ptr, stream  # noqa: E402

B, LENGTH = 512, 5000
HBM = 8.0e12


def timed(fn, reps, warmup=3):
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


def kernel_rows(runs, reps=50):
    lines, lost = [], []
    for (b, n, d) in ((512, 251, 768), (16, 2049, 1024)):
        nbytes = b * n * d * 2
        # launches walk a ring of distinct tensors larger than the 256-MB Infinity Cache together, so every launch streams from HBM
        ring = [torch.randn(b * n, d, device='cuda').to(torch.bfloat16) for _ in range(-(-640 * 2 ** 20 // nbytes))]
        out = torch.empty(b, d, device='cuda')
        turn = [0, 0]

        def ours():
            turn[0] += 1
            check(lib().ecgvit_pool_records(ptr(ring[turn[0] % len(ring)]), ptr(out), None, None, b, n, d, hip.POOL_MEAN, None, None, 1e-5, hip.BF16,
                                            stream()), 'pool_records')

        def ref():
            turn[1] += 1
            return ring[turn[1] % len(ring)].view(b, n, d).float().mean(1)
        turn[0] = turn[1] = 0
        ours()
        err = float((out - ref()).abs().max())
        tk, tt = [], []
        for r in range(runs):
            for which in ((0, 1) if r % 2 == 0 else (1, 0)):
                (tk if which == 0 else tt).append(timed(ours if which == 0 else ref, reps))
        k, t = min(tk), min(tt)
        lines.append(f'    B = {b:3d}, N = {n:4d}, d = {d:4d}, bf16 ({nbytes / 1e6:.1f} MB read): ecgvit_pool_records ' + ' '.join(f'{v:7.1f}' for v in tk)
                     + f'  best {k:7.1f} us = {nbytes / (k * 1e-6) / HBM:.3f} of 8 TB/s;  torch ' + ' '.join(f'{v:7.1f}' for v in tt)
                     + f'  best {t:7.1f} us = {nbytes / (t * 1e-6) / HBM:.3f};  kernel / torch {k / t:.3f}  (max |difference| {err:.1e})')
        if k > t:
            lost.append((b, n, d, k, t))
        del ring, out
    return lines, lost


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=3)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r16_encode.txt'))
    a = ap.parse_args()
    import bench
    lines = [f'sources: bench.kernel_source_hash() = {bench.kernel_source_hash()}; {torch.cuda.get_device_name(0)}',
             f'(a) mean pool over token rows, us per launch, {a.runs} alternating runs of 50 launches over a ring of tensors past the 256-MB Infinity Cache (torch: x.view(B, N, d).float().mean(1) on the same tensor)']
    rows, lost = kernel_rows(a.runs)
    lines += rows

    conf, _ = bench.make_config(E, 'base', 20, LENGTH, None)
    torch.manual_seed(0)
    model = E.EcgVit(config=conf, compute_dtype=torch.bfloat16).cuda().train()
    x, y = E.workload.synthetic_batch(B, length=LENGTH, seed=77)
    x, y = x.cuda(), y.cuda()
    ev = E.HipEvaluator(model, eval_batch_size=B)
    passes = (('encode pool=cls (pruned last block)', lambda: model.encode(x)), ('encode pool=mean (full last block)', lambda: model.encode(x, pool='mean')),
              ('HipEvaluator.evaluate (forward + loss + counts)', lambda: ev.evaluate(x, y)))
    rate = {n: [] for n, _ in passes}
    for r in range(a.runs):
        for n, fn in (passes if r % 2 == 0 else passes[::-1]):
            rate[n].append(B / (timed(fn, a.steps, a.warmup) * 1e-6))
            print(f'run {r}: {n:48s} {rate[n][-1]:9.1f} records/s', flush=True)
    lines.append(f'(b) encoder pass, EcgVit-base, bf16, B = {B}, N = 251, eval mode, {a.steps} passes per run after {a.warmup} warm-up passes, {a.runs} alternating runs (records/s)')
    for n, _ in passes:
        lines.append(f'    {n:48s} ' + ' '.join(f'{v:9.1f}' for v in rate[n]) + f'   best {max(rate[n]):9.1f}')

    feats = model.encode(x, norm=False)
    head = lambda n: n.startswith('vit.mlp_head.')

    def probe_cached():
        st = E.HipProbeStep(model, dict(n_step=10 ** 6), sync_nonfinite=False)
        us = timed(lambda: st.step(feats, y), a.steps * 20, a.warmup)
        st.finish()
        return B / (us * 1e-6)

    def probe_full():
        for n, p in model.named_parameters():
            p.requires_grad_(head(n))
        st = E.HipTrainStep(model, dict(n_step=10 ** 6), sync_nonfinite=False)
        us = timed(lambda: st.step(x, y), a.steps, a.warmup)
        st.finish()
        for p in model.parameters():
            p.requires_grad_(True)
        return B / (us * 1e-6)
    steps = (('HipProbeStep on cached features', probe_cached), ('HipTrainStep, head alone trainable (linear probe)', probe_full))
    srate = {n: [] for n, _ in steps}
    for r in range(a.runs):
        for n, fn in (steps if r % 2 == 0 else steps[::-1]):
            srate[n].append(fn())
            print(f'run {r}: {n:48s} {srate[n][-1]:9.1f} records/s', flush=True)
    lines.append(f'(c) probe step, B = {B}, {a.runs} alternating runs (records/s; {a.steps * 20} steps per run on cached features, {a.steps} through the encoder)')
    for n, _ in steps:
        lines.append(f'    {n:48s} ' + ' '.join(f'{v:9.1f}' for v in srate[n]) + f'   best {max(srate[n]):9.1f}')
    pc, pf, enc = max(srate[steps[0][0]]), max(srate[steps[1][0]]), max(rate[passes[0][0]])
    lines.append(f'    cached / through the encoder: x {pc / pf:.1f} per step; the cache costs one encode pass at {enc:.0f} records/s '
                 f'(= {pf / enc:.2f} linear-probe epochs), paid once instead of every epoch')
    text = '\n'.join(lines) + '\n'
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as fh:
        fh.write(text)
    if lost:
        print('ecgvit_pool_records is SLOWER than the torch expression at', lost)
        sys.exit(1)


if __name__ == '__main__':
    main()
