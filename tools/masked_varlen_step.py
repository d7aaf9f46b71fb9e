#!/usr/bin/env python3
"""The masked pre-train step over records of unequal length against the zero-padded rectangular step, one GPU process, bf16, the base
config's dropout, records/s of three forms run alternately:
  padded  -- step_masked on the zero-padded (B, 12, 5000) batch with (B, m) indices (the rectangular step: the padding takes part in it)
  lengths -- the same batch with lengths=, flat mask_idx and mask_counts (padded rows, computed as zeros)
  ragged  -- (12, S) + lengths (packed rows only)
at the three mixes of tools/ragged_step.py: EcgVit-base, patch 4, B = 32, records uniform in [n/4, n] patches; patch 20, B = 512, lengths
uniform in [50 %, 100 %] of 5000 samples; and a near-full mix (every record >= 95 % of the width).
Writes profiles/r14_masked_varlen_step.txt (--out).
usage: python tools/masked_varlen_step.py [--runs 2] [--steps 5] [--warmup 2]"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import ecg_representation_learning_amd as E  # noqa: E402
from ragged_step import CASES, L, draw_lengths  # noqa: E402


def timed_steps(step, x, kw, steps, warmup, B):
    for _ in range(warmup):
        step.step_masked(x, **kw)
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(steps):
        step.step_masked(x, **kw)
    t1.record()
    torch.cuda.synchronize()
    return steps * B / (t0.elapsed_time(t1) / 1e3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=2)
    ap.add_argument('--steps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r14_masked_varlen_step.txt'))
    a = ap.parse_args()
    import bench
    lines = [f'sources: bench.kernel_source_hash() = {bench.kernel_source_hash()}; {torch.cuda.get_device_name(0)}',
             f'fused masked pre-train step (mask ratio 0.5), bf16, dropout of the base config, {a.steps} steps per run after {a.warmup} warm-up steps, '
             f'{a.runs} alternating runs (records/s); padded = zero-padded (B, 12, {L}) with (B, m) indices, lengths = the same batch with lengths= / '
             f'flat mask_idx / mask_counts, ragged = (12, S) + lengths']
    for ci, (name, P, B, lo) in enumerate(CASES):
        conf, _ = bench.make_config(E, 'base', P, L, None)
        torch.manual_seed(0)
        model = E.MaskedEcgVit(E.EcgVit(config=conf, compute_dtype=torch.bfloat16), mask_ratio=0.5).cuda().train()
        lengths = draw_lengths(B, P, lo, seed=1 + ci)
        g = torch.Generator().manual_seed(2 + ci)
        x = torch.randn(B, 12, L, generator=g)
        for b in range(B):
            x[b, :, int(lengths[b]):] = 0.0
        xr = torch.cat([x[b, :, :int(lengths[b])] for b in range(B)], dim=1).contiguous().cuda()
        x = x.cuda()
        idx2 = model.random_mask_indices(B, generator=g)
        idx, counts = model.random_mask_indices_varlen(lengths, generator=g)
        step = E.HipTrainStep(model, dict(n_step=10 ** 6), sync_nonfinite=False)
        forms = (('padded', x, dict(mask_idx=idx2)), ('lengths', x, dict(mask_idx=idx, lengths=lengths, mask_counts=counts)),
                 ('ragged', xr, dict(mask_idx=idx, lengths=lengths, mask_counts=counts)))
        res = {f: [] for f, _, _ in forms}
        for r in range(a.runs):
            for tag, xx, kw in (forms if r % 2 == 0 else forms[::-1]):
                res[tag].append(timed_steps(step, xx, kw, a.steps, a.warmup, B))
                print(f'{name}: run {r} {tag:8s} {res[tag][-1]:8.1f} records/s', flush=True)
        step.finish()
        n = L // P
        valid = float((lengths // P).float().mean())
        lines.append(f'  {name}: dropout {conf.hidden_dropout_prob}, n = {n} patch tokens (no CLS row), mean valid tokens {valid:.0f} '
                     f'(valid-row fraction {valid / n:.3f}), masked rows {int(counts.sum())} against {idx2.numel()} padded')
        for tag in res:
            v = res[tag]
            lines.append(f'    {tag:8s} ' + ' '.join(f'{r:8.1f}' for r in v) + f'   best {max(v):8.1f}   x {max(v) / max(res["padded"]):.3f} of padded'
                         f'   per run x ' + ' '.join(f'{r / q:.3f}' for r, q in zip(v, res['padded'])))
        del step, model, x, xr
        torch.cuda.empty_cache()
    text = '\n'.join(lines) + '\n'
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as fh:
        fh.write(text)


if __name__ == '__main__':
    main()
