#!/usr/bin/env python3
"""Ragged batches (records concatenated along time, (C, S) + lengths) against the padded forms, one GPU process:
  (a) the fused supervised step, bf16, records/s of three forms run alternately: padded (zero-padded to the width, no lengths), padded with
      `lengths=`, and ragged -- at the r10 shape (EcgVit-base, patch 4, N = 1251, B = 32, records uniform in [n/4, n] patches: mean 784
      valid tokens), at EcgVit-base, patch 20, B = 512 with lengths uniform in [50 %, 100 %] of 5000 samples, and at a near-full mix (every
      record >= 95 % of the width: the padded step keeps its CLS-only last block there);
  (b) the packed attention kernels against the padded varlen ones at the r10 shape (us per launch, dropout 0.1).
Writes profiles/r13_ragged_step.txt (--out).
usage: python tools/ragged_step.py [--runs 2] [--steps 5] [--warmup 2]"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ecg_representation_learning_amd as E  # noqa: E402
from ecg_representation_learning_amd.hip import lib, check, ptr, stream  # noqa: E402

L = 5000
CASES = (('r10: base, patch 4, B = 32, [n/4, n] patches', 4, 32, 0.25),
         ('base, patch 20, B = 512, [50 %, 100 %] of 5000', 20, 512, 0.5),
         ('near-full: base, patch 20, B = 512, [95 %, 100 %]', 20, 512, 0.95))


def draw_lengths(B, P, lo_frac, seed):
    n = L // P
    g = torch.Generator().manual_seed(seed)
    lo = max(1, int(n * lo_frac)) if lo_frac > 0.25 else (n - 1) // 4   # (r10 drew randint((N - 1) // 4, N) patches)
    return torch.randint(lo, n + 1, (B,), generator=g) * P


def timed_steps(step, x, y, lengths, steps, warmup, B):
    for _ in range(warmup):
        step.step(x, y, lengths=lengths)
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(steps):
        step.step(x, y, lengths=lengths)
    t1.record()
    torch.cuda.synchronize()
    return steps * B / (t0.elapsed_time(t1) / 1e3)


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) * 1e3 / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=2)
    ap.add_argument('--steps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r13_ragged_step.txt'))
    a = ap.parse_args()
    import bench
    lines = [f'sources: bench.kernel_source_hash() = {bench.kernel_source_hash()}; {torch.cuda.get_device_name(0)}',
             f'(a) fused supervised step, bf16, dropout of the base config, {a.steps} steps per run after {a.warmup} warm-up steps, {a.runs} alternating runs '
             f'(records/s); padded = zero-padded (B, 12, {L}), lengths = the same with lengths=, ragged = (12, S) + lengths']
    for ci, (name, P, B, lo) in enumerate(CASES):
        conf, _ = bench.make_config(E, 'base', P, L, None)
        torch.manual_seed(0)
        model = E.EcgVit(config=conf, compute_dtype=torch.bfloat16).cuda().train()
        lengths = draw_lengths(B, P, lo, seed=1 + ci)
        g = torch.Generator().manual_seed(2 + ci)
        x = torch.randn(B, 12, L, generator=g)
        for b in range(B):
            x[b, :, int(lengths[b]):] = 0.0
        xr = torch.cat([x[b, :, :int(lengths[b])] for b in range(B)], dim=1).contiguous().cuda()
        x, y = x.cuda(), (torch.rand(B, 71, generator=g) < 0.05).float().cuda()
        step = E.HipTrainStep(model, dict(n_step=10 ** 6), sync_nonfinite=False)
        forms = (('padded', x, None), ('lengths', x, lengths), ('ragged', xr, lengths))
        res = {f: [] for f, _, _ in forms}
        for r in range(a.runs):
            for tag, xx, ln in (forms if r % 2 == 0 else forms[::-1]):
                res[tag].append(timed_steps(step, xx, y, ln, a.steps, a.warmup, B))
                print(f'{name}: run {r} {tag:8s} {res[tag][-1]:8.1f} records/s', flush=True)
        step.finish()
        n = L // P
        valid = float((lengths // P + 1).float().mean())
        lines.append(f'  {name}: dropout {conf.hidden_dropout_prob}, N = {n + 1}, mean valid tokens {valid:.0f} of {n + 1} (valid-row fraction {valid / (n + 1):.3f})')
        for tag in res:
            v = res[tag]
            lines.append(f'    {tag:8s} ' + ' '.join(f'{r:8.1f}' for r in v) + f'   best {max(v):8.1f}   x {max(v) / max(res["padded"]):.3f} of padded'
                         f'   x {max(v) / max(res["lengths"]):.3f} of lengths')
        del step, model, x, xr, y
        torch.cuda.empty_cache()

    # (b) attention kernels at the r10 shape
    B, N, h, dh, p, reps = 32, 1251, 12, 64, 0.1, 20
    d, sc = h * dh, dh ** -0.5
    nt = (draw_lengths(B, 4, 0.25, seed=1) // 4 + 1).to(torch.int32)
    off = (torch.cumsum(nt.long(), 0) - nt.long()).to(torch.int32)
    M = int(nt.sum())
    ntd, offd = nt.cuda(), off.cuda()
    qkv = torch.randn(B * N, 3 * d, device='cuda').to(torch.bfloat16)
    o = torch.empty(B * N, d, device='cuda', dtype=torch.bfloat16)
    do = torch.randn(B * N, d, device='cuda').to(torch.bfloat16)
    lse = torch.empty(B * h * N, device='cuda')
    dqkv = torch.empty_like(qkv)
    fv = lambda: check(lib().ecgvit_attention_varlen_fwd(ptr(qkv), ptr(o), ptr(lse), ptr(ntd), B, N, h, dh, sc, p, 7, stream()), 'vfwd')
    bv = lambda: check(lib().ecgvit_attention_varlen_bwd(ptr(qkv), ptr(o), ptr(do), ptr(lse), ptr(dqkv), ptr(ntd), B, N, h, dh, sc, p, 7, stream()), 'vbwd')
    fr = lambda: check(lib().ecgvit_attention_ragged_fwd(ptr(qkv), ptr(o), ptr(lse), ptr(ntd), ptr(offd), B, N, h, dh, sc, p, 7, stream()), 'rfwd')
    br = lambda: check(lib().ecgvit_attention_ragged_bwd(ptr(qkv), ptr(o), ptr(do), ptr(lse), ptr(dqkv), ptr(ntd), ptr(offd), B, N, h, dh, sc, p, 7,
                                                         stream()), 'rbwd')
    t = [timed(f, reps) for f in (fv, fr, bv, br, fv, fr, bv, br)]
    lines.append(f'(b) attention at the r10 shape (B = {B}, N = {N}, {M} valid rows of {B * N}, h = {h}, dh = {dh}, dropout {p}), us per launch, two '
                 f'alternating passes of {reps} launches')
    lines.append(f'    forward   padded varlen {t[0]:8.1f} {t[4]:8.1f}   packed {t[1]:8.1f} {t[5]:8.1f}   packed / padded {min(t[1], t[5]) / min(t[0], t[4]):.3f}')
    lines.append(f'    backward  padded varlen {t[2]:8.1f} {t[6]:8.1f}   packed {t[3]:8.1f} {t[7]:8.1f}   packed / padded {min(t[3], t[7]) / min(t[2], t[6]):.3f}')
    text = '\n'.join(lines) + '\n'
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as fh:
        fh.write(text)


if __name__ == '__main__':
    main()
