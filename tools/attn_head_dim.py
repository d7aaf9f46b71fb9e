#!/usr/bin/env python3
"""128-wide against 64-wide attention heads at equal (B, N, d), in ONE process on one device: the fused forward and backward per launch (dh = 128:
the uniform form of attn_varlen_kernels.h; dh = 64: attention.hip) at 512 x 251 (d 768), 256 x 501 and 64 x 1251 (d 1024), then one whole supervised step of EcgVit-base
(d 768, 12 heads) against the same model with 6 heads through HipTrainStep.step at 251 and 1251 tokens.
usage: python tools/attn_head_dim.py [reps] [p]      (output: profiles/r09_attn_head_dim.txt)"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ecg_representation_learning_amd as E  # noqa: E402
from ecg_representation_learning_amd import hip  # noqa: E402
from ecg_representation_learning_amd.hip import lib, check, ptr, stream  # noqa: E402
from ecg_representation_learning_amd.workload import synthetic_batch  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
p = float(sys.argv[2]) if len(sys.argv) > 2 else 0.1
SHAPES = [(512, 251, 768), (256, 501, 1024), (64, 1251, 1024)]   # (B, N, d)


def attn_times(B, N, d, dh):
    h = d // dh
    torch.manual_seed(3)
    qkv = torch.randn(B * N, 3 * d, device='cuda').to(torch.bfloat16)
    out = torch.empty(B * N, d, device='cuda', dtype=torch.bfloat16)
    do = torch.randn(B * N, d, device='cuda').to(torch.bfloat16)
    lse = torch.empty(B * h * N, device='cuda')
    dqkv = torch.empty(B * N, 3 * d, device='cuda', dtype=torch.bfloat16)
    sc = dh ** -0.5
    fwd = lambda: check(lib().ecgvit_attention_fwd(ptr(qkv), ptr(out), ptr(lse), B, N, h, dh, sc, p, 7, hip.BF16, stream()), 'fwd')
    bwd = lambda: check(lib().ecgvit_attention_bwd(ptr(qkv), ptr(out), ptr(do), ptr(lse), ptr(dqkv), B, N, h, dh, sc, p, 7, hip.BF16, stream()), 'bwd')
    e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    for _ in range(2):
        fwd()
        bwd()
    e[0].record()
    for _ in range(reps):
        fwd()
    e[1].record()
    for _ in range(reps):
        bwd()
    e[2].record()
    torch.cuda.synchronize()
    return 1e3 * e[0].elapsed_time(e[1]) / reps, 1e3 * e[1].elapsed_time(e[2]) / reps


def step_ms(heads, N, batch, steps):
    conf = E.EcgVitConfig.from_defined('ecg-vit-base')
    conf.max_signal_length, conf.patch_size = 5000, 5000 // (N - 1)   # 10 s at 500 Hz, patch 20 -> 251 tokens, patch 4 -> 1251
    conf.num_attention_heads = heads
    torch.manual_seed(0)
    m = E.EcgVit(config=conf, compute_dtype=torch.bfloat16).cuda().train()
    step = E.HipTrainStep(m, dict(n_step=1000))
    x, y = synthetic_batch(batch, length=conf.max_signal_length, seed=1)
    x, y = x.cuda(), y.cuda()
    for _ in range(3):
        step.step(x, y)
    torch.cuda.synchronize()
    e = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    e[0].record()
    for _ in range(steps):
        step.step(x, y)
    e[1].record()
    torch.cuda.synchronize()
    step.finish()
    assert m._engine().dh == conf.hidden_size // heads and m._engine().N == N
    del m, step
    torch.cuda.empty_cache()
    return e[0].elapsed_time(e[1]) / steps


print(f'# fused attention per launch, dh 128 against dh 64 at equal (B, N, d); dropout p = {p}, {reps} launches each, one MI355X, one process')
print(f'{"B x N, d":>18} {"h":>6} {"fwd us":>16} {"bwd us":>16} {"fwd 128/64":>11} {"bwd 128/64":>11}')
for B, N, d in SHAPES:
    t = {dh: attn_times(B, N, d, dh) for dh in (64, 128)}
    torch.cuda.empty_cache()
    print(f'{f"{B} x {N}, {d}":>18} {f"{d // 64}/{d // 128}":>6} {f"{t[64][0]:.1f}/{t[128][0]:.1f}":>16} {f"{t[64][1]:.1f}/{t[128][1]:.1f}":>16} '
          f'{t[128][0] / t[64][0]:>11.3f} {t[128][1] / t[64][1]:>11.3f}', flush=True)

print('\n# whole supervised step (HipTrainStep.step, pruned last block), EcgVit-base d 768: 12 heads (dh 64) against 6 heads (dh 128)')
print(f'{"N":>6} {"batch":>6} {"12 heads ms":>12} {"6 heads ms":>12} {"6/12":>7}')
for N, batch in ((251, 512), (1251, 64)):
    t12, t6 = step_ms(12, N, batch, 5), step_ms(6, N, batch, 5)
    print(f'{N:>6} {batch:>6} {t12:>12.2f} {t6:>12.2f} {t6 / t12:>7.3f}', flush=True)
