#!/usr/bin/env python3
"""variable-length records, measured on one device; writes profiles/r10_attn_varlen.txt (usage: python3 tools/attn_varlen.py [reps] [steps]).
(a) the attnv_* kernels with every n_tok = N against the tuned uniform kernels (dh 64 and 128; 512 x 251, 256 x 501, 64 x 1251 at d = 768);
(b) the supervised step of EcgVit-base at patch 4 (N = 1251, bf16) on records whose lengths are uniform in [N/4, N] tokens, with `lengths`
against the same records zero-padded without it, in records/s.  Padded rows still go through the GEMMs and LayerNorms."""
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ecg_representation_learning_amd as E
from ecg_representation_learning_amd import hip
from ecg_representation_learning_amd.hip import lib, check, ptr, stream

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 10
lines = []


def out(s):
    print(s, flush=True)
    lines.append(s)


def timed(fn, n):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return 1e3 * e0.elapsed_time(e1) / n   # us per call


out('(a) fused attention, every n_tok = N: varlen kernels against the uniform kernels (us per launch, d = 768, dropout 0.1)')
out(f'{"dh":>4} {"B x N":>10} {"fwd uni":>9} {"fwd var":>9} {"ratio":>6} {"bwd uni":>9} {"bwd var":>9} {"ratio":>6}')
for dh in (64, 128):
    h = 768 // dh
    for B, N in ((512, 251), (256, 501), (64, 1251)):
        d = h * dh
        torch.manual_seed(3)
        qkv = torch.randn(B * N, 3 * d, device='cuda').to(torch.bfloat16)
        o = torch.empty(B * N, d, device='cuda', dtype=torch.bfloat16)
        do = torch.randn(B * N, d, device='cuda').to(torch.bfloat16)
        lse = torch.empty(B * h * N, device='cuda')
        dqkv = torch.empty(B * N, 3 * d, device='cuda', dtype=torch.bfloat16)
        nt = torch.full((B,), N, dtype=torch.int32, device='cuda')
        sc, p = dh ** -0.5, 0.1
        fu = lambda: check(lib().ecgvit_attention_fwd(ptr(qkv), ptr(o), ptr(lse), B, N, h, dh, sc, p, 7, hip.BF16, stream()), 'fwd')
        bu = lambda: check(lib().ecgvit_attention_bwd(ptr(qkv), ptr(o), ptr(do), ptr(lse), ptr(dqkv), B, N, h, dh, sc, p, 7, hip.BF16, stream()), 'bwd')
        fv = lambda: check(lib().ecgvit_attention_varlen_fwd(ptr(qkv), ptr(o), ptr(lse), ptr(nt), B, N, h, dh, sc, p, 7, stream()), 'vfwd')
        bv = lambda: check(lib().ecgvit_attention_varlen_bwd(ptr(qkv), ptr(o), ptr(do), ptr(lse), ptr(dqkv), ptr(nt), B, N, h, dh, sc, p, 7, stream()), 'vbwd')
        t = [timed(f, reps) for f in (fu, fv, bu, bv)]
        out(f'{dh:4d} {f"{B}x{N}":>10} {t[0]:9.1f} {t[1]:9.1f} {t[1] / t[0]:6.2f} {t[2]:9.1f} {t[3]:9.1f} {t[3] / t[2]:6.2f}')
        del qkv, o, do, lse, dqkv
        torch.cuda.empty_cache()

out('')
B = 32
conf = E.EcgVitConfig.from_defined('ecg-vit-base')
conf.max_signal_length, conf.patch_size = 5000, 4
N = conf.max_signal_length // conf.patch_size + 1
torch.manual_seed(0)
m = E.EcgVit(config=conf, compute_dtype=torch.bfloat16).cuda().train()
g = torch.Generator().manual_seed(1)
tok = torch.randint((N - 1) // 4, N, (B,), generator=g)          # valid patches per record, uniform in [n/4, n]
lengths = tok * conf.patch_size
x = torch.randn(B, 12, conf.max_signal_length, generator=g)
for b in range(B):
    x[b, :, int(lengths[b]):] = 0.0                                  # zero-padded to the batch width
x, y = x.cuda(), (torch.rand(B, 71, generator=g) < 0.05).float().cuda()
ts = E.HipTrainStep(m, dict(n_step=10 ** 6), sync_nonfinite=False)
res = {}
for tag, ln in (('padded', None), ('lengths', lengths), ('padded', None), ('lengths', lengths)):
    for _ in range(2):
        ts.step(x, y, lengths=ln)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        ts.step(x, y, lengths=ln)
    torch.cuda.synchronize()
    res.setdefault(tag, []).append(B * steps / (time.perf_counter() - t0))
ts.finish()
out(f'(b) supervised step, EcgVit-base, patch 4 (N = {N}), bf16, B = {B}, mean valid tokens {float(tok.float().mean() + 1):.0f} of {N}, '
    f'{steps} steps per run, two alternating runs each')
for tag, v in res.items():
    out(f'    {tag:8s} {" ".join(f"{r:8.1f}" for r in v)} records/s (best {max(v):.1f})')
out(f'    lengths / padded: {max(res["lengths"]) / max(res["padded"]):.3f} x')
path = os.path.join(ROOT, 'profiles', 'r10_attn_varlen.txt')
with open(path, 'w') as f:
    f.write('\n'.join(lines) + '\n')
print('wrote', path)
