#!/usr/bin/env python3
"""the fused attention forward and backward at the long-record shapes and at the 501-token comparison shape, in ONE process on one device
(profiling target: rocprofv3 --kernel-trace --stats -- python3 tools/attn_long.py [reps] [p]).  256 x 16 x 501 and 64 x 16 x 1001 hold the same
number of score elements (within 0.3 %): the ratio of their times is the cost of the long-record forms per score."""
import os, sys, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ecg_representation_learning_amd import hip
from ecg_representation_learning_amd.hip import lib, check, ptr, stream
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
p = float(sys.argv[2]) if len(sys.argv) > 2 else 0.1
SHAPES = [(256, 16, 501), (64, 16, 1001), (64, 16, 1251), (32, 16, 2048), (256, 16, 501), (64, 16, 1001)]   # (B, h, N); the first two again: drift
res = {}
for B, h, N in SHAPES:
    d = h * 64
    torch.manual_seed(3)
    qkv = torch.randn(B * N, 3 * d, device='cuda').to(torch.bfloat16)
    out = torch.empty(B * N, d, device='cuda', dtype=torch.bfloat16)
    do = torch.randn(B * N, d, device='cuda').to(torch.bfloat16)
    lse = torch.empty(B * h * N, device='cuda')
    dqkv = torch.empty(B * N, 3 * d, device='cuda', dtype=torch.bfloat16)
    e = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    fwd = lambda: check(lib().ecgvit_attention_fwd(ptr(qkv), ptr(out), ptr(lse), B, N, h, 64, 0.125, p, 7, hip.BF16, stream()), 'fwd')
    bwd = lambda: check(lib().ecgvit_attention_bwd(ptr(qkv), ptr(out), ptr(do), ptr(lse), ptr(dqkv), B, N, h, 64, 0.125, p, 7, hip.BF16, stream()), 'bwd')
    for _ in range(2):
        fwd(); bwd()
    e[0].record()
    for _ in range(reps):
        fwd()
    e[1].record()
    for _ in range(reps):
        bwd()
    e[2].record()
    torch.cuda.synchronize()
    tf, tb = 1e3 * e[0].elapsed_time(e[1]) / reps, 1e3 * e[1].elapsed_time(e[2]) / reps
    res.setdefault((B, h, N), []).append((tf, tb))
    print(f'attention {B} x {h} x {N}, p = {p}: {B * h * N * N / 1e9:.3f} G scores, forward {tf:.1f} us, backward {tb:.1f} us per launch '
          f'({1e6 * tf / (B * h * N * N):.3f} / {1e6 * tb / (B * h * N * N):.3f} ns per 1000 scores)', flush=True)
    del qkv, out, do, lse, dqkv
    torch.cuda.empty_cache()
a, b = res[(256, 16, 501)], res[(64, 16, 1001)]
fa, ba = min(x[0] for x in a), min(x[1] for x in a)
fb, bb = min(x[0] for x in b), min(x[1] for x in b)
print(f'64 x 16 x 1001 against 256 x 16 x 501 (best of two, same score count within 0.3 %): forward {fb / fa:.3f} x, backward {bb / ba:.3f} x')
