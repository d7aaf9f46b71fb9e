#!/usr/bin/env python3
"""Attention rollout for whole batches, one GPU process:
  (a) `ecgvit_rollout_colsum` (both launches) against `ecgvit_attention_fwd` at the same shape and in the same run, us per launch, at
      512 x 251 tokens, h = 12, dh = 64 and at 16 x 2048 tokens, h = 16, dh = 64 (2048 is the longest record the fused bf16 attention and the
      rollout kernels take).  The forward does the same Q K^T plus a P V product: a colsum slower than the forward is reported as such;
  (b) `EcgVit.attention_rollout_batch`, EcgVit-base, bf16, B = 64 records of 5000 samples (N = 251), against 64 calls of the one-record
      `attention_rollout` on the same records, ms per 64 records;
  (c) the peak device memory of one call of (b) above the resting allocation, next to one layer's (B, h, N, N) f32 tensor;
  (d) the errors tests/test_gpu_rollout.py measures on the bf16 engine (its own printed figures: the test is run from here).
Writes profiles/r17_rollout.txt (--out).
usage: python tools/rollout_rate.py [--runs 3] [--reps 20]"""
import argparse
import contextlib
import io
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ecg_representation_learning_amd as E  # noqa: E402
from ecg_representation_learning_amd import hip  # noqa: E402
from ecg_representation_learning_amd.hip import lib, check, ptr, stream  # noqa: E402

B, LENGTH = 64, 5000


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


def alternate(fns, runs, reps, warmup=3):
    """{name: [us per call, one per run]}: the candidates take turns inside every run, the order flips from run to run"""
    out = {n: [] for n, _ in fns}
    for r in range(runs):
        for n, fn in (fns if r % 2 == 0 else fns[::-1]):
            out[n].append(timed(fn, reps, warmup))
    return out


def kernel_rows(runs, reps):
    lines = []
    for (b, n, h, dh) in ((512, 251, 12, 64), (16, 2048, 16, 64)):
        d = h * dh
        scale = dh ** -0.5
        qkv = torch.randn(b * n, 3 * d, device='cuda').to(torch.bfloat16)
        out = torch.empty(b * n, d, device='cuda', dtype=torch.bfloat16)
        lse = torch.empty(b * h * n, device='cuda')
        w, r = torch.rand(b, n, device='cuda'), torch.empty(b, n, device='cuda')
        ws = torch.empty(lib().ecgvit_rollout_workspace(b, n, h), dtype=torch.uint8, device='cuda')

        def fwd():
            check(lib().ecgvit_attention_fwd(ptr(qkv), ptr(out), ptr(lse), b, n, h, dh, scale, 0.0, 0, hip.BF16, stream()), 'attention_fwd')

        def colsum():
            check(lib().ecgvit_rollout_colsum(ptr(qkv), ptr(lse), None, ptr(w), ptr(r), ptr(ws), None, None, b, n, h, dh, scale, hip.BF16, stream()),
                  'rollout_colsum')
        fwd()
        t = alternate((('colsum', colsum), ('fwd', fwd)), runs, reps)
        k, f = min(t['colsum']), min(t['fwd'])
        flops = 2.0 * b * h * n * n * dh   # Q K^T alone (the forward does twice that)
        lines.append(f'    B = {b:3d}, N = {n:4d}, h = {h:2d}, dh = {dh}: ecgvit_rollout_colsum ' + ' '.join(f'{v:7.1f}' for v in t['colsum'])
                     + f'  best {k:7.1f} us ({flops / (k * 1e-6) / 1e12:.1f} TFLOP/s of Q K^T);  ecgvit_attention_fwd ' + ' '.join(f'{v:7.1f}' for v in t['fwd'])
                     + f'  best {f:7.1f} us;  colsum / fwd {k / f:.3f}' + ('  -- SLOWER than the forward' if k > f else ''))
        del qkv, out, lse, w, r, ws
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=3)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r17_rollout.txt'))
    a = ap.parse_args()
    import bench
    lines = [f'sources: bench.kernel_source_hash() = {bench.kernel_source_hash()}; {torch.cuda.get_device_name(0)}',
             f'(a) weighted column sum of P (two launches: per (record, head, 128-key block), then over the heads) next to the fused forward at the same shape, bf16, '
             f'us per call, {a.runs} alternating runs of {a.reps} calls (16 x 2049 tokens is past the 2048-token limit of both kernels: measured at 2048)']
    lines += kernel_rows(a.runs, a.reps)

    conf, _ = bench.make_config(E, 'base', 20, LENGTH, None)
    torch.manual_seed(0)
    model = E.EcgVit(config=conf, compute_dtype=torch.bfloat16).cuda().eval()
    x, _ = E.workload.synthetic_batch(B, length=LENGTH, seed=77)
    x = x.cuda()

    def batch():
        return model.attention_rollout_batch(x)

    def one_by_one():
        return [model.attention_rollout(x[b]) for b in range(B)]
    got = batch()
    ref = torch.stack([m for _, m in one_by_one()])
    err = float((got.maps - ref).abs().max())
    t = alternate((('batch', batch), ('one', one_by_one)), a.runs, 3, warmup=1)
    kb, ko = min(t['batch']), min(t['one'])
    lines.append(f'(b) attention maps of {B} records, EcgVit-base, bf16, N = 251, ms per {B} records, {a.runs} alternating runs of 3 calls '
                 f'(max |batch - one by one| {err:.1e}: the two read different passes\' bf16 activations)')
    lines.append('    attention_rollout_batch (one pass, B = 64)     ' + ' '.join(f'{v / 1e3:8.2f}' for v in t['batch']) + f'   best {kb / 1e3:8.2f} ms = {kb / B:8.1f} us per record')
    lines.append('    attention_rollout, 64 calls (B = 1 each)       ' + ' '.join(f'{v / 1e3:8.2f}' for v in t['one']) + f'   best {ko / 1e3:8.2f} ms = {ko / B:8.1f} us per record')
    lines.append(f'    batch / one by one: x {ko / kb:.1f} faster per record')
    del got, ref
    batch()
    torch.cuda.synchronize()
    rest = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = batch()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - rest
    one_layer = B * conf.num_attention_heads * 251 * 251 * 4
    lines.append(f'(c) peak device memory of one attention_rollout_batch call of (b) above the resting allocation (activation slabs included at rest): '
                 f'{peak / 1e6:.2f} MB; one layer\'s (B, h, N, N) f32 tensor: {one_layer / 1e6:.1f} MB, x {conf.num_hidden_layers} layers = '
                 f'{one_layer * conf.num_hidden_layers / 1e9:.2f} GB')
    del out

    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    import test_gpu_rollout as T
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        for hidden in (128, 256):
            T.test_bf16_engine_in_every_batch_form(hidden)
    lines.append('(d) errors of the bf16 engine as tests/test_gpu_rollout.py::test_bf16_engine_in_every_batch_form measures them (hidden 128 / 256, 2 heads, 3 layers, '
                 'L = 1000, P = 4, B = 6; maps in [0, 1])')
    lines += ['    ' + ln for ln in buf.getvalue().splitlines() if ln.startswith('rollout')]
    text = '\n'.join(lines) + '\n'
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as fh:
        fh.write(text)


if __name__ == '__main__':
    main()
