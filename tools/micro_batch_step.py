#!/usr/bin/env python3
"""Gradient accumulation over micro-batches in the fused train step (HipTrainStep.step(..., micro_batch_size=)), one GPU process:
  (a) the engine's activation pool per configuration, from VitEngine._act_spec (host arithmetic, nothing allocated): EcgVit-large at 2048
      tokens (max_signal_length 20470, patch 10) at B = 256 / 128 / 64 / 32, EcgVit-base at 251 tokens at B = 512 / 128;
  (b) EcgVit-base, bf16, B = 512, 251 tokens, dropout 0.1: records/s at micro_batch_size None / 256 / 128 / 64, alternating runs, next to
      unsplit steps over the first 256 / 128 / 64 records (what one pass of that size runs at, optimiser included);
  (c) the accumulate kernel alone over the base flat buffer: us per mode and GB/s;
  (d) EcgVit-large at 2048 tokens, bf16, B = 256 at micro_batch_size 32: a few timed steps and the peak device memory.
Writes profiles/r12_micro_batch.txt (--out).
usage: python tools/micro_batch_step.py [--runs 3] [--steps 10] [--warmup 3] [--large-steps 3]"""
import argparse
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ecg_representation_learning_amd as E  # noqa: E402
from ecg_representation_learning_amd import hip  # noqa: E402
from ecg_representation_learning_amd.engine import ParamLayout, VitEngine  # noqa: E402

BASE_B, BASE_LEN = 512, 5000
LARGE_B, LARGE_LEN, LARGE_PATCH, LARGE_MB = 256, 20470, 10, 32


def pool_bytes(conf, B, dtype=torch.bfloat16):
    """bytes of every slab `_act_spec` names for a supervised pass over B records (the pool a plain step over B records allocates)"""
    eng = VitEngine(C=conf.num_channels, L=conf.max_signal_length, P=conf.patch_size, d=conf.hidden_size, h=conf.num_attention_heads,
                    f=conf.intermediate_size, Ly=conf.num_hidden_layers, K=71, p_hidden=conf.hidden_dropout_prob,
                    p_emb=conf.attention_probs_dropout_prob, dtype=dtype, layout=ParamLayout([]))
    eng.WT = {'bound': True}   # as after bind(): the bf16 engine holds transposed shadows (the e4m3 saved FFN tensor needs them)
    return sum(int(torch.Size(sh).numel()) * dt.itemsize for sh, dt in eng._act_spec(B, False, 0).values())


def time_steps(step, x, y, mb, steps, warmup):
    if isinstance(mb, str):   # 'B=n': an unsplit step over the first n records
        n = int(mb[2:])
        x, y, mb = x[:n], y[:n], None
    for _ in range(warmup):
        step.step(x, y, micro_batch_size=mb)
    step.finish()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(steps):
        step.step(x, y, micro_batch_size=mb)
    t1.record()
    step.finish()
    torch.cuda.synchronize()
    return steps * x.shape[0] / (t0.elapsed_time(t1) / 1e3)


def time_accumulate(model, iters, reps):
    """us per launch of each mode over one whole-buffer span of the model's flat gradient buffer"""
    l, st = hip.lib(), hip.stream()
    g = model._gflat
    n = g.numel()
    g.normal_()
    acc = torch.zeros_like(g)
    spans = torch.tensor([[0, n, 0]], dtype=torch.int64, device=g.device)
    modes = (('INIT  acc = g', hip.ACC_INIT, 8), ('ADD   acc += g', hip.ACC_ADD, 12), ('FOLD  g += acc', hip.ACC_FOLD, 12))
    res = {name: [] for name, _, _ in modes}
    for _ in range(reps):
        for name, mode, _ in modes:
            launch = lambda: hip.check(l.ecgvit_grad_accumulate(acc.data_ptr(), g.data_ptr(), spans.data_ptr(), 1, n, mode, 1.0, st),
                                       'grad_accumulate')
            if mode == hip.ACC_FOLD:
                acc.zero_()   # g += 0: the buffers stay finite however often it runs
            launch()
            torch.cuda.synchronize()
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(iters):
                launch()
            t1.record()
            torch.cuda.synchronize()
            res[name].append(t0.elapsed_time(t1) * 1e3 / iters)
    return [(name, bpe, res[name]) for name, _, bpe in modes], n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=3)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--large-steps', type=int, default=3)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r12_micro_batch.txt'))
    a = ap.parse_args()
    import bench
    lines = [f'sources: bench.kernel_source_hash() = {bench.kernel_source_hash()}; {torch.cuda.get_device_name(0)}']

    # (a) host arithmetic only
    large, _ = bench.make_config(E, 'large', LARGE_PATCH, LARGE_LEN, None)
    base, _ = bench.make_config(E, 'base', 20, BASE_LEN, None)
    d, f, ly = large.hidden_size, large.intermediate_size, large.num_hidden_layers
    N = LARGE_LEN // LARGE_PATCH + 1
    per_record = ly * N * (2 * (8 * d + f) + f)
    lines.append(f'(a) activation pool of a supervised bf16 pass (VitEngine._act_spec, every slab, layer and backward scratch included; nothing allocated)')
    lines.append(f'    EcgVit-large, {N} tokens (max_signal_length {LARGE_LEN}, patch {LARGE_PATCH}); per-layer slabs alone {ly} x {N} x (2(8d + f) + f) B '
                 f'= {per_record / 1e9:.3f} GB per record')
    for B in (256, 128, 64, 32):
        lines.append(f'        B = {B:4d}: {pool_bytes(large, B) / 1e9:8.1f} GB')
    lines.append(f'    EcgVit-base, {BASE_LEN // 20 + 1} tokens (max_signal_length {BASE_LEN}, patch 20)')
    for B in (512, 128):
        lines.append(f'        B = {B:4d}: {pool_bytes(base, B) / 1e9:8.1f} GB')
    print('\n'.join(lines), flush=True)

    # (b) base step at four micro-batch sizes, alternating order
    torch.manual_seed(0)
    model = E.EcgVit(config=base, compute_dtype=torch.bfloat16).cuda().train()
    x, y = E.workload.synthetic_batch(BASE_B, length=BASE_LEN, seed=77)
    x, y = x.cuda(), y.cuda()
    step = E.HipTrainStep(model, dict(n_step=10 ** 6), sync_nonfinite=False)
    cases = [None, 256, 128, 64, 'B=256', 'B=128', 'B=64']
    rates = {mb: [] for mb in cases}
    for r in range(a.runs):
        for mb in (cases if r % 2 == 0 else cases[::-1]):
            rates[mb].append(time_steps(step, x, y, mb, a.steps, a.warmup))
            print(f'run {r}: {str(mb):5s} {rates[mb][-1]:8.1f} records/s', flush=True)
    full = max(rates[None])
    lines.append(f'(b) fused supervised step, EcgVit-base, bf16, B = {BASE_B}, N = 251, dropout {base.hidden_dropout_prob}, {a.steps} steps per run after '
                 f'{a.warmup} warm-up steps, {a.runs} alternating runs (records/s; best run against the best unsplit B = {BASE_B} run).  '
                 f'micro_batch_size m: one optimiser step over B / m passes; B=n: a plain unsplit step over n records (one pass + its own optimiser pass)')
    for mb in cases:
        rs = rates[mb]
        name = f'B=512, micro_batch_size {mb}' if not isinstance(mb, str) else f'{mb}, unsplit'
        lines.append(f'    {name:30s} ' + ' '.join(f'{v:8.1f}' for v in rs) + f'   best {max(rs):8.1f}   x {max(rs) / full:.3f}'
                     f'   ({(BASE_B if not isinstance(mb, str) else int(mb[2:])) / max(rs) * 1e3:.2f} ms per optimiser step)')

    # (c) the accumulate kernel alone
    res, n = time_accumulate(model, 50, a.runs)
    lines.append(f'(c) ecgvit_grad_accumulate alone over the base flat buffer, one span of {n} elements, 50 launches per run (us per launch; '
                 f'GB/s at 8 B per element for INIT, 12 B for ADD / FOLD)')
    for name, bpe, ts in res:
        lines.append(f'    {name:16s} ' + ' '.join(f'{v:8.1f}' for v in ts) + f'   best {min(ts):8.1f} us   {bpe * n / min(ts) / 1e3:7.0f} GB/s')
    del step, model, x, y
    torch.cuda.empty_cache()
    print('\n'.join(lines[-6:]), flush=True)

    # (d) EcgVit-large at 2048 tokens, the reference's batch of 256 on one device
    torch.manual_seed(0)
    torch.cuda.reset_peak_memory_stats()
    model = E.EcgVit(config=large, compute_dtype=torch.bfloat16).cuda().train()
    x, y = E.workload.synthetic_batch(LARGE_B, length=LARGE_LEN, seed=77)
    x, y = x.cuda(), y.cuda()
    step = E.HipTrainStep(model, dict(n_step=10 ** 6), sync_nonfinite=True)
    t = time.time()
    loss, _ = step.step(x, y, micro_batch_size=LARGE_MB)
    torch.cuda.synchronize()
    first = time.time() - t
    ts, losses = [], [float(loss)]
    for _ in range(a.large_steps):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        loss, _ = step.step(x, y, micro_batch_size=LARGE_MB)
        t1.record()
        torch.cuda.synchronize()
        ts.append(t0.elapsed_time(t1))
        losses.append(float(loss))
    peak = torch.cuda.max_memory_allocated() / 1e9
    lines.append(f'(d) EcgVit-large, bf16, {N} tokens, dropout {large.hidden_dropout_prob}, B = {LARGE_B} on one device at micro_batch_size {LARGE_MB} '
                 f'({(LARGE_B + LARGE_MB - 1) // LARGE_MB} passes per optimiser step): first step {first:.1f} s (allocation included), then '
                 + ', '.join(f'{v:.0f}' for v in ts) + f' ms per step = {LARGE_B / (min(ts) / 1e3):.1f} records/s (best); loss '
                 + ' -> '.join(f'{v:.4f}' for v in losses) + f'; grad_norm {step.grad_norm():.4f}; peak device memory {peak:.1f} GB '
                 f'(pool for {LARGE_MB} records: {pool_bytes(large, LARGE_MB) / 1e9:.1f} GB)')
    text = '\n'.join(lines) + '\n'
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as fh:
        fh.write(text)


if __name__ == '__main__':
    main()
