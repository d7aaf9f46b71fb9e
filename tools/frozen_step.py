#!/usr/bin/env python3
"""What frozen parameters save in the fused supervised step: EcgVit-base, bf16, B = 512 records of 5000 samples (N = 251 tokens), its configured dropout,
four setups timed in alternating runs on one device -- every parameter trainable, linear probe (the head alone), the top 2 blocks + head,
the top 6 blocks + head -- in records/s; then the optimiser pass alone: the span kernels over one whole-buffer span against the
whole-buffer kernels (sum of squares + clip/AdamW, us per pass).  Writes profiles/r11_frozen_step.txt.
usage: python tools/frozen_step.py [--runs 3] [--steps 10] [--warmup 3]"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ecg_representation_learning_amd as E  # noqa: E402
from ecg_representation_learning_amd import hip  # noqa: E402

B, LENGTH = 512, 5000


def setups(ly):
    head = lambda n: n.startswith('vit.mlp_head.')
    top = lambda k: (lambda n: head(n) or any(n.startswith(f'vit.transformer.layers.{i}.') for i in range(ly - k, ly)))
    return [('full step', lambda n: True), ('linear probe', head), ('top 2 blocks + head', top(2)), ('top 6 blocks + head', top(6))]


def time_steps(model, x, y, trainable, steps, warmup):
    """records/s of `steps` fused steps with `trainable`; a fresh optimiser each time (every parameter's own step count from 1, so that the
    full step runs the whole-buffer kernels)"""
    for n, p in model.named_parameters():
        p.requires_grad_(trainable(n))
    step = E.HipTrainStep(model, dict(n_step=10 ** 6), sync_nonfinite=False)
    for _ in range(warmup):
        step.step(x, y)
    step.finish()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(steps):
        step.step(x, y)
    t1.record()
    step.finish()
    torch.cuda.synchronize()
    return steps * B / (t0.elapsed_time(t1) / 1e3)


def time_optimiser(model, iters, reps):
    """us per (sumsq + clip/AdamW) pass over the whole flat buffer: whole-buffer kernels vs one whole-buffer span"""
    l, st = hip.lib(), hip.stream()
    p, g = model._pflat, model._gflat
    n = p.numel()
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    g.normal_().mul_(1e-3)
    wlow = model._wlow
    ws = torch.empty(max(l.ecgvit_sumsq_workspace(n), l.ecgvit_sumsq_spans_workspace(1)), dtype=torch.uint8, device=p.device)
    s = torch.empty(1, device=p.device)
    out = torch.empty(2, device=p.device)
    spans = torch.tensor([[0, n, 0]], dtype=torch.int64, device=p.device)
    pc, mc, vc = p.clone(), m.clone(), v.clone()   # restored afterwards: the model's weights are not the point here

    def whole():
        hip.check(l.ecgvit_sumsq(g.data_ptr(), n, s.data_ptr(), ws.data_ptr(), st), 'sumsq')
        hip.check(l.ecgvit_adamw_step(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), wlow.data_ptr(), n, s.data_ptr(), 1.0, 1.0, 1e-9,
                                      0.9, 0.999, 1e-8, 0.0, 1, 1, out.data_ptr(), st), 'adamw_step')

    def span():
        hip.check(l.ecgvit_sumsq_spans(g.data_ptr(), spans.data_ptr(), 1, n, s.data_ptr(), ws.data_ptr(), st), 'sumsq_spans')
        hip.check(l.ecgvit_adamw_step_spans(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), wlow.data_ptr(), spans.data_ptr(), 1, n,
                                            s.data_ptr(), 1.0, 1.0, 1e-9, 0.9, 0.999, 1e-8, 0.0, 1, 1, out.data_ptr(), st), 'adamw_step_spans')

    res = {'whole-buffer kernels': [], 'span kernels, one span': []}
    for _ in range(reps):
        for name, fn in (('whole-buffer kernels', whole), ('span kernels, one span', span)):
            fn()
            torch.cuda.synchronize()
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(iters):
                fn()
            t1.record()
            torch.cuda.synchronize()
            res[name].append(t0.elapsed_time(t1) * 1e3 / iters)
    p.copy_(pc), m.copy_(mc), v.copy_(vc)
    return res, n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=3)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r11_frozen_step.txt'))
    a = ap.parse_args()
    import bench
    conf, _ = bench.make_config(E, 'base', 20, LENGTH, None)   # the bench line's base workload: patch 20, 251 tokens, configured dropout
    torch.manual_seed(0)
    model = E.EcgVit(config=conf, compute_dtype=torch.bfloat16).cuda().train()
    x, y = E.workload.synthetic_batch(B, length=LENGTH, seed=77)
    x, y = x.cuda(), y.cuda()
    cases = setups(conf.num_hidden_layers)
    rates = {name: [] for name, _ in cases}
    for r in range(a.runs):
        for name, tr in (cases if r % 2 == 0 else cases[::-1]):
            rates[name].append(time_steps(model, x, y, tr, a.steps, a.warmup))
            print(f'run {r}: {name:22s} {rates[name][-1]:8.1f} records/s', flush=True)
    for p in model.parameters():
        p.requires_grad_(True)
    opt, n = time_optimiser(model, 20, a.runs)
    full = max(rates['full step'])
    lines = [f'(a) fused supervised step, EcgVit-base, bf16, B = {B}, N = 251, dropout {conf.hidden_dropout_prob}, {a.steps} steps per run after {a.warmup} warm-up steps, '
             f'{a.runs} alternating runs (records/s; speed-up of the best run over the best full step)']
    for name, _ in cases:
        rs = rates[name]
        lines.append(f'    {name:22s} ' + ' '.join(f'{v:8.1f}' for v in rs) + f'   best {max(rs):8.1f}   x {max(rs) / full:.2f}')
    lines.append(f'(b) optimiser pass alone (sum of squares + clip/AdamW with the bf16 shadow) over the whole flat buffer, {n} elements, '
                 f'20 passes per run (us per pass)')
    for name, ts in opt.items():
        lines.append(f'    {name:22s} ' + ' '.join(f'{v:8.1f}' for v in ts) + f'   best {min(ts):8.1f}')
    text = '\n'.join(lines) + '\n'
    print(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
