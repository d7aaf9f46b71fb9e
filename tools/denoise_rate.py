#!/usr/bin/env python3
"""The denoiser's kernels (csrc/denoise.hip) at corpus shape, one GPU process: resident stores of 512 x 12 x 2500 and 512 x 12 x 5000 f32.
  low-pass         ms per launch, bytes/s (one read and one write of the store)
  noise estimate   ms per launch
  non-local means  ms per launch, weights/s -- `evaluated`: the (sample, shift) pairs whose neighbour lies in (0, n), M (n - 1), which is what
                   the kernel computes; `nominal`: the M (2n - 1) shifts the reference loops over -- and the share of the vector-issue bound:
                   a SIMD that holds two or more waves issues a wave64 vector instruction every 2 cycles (one wave alone: every 4) and a
                   transcendental (`v_exp_f32`) at twice that cost, so the bound is CUs x 4 SIMDs x 64 lanes x the board's peak clock over
                   2 (plain instructions per weight) + 4 (v_exp_f32 per weight) cycles, with the counts of the fast body as
                   tools/code_objects.py reads them from the built library (158 VGPRs: three waves per SIMD)
  baseline         the numpy restatement (tests/denoise_ref.py, f64) on a sample of the runs of one lead, scaled to the store
Warm-up, device events, `--reps` launches each.  Writes profiles/r20_denoise.txt (--out).
usage: python tools/denoise_rate.py [--reps 3] [--records 512]"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import ecg_representation_learning_amd as E  # noqa: E402

C, P = 12, 10
PEAK_CLOCK = 2.4e9      # Hz


def timed(fn, reps, warmup=1):
    """ms per call"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--records', type=int, default=512)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r20_denoise.txt'))
    a = ap.parse_args()
    import bench
    import code_objects
    import denoise_ref as R
    blocks = code_objects.hot_blocks(E.hip.LIB_PATH, 'nlm_kernelILi4096')
    n_exp = max(1, sum(m for _, m in blocks))
    per_weight = sum(v for v, _ in blocks) / n_exp
    cycles = 2.0 * (per_weight - 1.0) + 4.0                 # per weight and wave64 instruction stream: one v_exp_f32 at twice the plain cost
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    issue = cus * 4 * 64 * PEAK_CLOCK * per_weight / cycles  # so that issue / per_weight is the bound in weights/s
    lines = [f'sources: bench.kernel_source_hash() = {bench.kernel_source_hash()}; {torch.cuda.get_device_name(0)}, {cus} CUs',
             f'non-local means fast body: {per_weight:.2f} vector instructions per weight ({blocks}: (vector, v_exp_f32) per block); '
             f'= {cycles:.1f} issue cycles per weight with two or more waves per SIMD (plain 2, v_exp_f32 4); vector-issue bound {issue / per_weight / 1e12:.2f} T weights/s at {PEAK_CLOCK / 1e9:.1f} GHz',
             f'{a.reps} launches after one warm-up, device events']
    n = a.records
    for L, sw in ((2500, None), (5000, None), (5000, 40)):
        g = torch.Generator(device='cuda').manual_seed(20)
        t = torch.arange(L, device='cuda', dtype=torch.float32)
        x = (torch.sin(t / 13.0)[None, None, :] * torch.rand((n, C, 1), device='cuda', generator=g) + 0.05 * torch.randn((n, C, L), device='cuda', generator=g)).contiguous()
        out = torch.empty_like(x)
        t_lp = timed(lambda: E.lowpass(x, out=out), a.reps)
        t_sg = timed(lambda: E.estimate_noise_std(x), a.reps)
        sg = E.estimate_noise_std(x)
        t_nlm = timed(lambda: E.nlm(x, sigma=sg, search_width=sw, out=out), a.reps)
        M = L - 2 * P - 1
        if sw is not None:
            lines.append(f'    non-local means, search_width = {sw}  {t_nlm:10.2f} ms  (same store; 2 x {sw} - 1 shifts per sample)')
            print(lines[-1], flush=True)
            continue
        ev, nom = float(n) * C * M * (L - 1), float(n) * C * M * (2 * L - 1)
        lines.append(f'store {n} x {C} x {L} f32 = {x.numel() * 4 / 1e6:.0f} MB')
        lines.append(f'    low-pass (f64, zero-phase)   {t_lp:10.2f} ms  {2 * x.numel() * 4 / (t_lp * 1e-3) / 1e9:8.1f} GB/s')
        lines.append(f'    noise estimate               {t_sg:10.2f} ms  {n * C / (t_sg * 1e-3) / 1e3:8.1f} k leads/s')
        lines.append(f'    non-local means              {t_nlm:10.2f} ms  {ev / (t_nlm * 1e-3) / 1e12:8.3f} T weights/s evaluated = {ev / (t_nlm * 1e-3) / (issue / per_weight):.2f} of the '
                     f'vector-issue bound  ({nom / (t_nlm * 1e-3) / 1e12:.3f} T/s nominal)')
        # the numpy restatement on a sample of the runs of one lead, scaled
        lead = x[0, 0].cpu().numpy().astype(np.float64)
        K = R.n_runs(L, P)
        runs = list(range(0, K, max(1, K // 8)))
        t0 = time.perf_counter()
        R.nlm(lead, float(sg[0, 0]), runs=runs)
        t_np = (time.perf_counter() - t0) * K / len(runs) * n * C
        lines.append(f'    numpy restatement (f64), {len(runs)} of {K} runs of one lead scaled to the store: {t_np:10.1f} s = x {t_np * 1e3 / t_nlm:.0f} the kernel')
        print('\n'.join(lines[-5:]), flush=True)
        del x, out
    text = '\n'.join(lines) + '\n'
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as fh:
        fh.write(text)


if __name__ == '__main__':
    main()
