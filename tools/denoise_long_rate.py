#!/usr/bin/env python3
"""The Holter-length forms of the denoiser (csrc/denoise.hip: ecgvit_filtfilt_long, ecgvit_nlm_sigma_long, ecgvit_nlm_denoise_tiled,
ecgvit_rloess_tiled; `tiled=True` in denoise.py) beside the resident kernels, one GPU process.  No ratio is fixed in advance: the resident
kernel in the same run is the yardstick.
  512 x 12 x 5000     tiled against resident, all four stages: what the tiling costs where it is not needed
  1 x 12 x 32768      tiled against resident: the few-records case (the resident kernels put 12 workgroups on the board); the low-pass here
                      is 12 concurrent chains of lane 0, so its time over 2 (n + 54) steps is the serial walk's cost per sample and pass
  75 x 12 x 462600    the INCART shape (30 minutes at 257 Hz), tiled only -- no resident kernel takes it: low-pass, noise estimate and robust
                      LOESS at 500 points on the whole store; non-local means with search_width=2500 on the whole store, and with the full
                      search on ONE record, scaled by 75 to the corpus
The stores are beats (Gaussian bumps every 36 .. 46 samples) + a sway + Gaussian noise 0.05, the third store of tools/loess_rate.py.  Every
stage runs out of place (`out=` a second store): the in-place scratch of the tiled stages is not priced here.
Warm-up, device events.  Writes profiles/r22_denoise_long.txt (--out).
usage: python tools/denoise_long_rate.py [--reps 2] [--incart-records 75]"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import ecg_representation_learning_amd as E  # noqa: E402

C, P = 12, 10
INCART = 462600


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


def store(n, L, seed):
    g = torch.Generator(device='cuda').manual_seed(seed)
    u = lambda lo, hi: lo + (hi - lo) * torch.rand((n, C, 1), device='cuda', generator=g)    # noqa: E731
    x = torch.empty((n, C, L), device='cuda')
    t = torch.arange(L, device='cuda', dtype=torch.float32)
    for lo in range(0, n, 16):                                   # 16 records at a time: the intermediates of the long store stay small
        s = slice(lo, min(n, lo + 16))
        period = u(36, 46)[s]
        phase = torch.remainder(t[None, None, :] - u(0, 41)[s], period)
        beats = torch.exp(-0.5 * (torch.minimum(phase, period - phase) / 2.5) ** 2)
        x[s] = u(0.5, 1.5)[s] * beats + 0.2 * torch.sin(2 * np.pi * t[None, None, :] / u(150, 400)[s] + u(0, 6)[s])
        x[s] += 0.05 * torch.randn(x[s].shape, device='cuda', generator=g)
    return x


def weights(n, L, W=None):
    """(sample, shift) pairs the non-local means evaluates: neighbours in (0, n) within the search width"""
    M = L - 2 * P - 1
    return float(n) * C * M * ((L - 1) if W is None else min(L - 1, 2 * W - 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=2)
    ap.add_argument('--incart-records', type=int, default=75)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r22_denoise_long.txt'))
    a = ap.parse_args()
    import bench
    import code_objects
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    lines = [f'sources: bench.kernel_source_hash() = {bench.kernel_source_hash()}; {torch.cuda.get_device_name(0)}, {cus} CUs',
             f'{a.reps} launches after one warm-up, device events (the INCART shape: one launch, no warm-up of its own); every stage out of place; '
             f'stores: beats + sway + Gaussian noise 0.05']
    for name, k in sorted(code_objects.kernels(E.hip.LIB_PATH).items()):
        if 'nlm_tiled_kernel' in name or 'rloess_tiled_kernel' in name or 'filtfilt_kernel' in name or 'nlm_sigma_kernel' in name:
            lines.append(f'    {name}: {k["vgpr_count"]} VGPRs, VGPR spills {k["vgpr_spill_count"]}, SGPR spills {k["sgpr_spill_count"]}, scratch {k["private_segment_fixed_size"]} B, '
                         f'LDS {k["group_segment_fixed_size"]} B')

    def note(s):
        lines.append(s)
        print(s, flush=True)

    def pair(what, fn, extra=lambda ms: ''):
        r, t = timed(lambda: fn(False), a.reps), timed(lambda: fn(True), a.reps)
        note(f'    {what:44s} resident {r:10.2f} ms   tiled {t:10.2f} ms   tiled / resident {t / r:5.2f}{extra(t)}')
        return r, t

    for n, L in ((512, 5000), (1, 32768)):
        x = store(n, L, 22)
        out = torch.empty_like(x)
        note(f'store {n} x {C} x {L} f32 = {x.numel() * 4 / 1e6:.0f} MB')
        _, t_lp = pair('low-pass (f64, zero-phase; the same kernel)', lambda tl: E.lowpass(x, out=out, tiled=tl))
        if n == 1:
            note(f'        the serial walk: {t_lp * 1e6 / (2 * (L + 54)):.1f} ns per sample and pass of one lane ({C} chains side by side; 2 passes over n + 54 samples)')
        pair('noise estimate (the same kernel)', lambda tl: E.estimate_noise_std(x, tiled=tl))
        sg = E.estimate_noise_std(x)
        pair('non-local means, full search', lambda tl: E.nlm(x, sigma=sg, out=out, tiled=tl),
             lambda ms: f'   {weights(n, L) / (ms * 1e-3) / 1e12:.3f} T weights/s tiled')
        pair('non-local means, search_width=2500', lambda tl: E.nlm(x, sigma=sg, search_width=2500, out=out, tiled=tl),
             lambda ms: f'   {weights(n, L, 2500) / (ms * 1e-3) / 1e12:.3f} T weights/s tiled')
        pair('robust LOESS npoints 500 robust_iters 10', lambda tl: E.rloess(x, 500, subtract=True, out=out, tiled=tl),
             lambda ms: f'   {ms * 1e6 / (n * C * L):.2f} ns per sample tiled')
        if n == 1:
            for tile in (512, 1024):
                ms = timed(lambda: E.rloess(x, 500, subtract=True, out=out, tiled=True, tile=tile), a.reps)
                note(f'    robust LOESS, tile={tile:5d}: tiled {ms:10.2f} ms')
            for tile in (960, 1920, 3840):
                ms = timed(lambda: E.nlm(x, sigma=sg, out=out, tiled=True, tile=tile), a.reps)
                note(f'    non-local means, full search, tile={tile:5d}: tiled {ms:10.2f} ms')
        del x, out

    n, L = a.incart_records, INCART
    x = store(n, L, 23)
    out = torch.empty_like(x)
    note(f'store {n} x {C} x {L} f32 = {x.numel() * 4 / 1e9:.2f} GB (the INCART shape), tiled=True')
    one = lambda fn: timed(fn, 1, warmup=0)    # noqa: E731
    per = max(1, E.denoise._WS_BYTES // E.hip.lib().ecgvit_denoise_workspace_long(1, C, L))
    ms = one(lambda: E.lowpass(x, out=out, tiled=True))
    note(f'    low-pass                                   {ms:10.1f} ms   ({per} records a launch: the f64 workspace stays within {E.denoise._WS_BYTES >> 20} MiB; '
         f'{ms * 1e6 / (-(-n // per) * 2 * (L + 54)):.1f} ns per sample and pass of a launch)')
    ms = one(lambda: E.estimate_noise_std(x, tiled=True))
    note(f'    noise estimate                             {ms:10.1f} ms')
    sg = E.estimate_noise_std(x, tiled=True)
    ms = one(lambda: E.rloess(x, 500, subtract=True, out=out, tiled=True))
    note(f'    robust LOESS npoints 500 robust_iters 10   {ms:10.1f} ms   {ms * 1e6 / (n * C * L):.2f} ns per sample')
    ms = one(lambda: E.nlm(x, sigma=sg, search_width=2500, out=out, tiled=True))
    note(f'    non-local means, search_width=2500         {ms:10.1f} ms   {weights(n, L, 2500) / (ms * 1e-3) / 1e12:.3f} T weights/s')
    x1, o1, s1 = x[:1].contiguous(), out[:1], sg[:1].contiguous()
    ms = one(lambda: E.nlm(x1, sigma=s1, out=o1, tiled=True))
    note(f'    non-local means, full search, ONE record   {ms:10.1f} ms   {weights(1, L) / (ms * 1e-3) / 1e12:.3f} T weights/s; x {n} records = {ms * n / 1e3:.1f} s for the corpus')
    assert torch.isfinite(out).all()
    text = '\n'.join(lines) + '\n'
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as fh:
        fh.write(text)


if __name__ == '__main__':
    main()
