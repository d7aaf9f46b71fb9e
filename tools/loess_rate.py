#!/usr/bin/env python3
"""The robust LOESS baseline (csrc/denoise.hip, rloess_kernel) at corpus shape beside the three other kernels of the denoiser, one GPU process:
resident stores of 512 x 12 x 2500 and 512 x 12 x 5000 f32.
  low-pass, noise estimate, non-local means    ms per launch (tools/denoise_rate.py prices them)
  robust LOESS    ms per launch at npoints 250 and 500, robust_iters 10 and 0; the mean robust iterations per sample (from `return_iters`);
                  ns per fit (a sample runs 1 + iterations fits) on the whole board; records/s
  instructions    per (sample, robust iteration) of one wave, counted in the disassembly of the built library: the loop nest of the kernel is
                  read from its backward branches (sample loop > robust loop > the median's bit loop, the one with the scalar population
                  counts); `outside`: the robust loop without the bit loop (residuals, the median's two wave reductions, the fit with its eight
                  moment sums and their butterflies, the elimination; the static count holds the branches of both degrees: degree 1 adds one
                  division, about 30 instructions, that degree 2 does not run); `per pass`: the bit loop's body, run once per bit until one candidate is
                  left -- the mean number of passes is counted in numpy on the first fit's residuals of one lead of the store.
  stores          four signals per shape: how many robust iterations a sample runs (2 to the cap of 10) is the signal's doing, and the
                  table gives the mean and the share of samples at the cap beside each time.
                  Vector instructions, the f64 ones among them, cross-lane (ds_bpermute / DPP) and scalar ones are listed apart: nobody has
                  measured this board's f64 vector issue rate on such a loop, so the table gives the counts and the measured time and
                  leaves the ratio to the reader.
Warm-up, device events, `--reps` launches each.  Writes profiles/r21_loess.txt (--out).
usage: python tools/loess_rate.py [--reps 2] [--records 512]"""
import argparse
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import ecg_representation_learning_amd as E  # noqa: E402

C = 12


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


def kind(ins):
    """-> (vector, f64 vector, cross-lane, scalar) of one disassembled instruction"""
    op = ins.split()[0]
    cross = op.startswith('ds_bpermute') or op.startswith('ds_swizzle') or 'dpp' in ins or op.startswith('v_readlane') or op.startswith('v_permlane')
    return np.array([op.startswith('v_'), op.startswith('v_') and '_f64' in op, cross, op.startswith('s_') and not op.startswith('s_waitcnt') and not op.startswith('s_nop')], int)


def loop_counts(lib, kernel):
    """the loop nest of `kernel` from its backward branches -> {'outside': counts of the robust loop without the bit loop, 'pass': counts of the
    bit loop}, counts = (vector, f64 vector, cross-lane, scalar) instructions"""
    import code_objects
    for img in code_objects.code_objects(lib):
        with tempfile.NamedTemporaryFile(suffix='.co', delete=False) as f:
            f.write(img)
            name = f.name
        try:
            txt = subprocess.run([code_objects.OBJDUMP, '-d', name], capture_output=True, text=True, check=True).stdout
        finally:
            os.unlink(name)
        lines = txt.splitlines()
        head = [k for k, l in enumerate(lines) if re.match(r'^[0-9a-f]+ <\S*' + re.escape(kernel) + r'\S*>:', l)]
        if not head:
            continue
        start = int(lines[head[0]].split()[0], 16)
        body = []
        for l in lines[head[0] + 1:]:
            if re.match(r'^[0-9a-f]+ <', l):
                break
            m = re.match(r'^\s+(.*?)\s+// ([0-9A-F]+):', l)
            if m:
                t = re.search(r'<\S+\+0x([0-9a-f]+)>\s*$', l)
                body.append((int(m.group(2), 16) - start, m.group(1), int(t.group(1), 16) if t and 'branch' in m.group(1) else None))
        heads = {}
        for off, _, tgt in body:               # a loop per header: from the target of its backward branches to the last of them
            if tgt is not None and tgt <= off:
                heads[tgt] = max(heads.get(tgt, 0), off)
        loops = sorted(heads.items(), key=lambda lo: lo[0] - lo[1])          # widest first
        has = lambda lo, word: any(lo[0] <= off <= lo[1] and ins.startswith(word) for off, ins, _ in body)   # noqa: E731
        nest = [lo for lo in loops if has(lo, 's_bcnt1')]                    # sample loop, robust loop, (the compiler's inner ones,) bit loop
        # the counts below are attributed by position: refuse a nest the compiler has shaped otherwise (an unrolled or split loop)
        if len(nest) < 3 or not all(nest[k][0] <= nest[k + 1][0] and nest[k + 1][1] <= nest[k][1] for k in range(len(nest) - 1)):
            raise RuntimeError(f'{kernel}: the loops that hold the population counts are not one nest of sample > robust > bit loop: {nest}')
        robust, bit = nest[1], nest[-1]
        if not (has(robust, 'v_div_scale_f64') and not has(bit, 'v_div_scale_f64') and not has(bit, 'ds_bpermute')):
            raise RuntimeError(f'{kernel}: the robust loop must hold the fit (its divisions) and the bit loop neither a division nor a butterfly')
        count = lambda lo, skip=None: sum((kind(ins) for off, ins, _ in body if lo[0] <= off <= lo[1] and not (skip and skip[0] <= off <= skip[1])), np.zeros(4, int))   # noqa: E731
        return {'outside': count(robust, bit), 'pass': count(bit)}
    raise RuntimeError(f'{kernel} not found in {lib}')


def mean_passes(lead, npoints):
    """the mean number of bit-loop passes of the median over the first fit's residuals of every window of one lead (numpy): a pass per bit from
    bit 62 until the median's candidates are one"""
    y = lead.astype(np.float64)
    n = len(y)
    m = min(npoints, n)
    j = np.arange(n)
    lo = np.clip(j - (m - 1) // 2 if m & 1 else j - m // 2, 0, n - m)
    d = np.maximum(j - lo, lo + m - 1 - j)
    idx = lo[:, None] + np.arange(m)[None, :]
    s = (idx - j[:, None]) / d[:, None]
    w = (1.0 - np.abs(s) ** 3) ** 3
    basis = np.stack([np.ones_like(s), s, s * s], axis=2)                    # the distance-weighted quadratic through the normal equations
    co = np.linalg.solve(np.einsum('nm,nmi,nmk->nik', w, basis, basis), np.einsum('nm,nmi,nm->ni', w, basis, y[idx])[:, :, None])[:, :, 0]
    aerr = np.ascontiguousarray(np.abs(np.einsum('nmi,ni->nm', basis, co) - y[idx]))
    keys = np.sort(aerr.view(np.uint64), axis=1)
    k = (m - 1) // 2
    x = np.concatenate([keys[:, :k], keys[:, k + 1:]], axis=1) ^ keys[:, k:k + 1]
    bits = np.where(x.min(axis=1) == 0, 0, np.frexp(x.min(axis=1).astype(np.float64))[1])      # bit length of the closest other key's difference
    return float(np.minimum(64 - bits, 63).mean())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=2)
    ap.add_argument('--records', type=int, default=512)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r21_loess.txt'))
    a = ap.parse_args()
    import bench
    import code_objects
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    lines = [f'sources: bench.kernel_source_hash() = {bench.kernel_source_hash()}; {torch.cuda.get_device_name(0)}, {cus} CUs',
             f'{a.reps} launches after one warm-up, device events; robust LOESS: degree 2, f64, one wave per sample, one workgroup of 8 waves per (record, lead)']
    res = code_objects.kernels(E.hip.LIB_PATH)
    static = {}
    for npts, nv in ((250, 4), (500, 8)):
        kname = f'rloess_kernelILi{nv}ELi8192E'
        k = next(v for name, v in res.items() if kname in name)
        static[npts] = loop_counts(E.hip.LIB_PATH, kname)
        o, p = static[npts]['outside'], static[npts]['pass']
        lines.append(f'rloess_kernel<{nv} slots per lane> (npoints {npts}): {k["vgpr_count"]} VGPRs, scratch {k["private_segment_fixed_size"]} B, LDS {k["group_segment_fixed_size"]} B; '
                     f'per (sample, robust iteration) and wave, outside the bit loop: {o[0]} vector ({o[1]} f64, {o[2]} cross-lane), {o[3]} scalar; '
                     f'per bit-loop pass: {p[0]} vector ({p[1]} f64 / 64-bit compares), {p[3]} scalar')
    n = a.records
    for L in (2500, 5000):
        g = torch.Generator(device='cuda').manual_seed(21)
        t = torch.arange(L, device='cuda', dtype=torch.float32)
        noise = torch.randn((n, C, L), device='cuda', generator=g)
        u = lambda lo, hi: lo + (hi - lo) * torch.rand((n, C, 1), device='cuda', generator=g)    # noqa: E731
        x = (torch.sin(t / 13.0)[None, None, :] * u(0, 1) + 0.05 * noise).contiguous()
        out = torch.empty_like(x)
        t_lp = timed(lambda: E.lowpass(x, out=out), a.reps)
        t_sg = timed(lambda: E.estimate_noise_std(x), a.reps)
        sg = E.estimate_noise_std(x)
        t_nlm = timed(lambda: E.nlm(x, sigma=sg, out=out), a.reps)
        lines.append(f'store {n} x {C} x {L} f32 = {x.numel() * 4 / 1e6:.0f} MB; the three other kernels on the first store below')
        lines.append(f'    low-pass (f64, zero-phase)   {t_lp:10.2f} ms')
        lines.append(f'    noise estimate               {t_sg:10.2f} ms')
        lines.append(f'    non-local means              {t_nlm:10.2f} ms')
        print('\n'.join(lines[-4:]), flush=True)
        # how long the robust loop runs is the signal's doing: four stores, from one where it stops at once to ones where samples reach the cap
        hit = torch.rand(x.shape, device='cuda', generator=g) < 0.04
        spike = hit * (1.0 + 2.0 * torch.rand(x.shape, device='cuda', generator=g)) * torch.sign(torch.randn(x.shape, device='cuda', generator=g))
        period = u(36, 46)
        phase = torch.remainder(t[None, None, :] - u(0, 41), period)
        beats = torch.exp(-0.5 * (torch.minimum(phase, period - phase) / 2.5) ** 2)
        stores = (('a sine of period 82 and random amplitude + Gaussian noise 0.05 (the store of tools/denoise_rate.py)', lambda: x),
                  ('the same with a spike of 1 .. 3 on 4 % of the samples', lambda: x + spike),
                  ('beats (Gaussian bumps of width 2.5 every 36 .. 46 samples, amplitude 0.5 .. 1.5) + a sway of period 150 .. 400 + Gaussian noise 0.05',
                   lambda: u(0.5, 1.5) * beats + 0.2 * torch.sin(2 * np.pi * t[None, None, :] / u(150, 400) + u(0, 6)) + 0.05 * noise),
                  ('a sine of period 628 and amplitude 0.7 + Gaussian noise 0.01', lambda: 0.7 * torch.sin(t / 100.0)[None, None, :] + 0.01 * noise))
        for what, make in stores:
            y = make().contiguous()
            lines.append(f'  {what}')
            lead = y[0, 0].cpu().numpy()
            for npts in (250, 500):
                it4 = E.rloess(y[:4].contiguous(), npts, return_iters=True)[1].float()
                its, capped = it4.mean().item(), (it4 == 10).float().mean().item()
                passes = mean_passes(lead, npts)
                o, p = static[npts]['outside'], static[npts]['pass']
                for ri in (10, 0):
                    ms = timed(lambda: E.rloess(y, npts, robust_iters=ri, subtract=True, out=out), a.reps)
                    fits = float(n) * C * L * (1 + (its if ri else 0.0))
                    extra = (f'; {its:.2f} robust iterations per sample, {100 * capped:.1f} % at the cap (first 4 records), {passes:.1f} bit-loop passes per median '
                             f'(first fit, one lead): {o[0] + passes * p[0]:.0f} vector + {o[3] + passes * p[3]:.0f} scalar instructions per (sample, iteration) and wave') if ri else ''
                    lines.append(f'    robust LOESS npoints {npts} robust_iters {ri:2d}  {ms:10.2f} ms  {ms * 1e6 / fits:8.3f} ns per fit  {n / (ms * 1e-3):9.0f} records/s{extra}')
                    print(lines[-1], flush=True)
            del y
        del x, out, noise, spike, beats, phase, hit
    text = '\n'.join(lines) + '\n'
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as fh:
        fh.write(text)


if __name__ == '__main__':
    main()
