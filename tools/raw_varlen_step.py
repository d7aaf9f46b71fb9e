#!/usr/bin/env python3
"""Raw records of unequal length through the fused per-record input transform (`FusedInputTransform(per_record=True)`), one GPU process,
EcgVit-base, bf16, patch 20, B = 512, raw lengths uniform in [50 %, 100 %] of 5000 and the near-full mix [95 %, 100 %]:
  (a) `ecgvit_patch_gather_transform_varlen` alone (us per launch, HIP events over a loop) on the ragged raw batch and on the padded one,
      against `ecgvit_patch_gather_transform` on a rectangular batch of the same number of samples: HBM streams of the same bytes;
  (b) the ragged supervised step fed raw records through the fused transform, against what the caller had to do before it existed: the same
      records normalised, zero-padded per record and re-concatenated with torch ops on the device INSIDE the timed region -- a loop over
      the records, and the cheapest batched form (one normalise over (C, S), one index scatter into zeros; its index built per batch on
      the host) -- then the ragged step without a transform.  TimeOut off in all three (the torch forms do not apply it).
Writes profiles/r15_raw_varlen_step.txt (--out).
usage: python tools/raw_varlen_step.py [--runs 2] [--steps 5] [--warmup 2]"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ecg_representation_learning_amd as E  # noqa: E402
from ecg_representation_learning_amd.engine import RaggedBatch, RawPaddedBatch, check_raw_lengths  # noqa: E402
from ecg_representation_learning_amd.hip import lib, check, ptr, stream  # noqa: E402

L, P, B, C = 5000, 20, 512, 12
CASES = (('[50 %, 100 %] of 5000', 0.5), ('near-full: [95 %, 100 %]', 0.95))


def draw_raw(lo_frac, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(int(L * lo_frac), L, (B,), generator=g)   # < L: the padded length stays <= max_signal_length


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


def host_loop(x, raw, mean, inv_std):
    """per record: normalise, zero-pad to its own patch multiple (the reference's extra patch included), re-concatenate"""
    out = []
    for r in torch.split(x, raw.tolist(), dim=1):
        t = (r - mean) * inv_std
        out.append(torch.nn.functional.pad(t, (0, P - t.shape[1] % P)))
    return torch.cat(out, dim=1)


def host_batched(x, raw, padded, mean, inv_std):
    """one normalise over (C, S_raw), one scatter into zeros (C, S_padded); the destination index is built on the host per batch"""
    dst0 = torch.cumsum(padded, 0) - padded
    src0 = torch.cumsum(raw, 0) - raw
    idx = torch.arange(int(raw.sum())) + torch.repeat_interleave(dst0 - src0, raw)
    idx = idx.pin_memory().to(x.device, non_blocking=True)
    out = torch.zeros(C, int(padded.sum()), device=x.device)
    out[:, idx] = (x - mean) * inv_std
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=2)
    ap.add_argument('--steps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r15_raw_varlen_step.txt'))
    a = ap.parse_args()
    import bench
    dev = torch.device('cuda')
    mean = torch.linspace(-0.5, 0.5, C)
    std = torch.linspace(0.5, 2.0, C)
    xf = E.FusedInputTransform(mean, std, P, per_record=True)
    lines = [f'sources: bench.kernel_source_hash() = {bench.kernel_source_hash()}; {torch.cuda.get_device_name(0)}',
             f'EcgVit-base, bf16, patch {P}, B = {B}, raw record lengths uniform in the stated range of {L} samples']
    # (a) the gather kernels alone
    lines.append(f'(a) patch gather + transform alone, bf16 rows, us per launch over {a.reps} launches, two alternating passes: the per-record kernel on '
                 f'the ragged (12, S_raw) batch and on the padded (B, 12, {L}) batch, the rectangular kernel on (B, 12, S_raw / B)')
    m_d, i_d = xf.device_stats(dev)
    for ci, (name, lo) in enumerate(CASES):
        raw, padded = check_raw_lengths(draw_raw(lo, 1 + ci), xf, L)
        S = int(raw.sum())
        rg = RaggedBatch(padded, P, dev, raw)
        rp = RawPaddedBatch(raw, padded, P, C, L, dev)
        xr = torch.randn(C, S, device=dev)
        xp = torch.randn(B, C, L, device=dev)
        Lr = S // B
        Lrect = xf.padded_length(Lr)
        xq = torch.randn(B, C, Lr, device=dev)
        out = torch.empty(max(rg.M - B, B * (rp.width // P), B * (Lrect // P)), C * P, device=dev, dtype=torch.bfloat16)

        def varlen(x, rs):
            return lambda: check(lib().ecgvit_patch_gather_transform_varlen(
                ptr(x), ptr(out), ptr(rs.src_off), rs.lead_stride, ptr(rs.raw_len), ptr(rs.n_patch), ptr(rs.row_off), rs.nrows, rs.n_max, B, C, P,
                C * P, ptr(m_d), ptr(i_d), None, None, E.hip.BF16, stream()), 'varlen')
        rect = lambda: check(lib().ecgvit_patch_gather_transform(ptr(xq), ptr(out), B, C, Lr, Lrect, P, C * P, ptr(m_d), ptr(i_d), None, None,
                                                                 E.hip.BF16, stream()), 'rect')
        fns = (('ragged', varlen(xr, rg.rawside)), ('padded', varlen(xp, rp.rawside)), ('rect', rect))
        t = {k: [] for k, _ in fns}
        for r in range(2):
            for k, f in (fns if r == 0 else fns[::-1]):
                t[k].append(timed(f, a.reps))
        gb = (S * C * 4 + (S // P) * C * P * 2) / 1e9
        lines.append(f'  {name}: S_raw = {S} ({gb * 1e3:.0f} MB read + written)')
        for k in t:
            lines.append(f'    {k:7s} ' + ' '.join(f'{v:8.1f}' for v in t[k]) + f'   best {min(t[k]):8.1f} us   {gb / (min(t[k]) * 1e-6):7.0f} GB/s'
                         f'   x {min(t[k]) / min(t["rect"]):.3f} of rect')
        del xr, xp, xq, out
    # (b) the ragged supervised step
    lines.append(f'(b) ragged supervised step, dropout of the base config, {a.steps} steps per run after {a.warmup} warm-up steps, {a.runs} alternating runs '
                 f'(records/s): fused = raw (12, S_raw) + per-record transform; loop / batched = torch ops on the device inside the timed region '
                 f'(normalise, pad per record, re-concatenate), then the ragged step without a transform')
    for ci, (name, lo) in enumerate(CASES):
        conf, _ = bench.make_config(E, 'base', P, L, None)
        raw, padded = check_raw_lengths(draw_raw(lo, 1 + ci), xf, L)
        g = torch.Generator().manual_seed(2 + ci)
        xr = torch.randn(C, int(raw.sum()), generator=g).cuda()
        y = (torch.rand(B, 71, generator=g) < 0.05).float().cuda()
        torch.manual_seed(0)
        m_f = E.EcgVit(config=conf, compute_dtype=torch.bfloat16).cuda().train().set_input_transform(xf)
        torch.manual_seed(0)
        m_p = E.EcgVit(config=conf, compute_dtype=torch.bfloat16).cuda().train()
        s_f = E.HipTrainStep(m_f, dict(n_step=10 ** 6), sync_nonfinite=False)
        s_p = E.HipTrainStep(m_p, dict(n_step=10 ** 6), sync_nonfinite=False)
        mc, ic = m_d[:, None], i_d[:, None]
        forms = (('fused', lambda: s_f.step(xr, y, lengths=raw)),
                 ('loop', lambda: s_p.step(host_loop(xr, raw, mc, ic), y, lengths=padded)),
                 ('batched', lambda: s_p.step(host_batched(xr, raw, padded, mc, ic), y, lengths=padded)))
        res = {k: [] for k, _ in forms}
        for r in range(a.runs):
            for k, f in (forms if r % 2 == 0 else forms[::-1]):
                for _ in range(a.warmup):
                    f()
                res[k].append(B / (timed(f, a.steps) * 1e-6))
                print(f'{name}: run {r} {k:8s} {res[k][-1]:8.1f} records/s', flush=True)
        s_f.finish()
        s_p.finish()
        lines.append(f'  {name}: dropout {conf.hidden_dropout_prob}, mean raw length {float(raw.float().mean()):.0f}, {int(padded.sum()) // P + B} packed token rows')
        for k in res:
            v = res[k]
            lines.append(f'    {k:8s} ' + ' '.join(f'{r:8.1f}' for r in v) + f'   best {max(v):8.1f}   fused x {max(res["fused"]) / max(v):.3f} of this')
        del s_f, s_p, m_f, m_p, xr, y
        torch.cuda.empty_cache()
    text = '\n'.join(lines) + '\n'
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as fh:
        fh.write(text)


if __name__ == '__main__':
    main()
