#!/usr/bin/env python3
"""Fourier resampling on the device (csrc/resample.hip; `resample`) beside its two yardsticks, one GPU process.  No rate is fixed in advance.
  stores            512 x 12 x 5000 -> 2500 (500 Hz), 512 x 12 x 4096 -> 2560 (400 Hz), 1 x 12 x 462 600 -> 450 000 (257 Hz; INCART)
  the call          `resample(store, fqs)`: a host clock around the whole call to a device synchronise (tables made and uploaded, workspace
                    allocated, launches), and the launch sequence alone (`ecgvit_resample` on prepared tables, device events)
  scipy             `scipy.signal.resample` on the same f32 store on the host, as the reference calls it (single precision), one thread
  the HBM floor     the plan's bytes -- 32 per complex element and pass, 24 per element for pack and for unpack, 16 per bin read and written by
                    the spectrum map -- at the stream rate `ecgvit_pool_records` reaches in this run on f32 rows of equal bytes, every launch
                    on another tensor of a ring past the Infinity Cache
  per pass          every pass of both plans alone over the store's transforms (`ecgvit_tools_resample_pass` of the tools library), device
                    events: ms, bytes / time, specialised (registers) or generic (a thread per output, r inputs each)
Stores: beats + sway + Gaussian noise 0.05 (tools/denoise_long_rate.py `store`).  Warm-up, device events.  Writes profiles/r23_resample.txt (--out).
--chirp: the table behind `resample.CHIRP_DEFAULT` instead (`chirp_main`): per prime r of 7 .. 65 521 and two shapes, the launch sequence with the
input side on the dense route and on the chirp route (Bluestein), alternating in this one process, and the headline shapes 512 x 4999 -> 2499,
1 x 131 101 -> 65 550 beside 512 x 5000 -> 2500.  Writes profiles/r24_resample_chirp.txt (--out).
usage: python tools/resample_rate.py [--reps 5] [--chirp]"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import ecg_representation_learning_amd as E  # noqa: E402
from ecg_representation_learning_amd import hip  # noqa: E402
from ecg_representation_learning_amd.hip import check, lib, ptr, stream  # noqa: E402

C = 12
STORES = ((512, 5000, 500), (512, 4096, 400), (1, 462600, 257))


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


def stream_rate(nbytes, reps):
    """bytes / s of ecgvit_pool_records (mean pool) over f32 rows of about nbytes, a ring of tensors past the Infinity Cache"""
    d, b = 1024, 512
    n = max(1, nbytes // (4 * d * b))
    ring = [torch.randn(b * n, d, device='cuda') for _ in range(max(2, -(-640 * 2 ** 20 // (4 * d * b * n))))]
    out = torch.empty(b, d, device='cuda')
    turn = [0]

    def run():
        turn[0] += 1
        check(lib().ecgvit_pool_records(ptr(ring[turn[0] % len(ring)]), ptr(out), None, None, b, n, d, hip.POOL_MEAN, None, None, 1e-5, hip.F32, stream()),
              'ecgvit_pool_records')
    ms = min(timed(run, reps) for _ in range(3))
    return 4 * d * b * n / (ms * 1e-3), 4 * d * b * n


CHIRP_PRIMES = (7, 13, 31, 61, 127, 257, 509, 1021, 4099, 16411, 65521)
CHIRP_SHAPES = ((512, 5000, 2500), (1, 460000, 225000))     # records, the length the input side is near, the output length (built radices only)


def chirp_main(a):
    """--chirp: where the chirp route (Bluestein) overtakes the generic pass.  Per tabled prime r and shape: the input length is r k, k of built radices
    only, nearest the shape's length, so r is the plan's one generic radix; the output length has built radices only and runs the same plain passes on both routes,
    so the two launch sequences differ in the input side alone.  Both are timed in this one process, in alternating order, each window at
    least ~20 ms of calls between two device events; the table gives the median and the minimum over the rounds."""
    import importlib
    import bench
    import code_objects
    RS = importlib.import_module('ecg_representation_learning_amd.resample')
    L = lib()
    lines = []

    def note(s):
        lines.append(s)
        print(s, flush=True)

    def side(n, sign, chirp):
        tables = {}
        return RS._side_tables(n, sign, chirp, tables, torch.device('cuda'))

    def compare(R, n_in, n_out, routes):
        """routes: [(chirp_in, chirp_out)] -> {route: (median ms, min ms)}, max |route - first route| / max |x|"""
        x = torch.randn((R, C, n_in), device='cuda', generator=torch.Generator('cuda').manual_seed(24))
        src = torch.arange(R, device='cuda', dtype=torch.int64) * (C * n_in)
        dst = torch.arange(R, device='cuda', dtype=torch.int64) * (C * n_out)
        fns, outs = {}, {}
        for ci, co in routes:
            ti, to = side(n_in, -1, ci), side(n_out, 1, co)
            ws = torch.empty(L.ecgvit_resample_chirp_workspace(R, C, n_in, n_out, ci, co) // 8, dtype=torch.float64, device='cuda')
            out = torch.empty((R, C, n_out), device='cuda')
            outs[(ci, co)] = out

            def fn(ti=ti, to=to, ws=ws, out=out):
                check(L.ecgvit_resample_chirp(ptr(x), ptr(out), ptr(src), n_in, ptr(dst), n_out, R, C, n_in, n_out, ptr(ti[0]), ptr(to[0]),
                                              ptr(ti[1]), ptr(ti[2]), ptr(to[1]), ptr(to[2]), ptr(ws), stream()), 'ecgvit_resample_chirp')
            fns[(ci, co)] = fn
        inner = {k: max(1, min(64, int(20.0 / max(timed(f, 1), 1e-3)))) for k, f in fns.items()}       # (timed() warms each route up once)
        ms = {k: [] for k in fns}
        for rnd in range(a.reps):
            for k in (routes if rnd % 2 == 0 else routes[::-1]):
                ms[k].append(timed(fns[k], inner[k], warmup=0))
        first = outs[routes[0]]
        dev = max(float((outs[k] - first).abs().max()) for k in routes) / float(x.abs().max())
        return {k: (float(np.median(v)), min(v)) for k, v in ms.items()}, dev

    note(f'sources: bench.kernel_source_hash() = {bench.kernel_source_hash()}; {torch.cuda.get_device_name(0)}, '
         f'{torch.cuda.get_device_properties(0).multi_processor_count} CUs')
    note(f'ecgvit_resample_chirp, the launch sequence alone on prepared tables (device events); {a.reps} rounds per row, the routes in alternating order, '
         f'a window of ~20 ms of calls (at least one); ms per call: median (minimum); stores: Gaussian noise')
    for name, k in sorted(code_objects.kernels(hip.LIB_PATH).items()):
        if 'rs_' in name and ('chirp' in name or 'rs_scale' in name):
            note(f'    {name}: {k["vgpr_count"]} VGPRs, VGPR spills {k["vgpr_spill_count"]}, scratch {k["private_segment_fixed_size"]} B')
    wins = {r: [] for r in CHIRP_PRIMES}
    smooth = sorted(2 ** i * 3 ** j * 5 ** k for i in range(20) for j in range(13) for k in range(9) if 2 ** i * 3 ** j * 5 ** k <= 1 << 19)
    for R, near, n_out in CHIRP_SHAPES:
        note(f'shape {R} x {C} x ~{near} -> {n_out} (plan {RS.plan(n_out)}): the input side on the dense route (its plan, a generic pass of radix r) and on the chirp route')
        for r in CHIRP_PRIMES:
            n_in = r * min(smooth, key=lambda k: abs(r * k - near))
            if abs(n_in - near) > near // 5:
                note(f'    r = {r:6d}: no length within 20% of {near} has this factor: not measured at this shape')
                continue
            res, dev = compare(R, n_in, n_out, [(0, 0), (1, 0)])
            (d_med, d_min), (c_med, c_min) = res[(0, 0)], res[(1, 0)]
            wins[r].append(c_med < d_med)
            note(f'    r = {r:6d}: n_in = {n_in:7d} plan {RS.plan(n_in)}, M = {RS.chirp_length(n_in)} plan {RS.plan(RS.chirp_length(n_in))}: dense {d_med:9.3f} ({d_min:9.3f}) ms, '
                 f'chirp {c_med:9.3f} ({c_min:9.3f}) ms, dense / chirp {d_med / c_med:8.2f}; max |chirp - dense| / max |x| = {dev:.1e}')
            torch.cuda.empty_cache()
    crossover = None
    for r in reversed(CHIRP_PRIMES):
        if not (wins[r] and all(wins[r])):
            break
        crossover = r
    note(f'the chirp route wins at every measured shape for the tabled primes {[r for r in CHIRP_PRIMES if wins[r] and all(wins[r])]}; '
         f'the smallest tabled prime from which it wins at every measured shape, and at every larger tabled prime: {crossover} (CHIRP_DEFAULT)')
    note('headline shapes, same run (routes as (input side, output side)):')
    for R, n_in, n_out, routes in ((512, 5000, 2500, [(0, 0)]), (512, 4999, 2499, [(0, 0), (1, 0), (1, 1)]), (1, 131101, 65550, [(1, 0), (1, 1)])):
        res, dev = compare(R, n_in, n_out, routes)
        word = {0: 'plain / dense', 1: 'chirp'}
        for (ci, co), (med, mn) in res.items():
            note(f'    {R} x {C} x {n_in} -> {n_out} ({word[ci]}, {word[co]}): {med:9.3f} ({mn:9.3f}) ms')
        if len(routes) > 1:
            note(f'        max |route - first route| / max |x| = {dev:.1e}' + ('; the dense input side of 131 101 is refused (a prime above 65 536)' if n_in == 131101 else ''))
        torch.cuda.empty_cache()
    with open(a.out, 'w') as fh:
        fh.write('\n'.join(lines) + '\n')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--chirp', action='store_true', help='the dense / chirp crossover table (profiles/r24_resample_chirp.txt)')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if a.out is None:
        a.out = os.path.join(ROOT, 'profiles', 'r24_resample_chirp.txt' if a.chirp else 'r23_resample.txt')
    if a.chirp:
        return chirp_main(a)
    import importlib
    import bench
    import code_objects
    from denoise_long_rate import store
    from scipy import signal
    from toolslib import tools_lib, TOOLS_LIB_PATH
    RS = importlib.import_module('ecg_representation_learning_amd.resample')
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    lines = []

    def note(s):
        lines.append(s)
        print(s, flush=True)

    note(f'sources: bench.kernel_source_hash() = {bench.kernel_source_hash()}; {torch.cuda.get_device_name(0)}, {cus} CUs')
    note(f'{a.reps} calls after one warm-up, device events unless a host clock is named; stores: beats + sway + Gaussian noise 0.05')
    for name, k in sorted(code_objects.kernels(TOOLS_LIB_PATH).items()):
        if any(f'rs_{w}_kernel' in name for w in ('pack', 'unpack', 'map', 'pass', 'generic')):
            note(f'    {name}: {k["vgpr_count"]} VGPRs, VGPR spills {k["vgpr_spill_count"]}, scratch {k["private_segment_fixed_size"]} B')
    tl = tools_lib()
    for n, L, fqs in STORES:
        num = E.resampled_length(L, fqs, 250)
        x = store(n, L, 23)
        T = n * C // 2
        plan_in, plan_out = E.resample_plan(L), E.resample_plan(num)
        note(f'store {n} x {C} x {L} f32 = {x.numel() * 4 / 1e6:.1f} MB at {fqs} Hz -> {num} samples at 250 Hz; {T} transforms; plans {plan_in} and {plan_out}')
        # the whole call, host clock
        y = E.resample(x, fqs)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.reps):
            y = E.resample(x, fqs)
        torch.cuda.synchronize()
        call_ms = (time.perf_counter() - t0) * 1e3 / a.reps
        # the launch sequence alone
        tw_in, tw_out = (torch.from_numpy(RS.twiddles(L, -1)).cuda(), torch.from_numpy(RS.twiddles(num, 1)).cuda())
        ws = torch.empty(lib().ecgvit_resample_workspace(n, C, L, num) // 8, dtype=torch.float64, device='cuda')
        src = torch.arange(n, device='cuda', dtype=torch.int64) * (C * L)
        dst = torch.arange(n, device='cuda', dtype=torch.int64) * (C * num)
        out = torch.empty((n, C, num), device='cuda')

        def seq():
            check(lib().ecgvit_resample(ptr(x), ptr(out), ptr(src), L, ptr(dst), num, n, C, L, num, ptr(tw_in), ptr(tw_out), ptr(ws), stream()), 'ecgvit_resample')
        seq_ms = min(timed(seq, a.reps) for _ in range(3))
        assert torch.equal(out, y)
        # scipy on the host, one thread (scipy.fft's default)
        xh = x.cpu().numpy()
        k = min(n, 32)
        t0 = time.perf_counter()
        yh = signal.resample(xh[:k], num, axis=-1)
        sc_ms = (time.perf_counter() - t0) * 1e3 / k
        err = float(np.abs(out[:k].cpu().numpy().astype(np.float64) - yh).max()) / float(np.abs(xh[:k]).max())
        # the floor
        el_in, el_out = T * L, T * num
        nbytes = 24 * el_in + 32 * el_in * len(plan_in) + 16 * (min(el_in, el_out) + el_out) + 32 * el_out * len(plan_out) + 24 * el_out
        rate, rate_bytes = stream_rate(x.numel() * 4, a.reps)
        floor_ms = nbytes / rate * 1e3
        note(f'    resample(store, {fqs}), host clock to a synchronise   {call_ms:9.3f} ms   {n / call_ms * 1e3:10.0f} records/s')
        note(f'    ecgvit_resample, the launch sequence alone            {seq_ms:9.3f} ms   {n / seq_ms * 1e3:10.0f} records/s   '
             f'({3 + len(plan_in) + len(plan_out)} launches)')
        note(f'    scipy.signal.resample, f32, one thread                {sc_ms * n:9.1f} ms   ({sc_ms:.3f} ms per record of 12 leads over {k} records; '
             f'launch sequence x {sc_ms * n / seq_ms:.0f}; max |device - scipy f32| / max |x| = {err:.1e})')
        note(f'    HBM floor of the plan: {nbytes / 1e9:.3f} GB at {rate / 1e12:.2f} TB/s (ecgvit_pool_records over {rate_bytes / 1e6:.0f} MB of f32 rows) = '
             f'{floor_ms:.3f} ms; the launch sequence is {seq_ms / floor_ms:.2f} x the floor')
        a_buf, b_buf = ws[:2 * T * max(L, num)], ws[2 * T * max(L, num):]
        tot = {'specialised': 0.0, 'generic': 0.0}
        for length, plan, tw in ((L, plan_in, tw_in), (num, plan_out, tw_out)):
            Ns = 1
            for r in plan:
                ms = min(timed(lambda: check(tl.ecgvit_tools_resample_pass(ptr(a_buf), ptr(b_buf), ptr(tw), length, T, Ns, r, stream()), 'pass'), a.reps)
                         for _ in range(2))
                kind = 'specialised' if r in RS.BUILT_RADICES else 'generic'
                tot[kind] += ms
                note(f'        length {length:7d} radix {r:4d} after {Ns:7d} ({kind:11s}) {ms:9.3f} ms   {32 * T * length / (ms * 1e-3) / 1e12:6.2f} TB/s of its 32 B per element'
                     + (f'   ({r} inputs per output: {16 * r * T * length / (ms * 1e-3) / 1e12:.2f} TB/s of loads)' if kind == 'generic' else ''))
                Ns *= r
        rest = seq_ms - tot['specialised'] - tot['generic']
        note(f'    passes: specialised {tot["specialised"]:.3f} ms, generic {tot["generic"]:.3f} ms'
             + (f' ({tot["generic"] / seq_ms:.0%} of the launch sequence)' if tot['generic'] else '') + f'; pack, spectrum map, unpack and gaps {rest:.3f} ms')
        del x, y, ws, out, a_buf, b_buf
        torch.cuda.empty_cache()
    text = '\n'.join(lines) + '\n'
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as fh:
        fh.write(text)


if __name__ == '__main__':
    main()
