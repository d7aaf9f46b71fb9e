#!/usr/bin/env python3
"""A/B of the LayerNorm entry points of TWO builds of the library in ONE process on ONE device: first every output of every case of
tests/layernorm_ref.py's lists through the six entry points, compared as bit patterns (differing elements and the largest distance in ulps of the
output's type); then HIP-event timings of the forward, the plain backward and the fused backward at p = 0.1 at the step's shapes, the two builds
interleaved per round (writing the same buffers, taking turns to go first), the first round discarded.  A row passes when the second build's median is at most the first's median plus the first's own
spread (max - min over its rounds).
usage: python tools/ln_ab.py [libA.so libB.so] [--rounds 11] [--iters 10] [--no-bits] [--no-time]; exit status 1 when a bit differs or a row is slower
(defaults: csrc/build/libecgvit_hip_prev.so, which `make prev` keeps, against the shipped library)"""
import argparse
import ctypes
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
from ecg_representation_learning_amd import hip  # noqa: E402
import layernorm_ref as R  # noqa: E402

ENTRIES = ('ecgvit_layernorm_fwd', 'ecgvit_layernorm_fwd_q8', 'ecgvit_layernorm_bwd_workspace', 'ecgvit_layernorm_bwd', 'ecgvit_layernorm_bwd_fused',
           'ecgvit_layernorm_bwd_fused_rowpitch', 'ecgvit_layernorm_bwd_fused_q8')
SEED = 0x5EED0BADC0FFEE
FILL = 0x5A                                   # every output starts as this byte in both builds: what a build leaves alone compares equal


def load(path):
    lib = ctypes.CDLL(path)
    for name in ENTRIES:
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = hip.SIGNATURES[name]
    return lib


def P(t):
    return None if t is None else t.data_ptr()


def out(shape, dtype):
    t = torch.empty(shape, device='cuda', dtype=dtype)
    t.view(torch.uint8).fill_(FILL)
    return t


class Case:
    """one shape's device inputs; mean / rstd for the backward come from the FIRST build's forward, so that the backward is compared alone"""

    def __init__(self, rows, d, dtype, libs, random=False):
        self.rows, self.d, self.dtype, self.libs = rows, d, dtype, libs
        if random:                                # the timing shapes: plain normal data, drawn on the device
            g = torch.Generator(device='cuda').manual_seed(rows * 4099 + d)
            t = {k: torch.randn(rows, d, device='cuda', generator=g).to(dtype) for k in ('x', 'dy', 'dres')}
            t['gamma'], t['beta'] = torch.randn(d, device='cuda', generator=g), torch.randn(d, device='cuda', generator=g)
        else:
            t = {k: v.cuda() for k, v in R.ln_inputs(rows, d, dtype).items()}
        self.t = t
        self.code = hip.BF16 if dtype == torch.bfloat16 else hip.F32
        self.exact = R.kernel_form(d, dtype)[0] == 'fit'
        self.ws = torch.empty(max(libs[0].ecgvit_layernorm_bwd_workspace(rows, d), 16), device='cuda', dtype=torch.uint8)
        self.one = torch.ones(1, device='cuda')
        self.stats = None

    def st(self):
        return torch.cuda.current_stream().cuda_stream

    def fwd(self, lib, o=None, q8=False, with_y=True, scale=None):
        rows, d, t = self.rows, self.d, self.t
        o = o or dict(y=out((rows, d), self.dtype), mean=out((rows,), torch.float32), rstd=out((rows,), torch.float32))
        if q8:
            o.setdefault('y8', out((rows, d), torch.uint8))
            o.setdefault('amax', torch.zeros(1, device='cuda'))
            rc = lib.ecgvit_layernorm_fwd_q8(P(t['x']), P(t['gamma']), P(t['beta']), P(o['y']) if with_y else None, P(o['mean']), P(o['rstd']), rows, d,
                                             R.EPS, P(o['y8']), P(scale), P(o['amax']), self.st())
        else:
            rc = lib.ecgvit_layernorm_fwd(P(t['x']), P(t['gamma']), P(t['beta']), P(o['y']), P(o['mean']), P(o['rstd']), rows, d, R.EPS, self.code, self.st())
        assert rc == 0, ('forward', rows, d, self.dtype, q8, rc)
        return o

    def bwd(self, lib, form, o=None, dres=True, p=0.0, pitch=1, with_dxm=True, scale=None):
        """form: 'bwd' | 'fused' | 'rowpitch' | 'q8'"""
        rows, d, t = self.rows, self.d, self.t
        if self.stats is None:
            s = self.fwd(self.libs[0])
            self.stats = (s['mean'], s['rstd'])
        mean, rstd = self.stats
        if o is None:
            o = dict(dx=out((rows, d), self.dtype), dgamma=out((d,), torch.float32), dbeta=out((d,), torch.float32))
            if form != 'bwd':
                o.update(dxm=out((rows, d), self.dtype), dcolsum=out((d,), torch.float32))
            if form == 'q8':
                o.update(g8=out((rows, d), torch.uint8), amax=torch.zeros(1, device='cuda'))
        a = (P(t['dy']), P(t['x']), P(t['gamma']), P(mean), P(rstd), P(t['dres']) if dres else None, P(o['dx']), P(o['dgamma']), P(o['dbeta']), P(self.ws), rows, d)
        if form == 'bwd':
            rc = lib.ecgvit_layernorm_bwd(*a, self.code, self.st())
        elif form == 'fused':
            rc = lib.ecgvit_layernorm_bwd_fused(*a, P(o['dxm']), P(o['dcolsum']), p, SEED, self.code, self.st())
        elif form == 'rowpitch':
            rc = lib.ecgvit_layernorm_bwd_fused_rowpitch(*a, P(o['dxm']), P(o['dcolsum']), p, SEED, pitch, self.code, self.st())
        else:
            rc = lib.ecgvit_layernorm_bwd_fused_q8(*a, P(o['dxm']) if with_dxm else None, P(o['dcolsum']), p, SEED, P(o['g8']), P(scale), P(o['amax']), self.st())
        assert rc == 0, (form, rows, d, self.dtype, p, rc)
        return o


def ordered(t):
    """the bit pattern as an integer that rises with the value (floats), or the byte itself"""
    if t.dtype == torch.uint8:
        return t.to(torch.int64)
    b = t.view(torch.int16 if t.element_size() == 2 else torch.int32).to(torch.int64)
    return torch.where(b < 0, -(b & (0x7FFF if t.element_size() == 2 else 0x7FFFFFFF)), b)


def shapes():
    s = []
    for dt in R.DTYPES:
        s += [(r, d, dt) for d in R.WIDTHS for r in R.WIDTH_ROWS]
        s += [(r, d, dt) for d in R.ROW_WIDTHS for r in R.ROW_COUNTS]
        s += [(r, d, dt) for d in R.CAPPED_WIDTHS for r in (R.CAPPED_BWD_ROWS, R.CAPPED_FWD_ROWS)]
        s += [(r, d, dt) for d in R.FUSED_WIDTHS[dt] for r in R.FUSED_ROWS]
    s += [(r, d, torch.bfloat16) for d in R.Q8_WIDTHS for r in set(R.Q8_FWD_ROWS + R.Q8_BWD_ROWS)]
    return sorted(set(s), key=lambda c: (str(c[2]), c[1], c[0]))


def compare_bits(libs):
    """every shape of the lists through every entry point and option that accepts it"""
    tally, differing = {}, []
    for rows, d, dt in shapes():
        k = Case(rows, d, dt, libs)
        scale = torch.full((1,), 0.02, device='cuda')
        runs = [('ecgvit_layernorm_fwd', '', lambda l: k.fwd(l))]
        for dres in (False, True):
            runs.append(('ecgvit_layernorm_bwd', f'dres={int(dres)}', lambda l, dres=dres: k.bwd(l, 'bwd', dres=dres)))
            for p in R.FUSED_P[dt]:
                runs.append(('ecgvit_layernorm_bwd_fused', f'dres={int(dres)} p={p}', lambda l, dres=dres, p=p: k.bwd(l, 'fused', dres=dres, p=p)))
        for p in R.FUSED_P[dt]:
            runs.append(('ecgvit_layernorm_bwd_fused_rowpitch', f'p={p} pitch={R.PITCH}', lambda l, p=p: k.bwd(l, 'rowpitch', p=p, pitch=R.PITCH)))
        if k.exact:
            for wy in (True, False):
                runs.append(('ecgvit_layernorm_fwd_q8', f'y={int(wy)}', lambda l, wy=wy: k.fwd(l, q8=True, with_y=wy, scale=scale)))
            for p in R.FUSED_P[dt]:
                for wd in (True, False):
                    runs.append(('ecgvit_layernorm_bwd_fused_q8', f'p={p} dxm={int(wd)}', lambda l, p=p, wd=wd: k.bwd(l, 'q8', p=p, with_dxm=wd, scale=scale)))
        form = '%s %d' % R.kernel_form(d, dt)
        for entry, opt, f in runs:
            a, b = f(libs[0]), f(libs[1])
            torch.cuda.synchronize()
            for name in a:
                n = tally.setdefault((entry, name), [0, 0, 0])
                n[0] += 1
                n[1] += a[name].numel()
                if not torch.equal(a[name].view(torch.uint8), b[name].view(torch.uint8)):
                    diff = (ordered(a[name]) - ordered(b[name])).abs()
                    n[2] += 1
                    differing.append(f'    {entry} {R.dtype_id(dt)} {rows} x {d} ({form}) {opt}: {name} differs in {int((diff != 0).sum())} of {a[name].numel()} '
                                     f'elements, by at most {int(diff.max())} ulp')
    print('bits, first build against second, per entry point and output: cases, elements, cases with any differing element')
    for (entry, name), (c, e, bad) in sorted(tally.items()):
        print(f'    {entry:38s} {name:8s} {c:5d} cases {e:12d} elements   {bad} differ')
    print('\n'.join(differing) if differing else '    every output of every case has the same bits in both builds')
    return not differing


TIMED = [  # (label, dtype, rows, d, emitting forms)
    ('bf16 exact-lane kernels, base step', torch.bfloat16, 128512, 768, False),
    ('bf16 exact-lane kernels + Q8 forms, fp8-large step', torch.bfloat16, 128256, 1024, True),
    ('f32 generic kernels MAXV 4', torch.float32, 128512, 768, False),
    ('bf16 generic kernels MAXV 1', torch.bfloat16, 128512, 128, False),
    ('f32 generic kernels MAXV 1', torch.float32, 128512, 128, False),
    ('bf16 generic kernels MAXV 1', torch.bfloat16, 8032, 128, False),
    ('f32 generic kernels MAXV 1', torch.float32, 8032, 128, False),
]


def time_rows(libs, names, rounds, iters):
    ok = True
    print(f'timings: HIP events around {iters} launches, {rounds} rounds with the builds interleaved, the first round discarded; us per launch: median (min .. max)')
    for label, dt, rows, d, q8 in TIMED:
        k = Case(rows, d, dt, libs, random=True)
        scale = torch.full((1,), 0.02, device='cuda')
        forms = [('fwd', lambda l, o: k.fwd(l, o)), ('bwd', lambda l, o: k.bwd(l, 'bwd', o)), ('bwd_fused p=0.1', lambda l, o: k.bwd(l, 'fused', o, p=0.1))]
        if q8:
            forms += [('fwd_q8', lambda l, o: k.fwd(l, o, q8=True, scale=scale)), ('bwd_fused_q8 p=0.1', lambda l, o: k.bwd(l, 'q8', o, p=0.1, scale=scale))]
        for fname, f in forms:
            bufs = f(libs[0], None)                    # ONE set of outputs for both builds: two sets sit on different pages and channels, which
            f(libs[1], bufs)                           # alone moved instruction-identical kernels by 3 us of 100 (also the warm-up launch of either build)
            torch.cuda.synchronize()
            t = [[] for _ in libs]
            for rnd in range(rounds):
                for i in ((0, 1) if rnd % 2 == 0 else (1, 0)):   # the build that goes first alternates
                    l = libs[i]
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(iters):
                        f(l, bufs)
                    e1.record()
                    torch.cuda.synchronize()
                    t[i].append(1e3 * e0.elapsed_time(e1) / iters)
            v = [sorted(x[1:]) for x in t]
            med = [x[len(x) // 2] for x in v]
            spread = v[0][-1] - v[0][0]
            good = med[1] <= med[0] + spread
            ok &= good
            print(f'    {label:42s} {R.dtype_id(dt):4s} {rows:6d} x {d:4d} {fname:18s} ' +
                  '   '.join(f'{names[i]} {med[i]:8.1f} ({v[i][0]:8.1f} .. {v[i][-1]:8.1f})' for i in range(len(libs))) +
                  f'   second - first {med[1] - med[0]:+7.1f}, first\'s spread {spread:6.1f}: {"ok" if good else "SLOWER"}')
            del bufs
        del k
        torch.cuda.empty_cache()
    return ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('libs', nargs='*')
    ap.add_argument('--rounds', type=int, default=11)
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--no-bits', action='store_true')
    ap.add_argument('--no-time', action='store_true')
    a = ap.parse_args()
    pk = os.path.join(ROOT, 'ecg-representation-learning_amd')
    paths = a.libs or [os.path.join(pk, 'csrc', 'build', 'libecgvit_hip_prev.so'), os.path.join(pk, 'libecgvit_hip.so')]
    assert len(paths) == 2, 'two libraries'
    import bench
    print('kernel_source_sha16:', bench.kernel_source_hash(), '(sources of the tree; first build =', paths[0], ', second =', paths[1], ')', flush=True)
    libs = [load(p) for p in paths]
    ok = True
    if not a.no_bits:
        ok &= compare_bits(libs)
    if not a.no_time:
        ok &= time_rows(libs, ('first', 'second'), a.rounds, a.iters)
    print('ln_ab:', 'ok' if ok else 'DIFFERENCES (see above)')
    sys.exit(0 if ok else 1)


if __name__ == '__main__':
    main()
