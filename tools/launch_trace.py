#!/usr/bin/env python3
"""Which C entry points a pass calls, in which order and with which non-pointer arguments -- for every batch form of the engine, at the
smallest shapes at which each route still differs from its neighbour, with a SHA-256 over what the pass returned and over the whole
gradient buffer.  Two runs of this file, one per build, show that a change of the host schedule moved no launch and no bit:

  python tools/launch_trace.py --out a.txt          # on one checkout
  python tools/launch_trace.py --out b.txt          # on the other (the file needs nothing but the public package surface)
  python tools/launch_trace.py --compare a.txt b.txt [a2.txt]   # a2: a second run on a's checkout; a form whose hash differs between
                                                                # a and a2 is reported and held to trace equality only

Every function of the loaded library object (`hip.lib()`) is wrapped; a pointer argument is recorded as `*` (`0` when NULL), every other
argument by value; for `ecgvit_gemm*` the scalar fields of the descriptor are written out.  One training forward + backward per form, the host
RNG seeded per form (so the dropout seeds are arguments like any other).  Shapes: C = 12, P = 4, d = 128, h = 2, f = 256, 2 layers, K = 5,
max_signal_length = 1000 (251 tokens), 4 records, hidden / embedding dropout 0.1; the fp8_linear form d = 512, h = 8, f = 1024, 16 records
(4 016 token rows: the 8-bit routes switch on at 2 048 rows and take products of K >= 384 only), two steps (the second runs on delayed
scales and the 8-bit emitting kernels).
The fused steps (`HipTrainStep.step` / `step_masked` unsplit and at micro_batch_size = 3 -- passes of 3 and 1 records, the short one last --, the
frozen linear probe, `HipProbeStep.step`) run two optimiser steps each, so the second step's count and lr are arguments in the trace, and hash
the loss, the outputs, the gradient buffer and the parameter buffer after each step.  The f32 supervised step at micro_batch_size = 3 runs at
dropout 0: the f32 attention dropout kernel takes B h N^2 in multiples of 8 only, which 251 tokens and 2 heads meet at B = 4 but not at 3 or 1.
Before anything is wrapped the file also times the host: forward + backward of the bf16 uniform form and the unsplit `HipTrainStep.step` on it
(sync_nonfinite=False), no synchronisation inside the loop.
usage: python tools/launch_trace.py [--out FILE] [--host-iters 300] | --compare A B [A2]"""
import argparse
import ctypes
import hashlib
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LENGTHS = (1000, 400, 12, 4)
RAW = (997, 401, 4, 1)   # 4 pads to 8 and 997 to 1000: the multiple-of-patch case and the width limit


# ------------------------------------------------------------------------------------------------ recording
def _is_pointer(t):
    return t is ctypes.c_void_p or t is ctypes.c_char_p or (isinstance(t, type) and issubclass(t, ctypes._Pointer))


def _scalar(v):
    return repr(float(v)) if isinstance(v, float) else str(int(v))


def _desc_fields(d):
    out = []
    for name, typ in d._fields_:
        v = getattr(d, name)
        out.append(f'{name}={"*" if v else "0"}' if typ is ctypes.c_void_p else f'{name}={_scalar(v)}')
    return out


def wrap_library(l, sink):
    """replace every function of the library object by a recorder around it; returns the originals (name -> function).  The functions are
    those the object has cached as attributes: `hip.lib()` touches every name of `hip.SIGNATURES` when it loads the library, so that is all
    of them -- an entry point fetched later by a plain getattr, outside SIGNATURES, would have no argtypes and is NOT recorded"""
    originals = {n: f for n, f in vars(l).items() if isinstance(f, l._FuncPtr)}
    for name, fn in originals.items():
        def rec(*args, _name=name, _fn=fn):
            parts = []
            for a, t in zip(args, _fn.argtypes or ()):
                if isinstance(t, type) and issubclass(t, ctypes._Pointer) and hasattr(a, '_obj'):   # byref(descriptor)
                    parts += _desc_fields(a._obj)
                elif _is_pointer(t):
                    parts.append('*' if a else '0')
                else:
                    parts.append(_scalar(a))
            sink.append(f'{_name}({", ".join(parts)})')
            return _fn(*args)
        setattr(l, name, rec)
    return originals


def unwrap_library(l, originals):
    for name, fn in originals.items():
        setattr(l, name, fn)


def digest(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        t = t.detach().contiguous()
        h.update(f'{tuple(t.shape)}{t.dtype}'.encode())
        h.update(t.cpu().reshape(-1).view(torch.uint8).numpy().tobytes())
    return h.hexdigest()


# ------------------------------------------------------------------------------------------------ the forms
def config(E, d=128, h=2, f=256, drop=0.1):
    return E.EcgVitConfig(max_signal_length=1000, patch_size=4, hidden_size=d, num_hidden_layers=2, num_attention_heads=h,
                          intermediate_size=f, hidden_dropout_prob=drop, attention_probs_dropout_prob=drop)


def model_of(E, dtype, xf=None, masked=False, fp8=False, drop=0.1):
    torch.manual_seed(1234)
    m = E.EcgVit(num_class=5, config=config(E, 512, 8, 1024) if fp8 else config(E, drop=drop), compute_dtype=dtype, fp8_linear=fp8)
    if xf is not None:
        m.set_input_transform(xf)
    w = E.MaskedEcgVit(m, mask_ratio=0.5) if masked else m
    w.cuda().train()
    return w


def transform(E, per_record):
    g = torch.Generator().manual_seed(5)
    return E.FusedInputTransform(torch.randn(12, generator=g), torch.rand(12, generator=g) + 0.5, 4, timeout=True, per_record=per_record)


def records(B, width, seed=77):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, 12, width, generator=g), (torch.rand(B, 5, generator=g) > 0.5).float()


def ragged(x, lengths):
    return torch.cat([x[b, :, :l] for b, l in enumerate(lengths)], dim=1).contiguous()


def grads(m):
    """every gradient of the model as the engine holds them: the views of its flat gradient buffer, in layout order"""
    return list(m._engine().G32.values())


def supervised(E, dtype, x, lengths=None, xf=None, fused_step=False, fp8=False, steps=1):
    """model(x, labels).loss.backward() (the full last block), or HipTrainStep.step (CLS rows only in the last block on the bf16 engine)"""
    m = model_of(E, dtype, xf, fp8=fp8)
    x, y = x.cuda(), records(x.shape[0] if x.dim() == 3 else len(lengths), 4)[1].cuda()
    lt = None if lengths is None else torch.tensor(lengths, dtype=torch.int64)
    out = []
    if fused_step:
        step = E.HipTrainStep(m, dict(n_step=10), sync_nonfinite=True)
        for _ in range(steps):
            loss, logits = step.step(x, y, lengths=lt)
            out += [loss, logits] + [t.clone() for t in grads(m) + list(m._engine().P32.values())]
        return out
    o = m(sample_values=x, labels=y, lengths=lt)
    o.loss.backward()
    return [o.loss, o.logits] + grads(m)


def masked(E, dtype, x, lengths=None, xf=None):
    w = model_of(E, dtype, xf, masked=True)
    g = torch.Generator().manual_seed(9)
    if lengths is None:
        o = w(x.cuda(), w.random_mask_indices(x.shape[0], generator=g))
    else:
        idx, counts = w.random_mask_indices_varlen(torch.tensor(lengths), generator=g)
        o = w(x.cuda(), idx, lengths=torch.tensor(lengths, dtype=torch.int64), mask_counts=counts)
    o.loss.backward()
    return [o.loss, o.logits] + grads(w.encoder)


def state(m):
    """copies of every gradient and every parameter as the engine holds them"""
    return [t.clone() for t in grads(m) + list(m._engine().P32.values())]


def fused(E, dtype, x, lengths=None, xf=None, mb=None, loss_weight=None, head_only=False, drop=0.1):
    """two `HipTrainStep.step` calls on 4 records; head_only: every parameter but vit.mlp_head.* frozen (span kernels, truncated backward)"""
    m = model_of(E, dtype, xf, drop=drop)
    m.loss_weight = loss_weight
    if head_only:
        for n, p in m.named_parameters():
            p.requires_grad_(n.startswith('vit.mlp_head.'))
    x, y = x.cuda(), records(4, 4)[1].cuda()
    lt = None if lengths is None else torch.tensor(lengths, dtype=torch.int64)
    step = E.HipTrainStep(m, dict(n_step=10), sync_nonfinite=True)
    out = []
    for _ in range(2):
        loss, logits = step.step(x, y, lengths=lt, micro_batch_size=mb)
        out += [loss, logits] + state(m)
    return out


def fused_masked(E, dtype, x, lengths=None, xf=None, mb=None):
    """two `HipTrainStep.step_masked` calls on 4 records, the mask of `masked`"""
    w = model_of(E, dtype, xf, masked=True)
    g = torch.Generator().manual_seed(9)
    kw = {}
    if lengths is None:
        idx = w.random_mask_indices(x.shape[0], generator=g)
    else:
        idx, counts = w.random_mask_indices_varlen(torch.tensor(lengths), generator=g)
        kw = dict(lengths=torch.tensor(lengths, dtype=torch.int64), mask_counts=counts)
    step = E.HipTrainStep(w, dict(n_step=10), sync_nonfinite=True)
    out = []
    for _ in range(2):
        loss, pred = step.step_masked(x.cuda(), idx, micro_batch_size=mb, **kw)
        out += [loss, pred] + state(w.encoder)
    return out


def probe(E, dtype, x):
    """two `HipProbeStep.step` calls on the cached features of 4 records"""
    m = model_of(E, dtype)
    feats, y = m.encode(x.cuda(), norm=False), records(4, 4)[1].cuda()
    step = E.HipProbeStep(m, dict(n_step=10), sync_nonfinite=True)
    out = [feats]
    for _ in range(2):
        loss, logits = step.step(feats, y)
        out += [loss, logits] + state(m)
    return out


def encode(E, x, lengths):
    m = model_of(E, torch.bfloat16)
    lt = torch.tensor(lengths, dtype=torch.int64)
    return [m.encode(x.cuda(), lengths=lt, pool=p, norm=n) for p, n in (('cls', True), ('mean', False))]


def rollout(E, x, lengths):
    m = model_of(E, torch.bfloat16)
    o = m.attention_rollout_batch(x.cuda(), lengths=torch.tensor(lengths, dtype=torch.int64))
    return [o.logits, o.maps, o.patch_counts]


def forms(E):
    bf16, f32 = torch.bfloat16, torch.float32
    x = records(4, 1000)[0]
    xr, xraw = ragged(x, LENGTHS), ragged(x, RAW)
    return [
        ('bf16 uniform, full width', lambda: supervised(E, bf16, x)),
        ('bf16 uniform, width 400', lambda: supervised(E, bf16, x[:, :, :400].contiguous())),
        ('bf16 lengths, padded', lambda: supervised(E, bf16, x, LENGTHS)),
        ('bf16 lengths, padded, cls_only_last (fused step)', lambda: supervised(E, bf16, x, LENGTHS, fused_step=True)),
        ('bf16 uniform, cls_only_last (fused step)', lambda: supervised(E, bf16, x, fused_step=True)),
        ('bf16 ragged', lambda: supervised(E, bf16, xr, LENGTHS)),
        ('bf16 raw records, padded', lambda: supervised(E, bf16, x, RAW, xf=transform(E, True))),
        ('bf16 raw records, padded, cls_only_last (fused step)', lambda: supervised(E, bf16, x, RAW, xf=transform(E, True), fused_step=True)),
        ('bf16 raw records, ragged', lambda: supervised(E, bf16, xraw, RAW, xf=transform(E, True))),
        ('bf16 whole-batch fused transform', lambda: supervised(E, bf16, x[:, :, :997].contiguous(), xf=transform(E, False))),
        ('bf16 masked, rectangular', lambda: masked(E, bf16, x)),
        ('bf16 masked, lengths, padded', lambda: masked(E, bf16, x, LENGTHS)),
        ('bf16 masked, ragged', lambda: masked(E, bf16, xr, LENGTHS)),
        ('bf16 masked, raw records, ragged', lambda: masked(E, bf16, xraw, RAW, xf=transform(E, True))),
        ('f32 uniform', lambda: supervised(E, f32, x)),
        ('f32 lengths, padded', lambda: supervised(E, f32, x, LENGTHS)),
        ('f32 masked, rectangular', lambda: masked(E, f32, x)),
        ('bf16 encode cls + mean, lengths, padded', lambda: encode(E, x, LENGTHS)),
        ('bf16 encode cls + mean, ragged', lambda: encode(E, xr, LENGTHS)),
        ('bf16 attention_rollout_batch, ragged', lambda: rollout(E, xr, LENGTHS)),
        ('fp8_linear uniform, 16 records, two fused steps', lambda: supervised(E, bf16, records(16, 1000)[0], fused_step=True, fp8=True, steps=2)),
        ('step bf16 uniform, mb=3', lambda: fused(E, bf16, x, mb=3)),
        ('step bf16 lengths, padded, mb=3', lambda: fused(E, bf16, x, LENGTHS, mb=3)),
        ('step bf16 ragged, mb=3', lambda: fused(E, bf16, xr, LENGTHS, mb=3)),
        ('step bf16 raw records, padded, mb=3', lambda: fused(E, bf16, x, RAW, xf=transform(E, True), mb=3)),
        ('step bf16 uniform, loss_weight', lambda: fused(E, bf16, x, loss_weight=[0.3, 2.0])),
        ('step bf16 uniform, loss_weight, mb=3', lambda: fused(E, bf16, x, loss_weight=[0.3, 2.0], mb=3)),
        ('step bf16 uniform, mb=4 (one pass)', lambda: fused(E, bf16, x, mb=4)),
        ('step f32 uniform, mb=3, dropout 0', lambda: fused(E, f32, x, mb=3, drop=0.0)),
        ('step_masked bf16 rectangular', lambda: fused_masked(E, bf16, x)),
        ('step_masked bf16 rectangular, mb=3', lambda: fused_masked(E, bf16, x, mb=3)),
        ('step_masked bf16 lengths, padded', lambda: fused_masked(E, bf16, x, LENGTHS)),
        ('step_masked bf16 lengths, padded, mb=3', lambda: fused_masked(E, bf16, x, LENGTHS, mb=3)),
        ('step_masked bf16 ragged', lambda: fused_masked(E, bf16, xr, LENGTHS)),
        ('step_masked bf16 ragged, mb=3', lambda: fused_masked(E, bf16, xr, LENGTHS, mb=3)),
        ('step_masked bf16 raw records, ragged, mb=3', lambda: fused_masked(E, bf16, xraw, RAW, xf=transform(E, True), mb=3)),
        ('step_masked bf16 lengths all full width, equal counts (as_rectangular)', lambda: fused_masked(E, bf16, x, (1000,) * 4)),
        ('step_masked f32 rectangular, mb=3', lambda: fused_masked(E, f32, x, mb=3)),
        ('step bf16 frozen linear probe', lambda: fused(E, bf16, x, head_only=True)),
        ('step bf16 frozen linear probe, mb=3', lambda: fused(E, bf16, x, head_only=True, mb=3)),
        ('HipProbeStep bf16', lambda: probe(E, bf16, x)),
        ('HipProbeStep f32', lambda: probe(E, f32, x)),
    ]


def host_time(E, iters, fused_step=False):
    """host microseconds per forward + backward of the bf16 uniform form, or (fused_step) per unsplit `HipTrainStep.step` on it with
    sync_nonfinite=False: the loop only enqueues (nothing inside it waits for the device)"""
    m = model_of(E, torch.bfloat16)
    x, y = (t.cuda() for t in records(4, 1000))
    step = E.HipTrainStep(m, dict(n_step=iters + 20), sync_nonfinite=False)

    def one():
        if fused_step:
            step.step(x, y)
        else:
            m(sample_values=x, labels=y).loss.backward()
    for _ in range(20):
        one()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        one()
    t1 = time.perf_counter()
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    return (t1 - t0) / iters * 1e6, (t2 - t0) / iters * 1e6


# ------------------------------------------------------------------------------------------------ comparing two outputs
def parse(path):
    """{form: (trace lines, sha256)} of an output file"""
    out, name = {}, None
    with open(path) as fh:
        for ln in fh.read().splitlines():
            if ln.startswith('== '):
                name = ln[3:]
                out[name] = ([], None)
            elif ln.startswith('sha256 ') and name is not None:
                out[name] = (out[name][0], ln.split()[1])
                name = None
            elif name is not None:
                out[name][0].append(ln)
    return out


def compare(a, b, a2=None):
    """prints one line per form; returns the number of forms whose trace or hash differs.  a2: a second run of the build that wrote `a`:
    a form whose hash differs between a and a2 is not reproducible on that build itself, is reported as such and held to its trace only"""
    A, B = parse(a), parse(b)
    unstable = set()
    if a2 is not None:
        A2 = parse(a2)
        unstable = {n for n in A if n not in A2 or A2[n][1] != A[n][1]}
    bad = 0
    for name in sorted(set(A) | set(B), key=lambda n: list(A).index(n) if n in A else len(A)):
        if name not in A or name not in B:
            print(f'{name}: only in {a if name in A else b}')
            bad += 1
            continue
        (ta, ha), (tb, hb) = A[name], B[name]
        same_t = ta == tb
        first = next((i for i, (u, v) in enumerate(zip(ta, tb)) if u != v), min(len(ta), len(tb)))
        held = name not in unstable
        print(f'{name}: trace {"identical (" + str(len(ta)) + " calls)" if same_t else f"DIFFERS at call {first} ({len(ta)} / {len(tb)} calls)"}; '
              f'sha256 {"equal" if ha == hb else "DIFFERS"}' + ('' if held else f' (not held: differs between {a} and {a2} too)'))
        if not same_t and first < min(len(ta), len(tb)):
            print(f'    {ta[first]}\n    {tb[first]}')
        bad += (not same_t) or (held and ha != hb)
    print(f'{len(A)} / {len(B)} forms; {bad} differ')
    return bad


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out')
    ap.add_argument('--host-iters', type=int, default=300)
    ap.add_argument('--compare', nargs='+', metavar='FILE', help='A B [A2]: B against A; A2 = a second run of the build that wrote A')
    a = ap.parse_args()
    if a.compare:
        if len(a.compare) not in (2, 3):
            ap.error('--compare takes A B [A2]')
        sys.exit(1 if compare(*a.compare) else 0)
    import ecg_representation_learning_amd as E
    from ecg_representation_learning_amd import hip
    import bench
    lines = [f'sources: bench.kernel_source_hash() = {bench.kernel_source_hash()}; {torch.cuda.get_device_name(0)}']
    if a.host_iters > 0:
        enq, tot = host_time(E, a.host_iters)
        lines.append(f'host: {enq:.1f} us per forward + backward to enqueue, {tot:.1f} us with the final synchronisation '
                     f'(bf16 uniform form, {a.host_iters} iterations)')
        enq, tot = host_time(E, a.host_iters, fused_step=True)
        lines.append(f'host: {enq:.1f} us per fused step (HipTrainStep.step, unsplit, sync_nonfinite=False) to enqueue, {tot:.1f} us with the '
                     f'final synchronisation (bf16 uniform form, {a.host_iters} iterations)')
    l = hip.lib()
    for name, run in forms(E):
        torch.manual_seed(4321)
        sink = []
        originals = wrap_library(l, sink)
        try:
            t0 = time.perf_counter()
            result = run()
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
        finally:
            unwrap_library(l, originals)
        lines += [f'== {name}'] + sink + [f'sha256 {digest(*result)}  ({len(sink)} calls, {dt:.2f} s)']
    text = '\n'.join(lines) + '\n'
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as fh:
            fh.write(text)


if __name__ == '__main__':
    main()
