"""-m gpu: frozen parameters (requires_grad=False) in the fused train step.

Frozen parameters stay bit-identical (no update, no decay, no moment update) on every engine form; the trainable ones, the loss and the
clip norm follow the reference sequence (`OracleTrainer`: torch's AdamW skips parameters without a gradient and keeps a step count per
parameter); the truncated backward neither reads nor writes the gradients it skips; the span kernels reduce to the whole-buffer ones; the
RCCL path with frozen layers equals the plain step."""
import math
import os
import socket

import pytest
import torch
import torch.distributed as dist

from hiputil import max_err
from oracle import vit_oracle as O
import ecg_representation_learning_amd as E
from ecg_representation_learning_amd import hip

pytestmark = pytest.mark.gpu
F32, BF16 = torch.float32, torch.bfloat16


def freeze(model, trainable):
    for n, p in model.named_parameters():
        p.requires_grad_(bool(trainable(n)))


def linear_probe(n):
    return n.startswith('vit.mlp_head.')


def top_blocks(k, ly):
    return lambda n: linear_probe(n) or any(n.startswith(f'vit.transformer.layers.{i}.') for i in range(ly - k, ly))


def bitfit(n):
    return n.endswith('.bias')


def _conf(d=256, h=4, f=512, ly=3, length=2000, drop=0.1):
    return E.EcgVitConfig(max_signal_length=length, patch_size=20, hidden_size=d, num_hidden_layers=ly, num_attention_heads=h,
                          intermediate_size=f, hidden_dropout_prob=drop, attention_probs_dropout_prob=drop)


def _frozen_run(model, trainable, steps, masked=False, B=24, length=2000):
    """`steps` fused steps with `trainable` -> {frozen name: (before, after)}, {trainable name: (before, after)}"""
    named = dict(model.named_parameters())
    freeze(model, trainable)
    before = {n: p.detach().clone() for n, p in named.items()}
    x, y = E.workload.synthetic_batch(B, length=length, seed=3)
    x, y = x.cuda(), y.cuda()
    st = E.HipTrainStep(model, dict(n_step=20, warmup_ratio=0.0), sync_nonfinite=True)
    torch.manual_seed(11)
    for _ in range(steps):
        if masked:
            st.step_masked(x, model.random_mask_indices(B, generator=torch.Generator().manual_seed(8)))
        else:
            st.step(x, y)
    st.finish()
    torch.cuda.synchronize()
    assert math.isfinite(st.grad_norm()) and st.grad_norm() > 0
    fro = {n: (before[n], p.detach()) for n, p in named.items() if not p.requires_grad}
    tra = {n: (before[n], p.detach()) for n, p in named.items() if p.requires_grad}
    return fro, tra


FORMS = {
    'f32': dict(conf=dict(d=64, h=2, f=128, length=400, drop=0.0), dtype=F32),
    'bf16': dict(conf=dict(), dtype=BF16),
    'fp8_linear': dict(conf=dict(d=512, h=8, f=1024, length=5000), dtype=BF16, fp8_linear=True, B=20),   # 5020 rows: the 8-bit kernels' floors
    'dh128': dict(conf=dict(h=2), dtype=BF16),
    'masked': dict(conf=dict(), dtype=BF16, masked=True),
}


@pytest.mark.parametrize('form', list(FORMS))
@pytest.mark.parametrize('setup', ['linear_probe', 'top1', 'bitfit'])
def test_frozen_parameters_stay_bit_identical(form, setup):
    spec = FORMS[form]
    c = spec['conf']
    torch.manual_seed(5)
    m = E.EcgVit(config=_conf(**c), compute_dtype=spec['dtype'], fp8_linear=spec.get('fp8_linear', False))
    trainable = {'linear_probe': linear_probe, 'top1': top_blocks(1, 3), 'bitfit': bitfit}[setup]
    if spec.get('masked'):
        if setup == 'linear_probe':   # the head takes no part in the masked objective: the pre-train head alone
            trainable = lambda n: n.startswith('to_pixels.')
        w = E.MaskedEcgVit(m, mask_ratio=0.5).cuda().train()
        fro, tra = _frozen_run(w, lambda n: trainable(n[len('encoder.'):] if n.startswith('encoder.') else n), 3, masked=True)
    else:
        m.cuda().train()
        fro, tra = _frozen_run(m, trainable, 3, B=spec.get('B', 24), length=c.get('length', 2000))
    assert fro and tra
    for n, (a, b) in fro.items():
        assert torch.equal(a, b), f'frozen {n} moved'
    moved = [n for n, (a, b) in tra.items() if not torch.equal(a, b)]
    assert len(moved) >= len(tra) // 2, moved     # (a parameter outside the objective is still decayed: it moves too)


def _parity_conf():
    return _conf(d=64, h=2, f=128, ly=3, length=400, drop=0.0)


def _parity(schedule, B=8, steps=3):
    """f32 fused steps vs OracleTrainer on the same flags; schedule(step) -> trainable predicate of that step"""
    torch.manual_seed(21)
    ref = O.OracleEcgVit(config=_parity_conf())
    ref.train()
    m = E.EcgVit(config=_parity_conf(), compute_dtype=F32)
    m.load_state_dict(ref.state_dict())
    m.cuda().train()
    x, y = O.synthetic_batch(B, length=400, seed=4)
    tr_ref = O.OracleTrainer(ref, n_step=10)
    st = E.HipTrainStep(m, dict(n_step=10), sync_nonfinite=True)
    for it in range(steps):
        freeze(ref, schedule(it))
        freeze(m, schedule(it))
        out = tr_ref.step(x, y)
        loss, _ = st.step(x.cuda(), y.cuda())
        assert abs(float(loss) - float(out.loss)) / float(out.loss) < 1e-4, it
        gn = float(tr_ref.last_grad_norm)
        assert abs(st.grad_norm() - gn) / gn < 1e-4, (it, st.grad_norm(), gn)
    ours = m.state_dict()
    for k, v in ref.state_dict().items():
        assert max_err(ours[k], v) < 3e-6, k
    return tr_ref


@pytest.mark.parametrize('setup', ['linear_probe', 'top1', 'bitfit'])
def test_fused_steps_match_oracle_on_the_same_flags(setup):
    trainable = {'linear_probe': linear_probe, 'top1': top_blocks(1, 3), 'bitfit': bitfit}[setup]
    _parity(lambda it: trainable)


def test_gradual_unfreezing_matches_torch_per_parameter_state():
    """2 steps linear probe, then the top block joins: its AdamW state starts at step 1 while the head goes on at 3 and 4"""
    tr = _parity(lambda it: linear_probe if it < 2 else top_blocks(1, 3), steps=4)
    steps = {int(s['step']) for s in tr.optimizer.state.values()}
    assert steps == {2, 4}


def test_truncated_backward_never_touches_skipped_gradients():
    """NaN in the gradient spans the plan skips: frozen Linear weights of the trainable blocks, everything below the lowest trainable
    block.  The step neither raises nor reads them, and they still hold NaN afterwards."""
    torch.manual_seed(5)
    ly = 4
    m = E.EcgVit(config=_conf(ly=ly), compute_dtype=BF16).cuda().train()
    trainable = lambda n: top_blocks(2, ly)(n) and not n.endswith('0.fn.to_out.0.weight')
    freeze(m, trainable)
    skipped = [n for n in m._param_names
               if (n.endswith('0.fn.to_out.0.weight') or not n.startswith(('vit.transformer.layers.2.', 'vit.transformer.layers.3.', 'vit.mlp_head.')))
               and n != f'vit.transformer.layers.{ly - 3}.1.fn.net.3.bias']   # (a by-product of block 2's fused LayerNorm backward)
    x, y = E.workload.synthetic_batch(24, length=2000, seed=3)
    st = E.HipTrainStep(m, dict(n_step=20, warmup_ratio=0.0), sync_nonfinite=True)
    for it in range(2):
        m._engine()
        for n in skipped:
            m._layout.view(m._gflat, n).fill_(float('nan'))
        st.step(x.cuda(), y.cuda())
        torch.cuda.synchronize()
        assert math.isfinite(st.grad_norm()), it
        for n in skipped:
            assert torch.isnan(m._layout.view(m._gflat, n)).all(), (it, n)
    assert all(torch.isfinite(p).all() for p in m.parameters())


def _buffers(count, seed):
    g = torch.Generator(device='cuda').manual_seed(seed)
    p = torch.randn(count, device='cuda', generator=g)
    gr = torch.randn(count, device='cuda', generator=g) * 1e-2
    mm = torch.randn(count, device='cuda', generator=g) * 1e-3
    v = torch.rand(count, device='cuda', generator=g) * 1e-5
    return p, gr, mm, v


def test_span_kernels_equal_the_whole_buffer_kernels():
    l, st = hip.lib(), hip.stream()
    count = 1 << 20 | 13
    ws = torch.empty(max(l.ecgvit_sumsq_workspace(count), l.ecgvit_sumsq_spans_workspace(1)), dtype=torch.uint8, device='cuda')
    for step in (1, 3, 17):
        a = _buffers(count, step)
        b = [t.clone() for t in a]
        lo_a = torch.zeros(count, dtype=BF16, device='cuda')
        lo_b = lo_a.clone()
        s_a = torch.empty(1, device='cuda')
        s_b = torch.empty(1, device='cuda')
        n_a = torch.empty(2, device='cuda')
        n_b = torch.empty(2, device='cuda')
        spans = torch.tensor([[0, count, 0]], dtype=torch.int64, device='cuda')
        hip.check(l.ecgvit_sumsq(a[1].data_ptr(), count, s_a.data_ptr(), ws.data_ptr(), st), 'sumsq')
        hip.check(l.ecgvit_sumsq_spans(b[1].data_ptr(), spans.data_ptr(), 1, count, s_b.data_ptr(), ws.data_ptr(), st), 'sumsq_spans')
        torch.cuda.synchronize()
        assert abs(float(s_a) - float(s_b)) <= 1e-6 * float(s_a)
        s_b.copy_(s_a)   # the same sumsq in: the updates must agree bit for bit
        args = (s_a, 0.5, 1.0, 3e-4, 0.9, 0.999, 1e-8, 1e-2)
        hip.check(l.ecgvit_adamw_step(a[0].data_ptr(), a[1].data_ptr(), a[2].data_ptr(), a[3].data_ptr(), lo_a.data_ptr(), count,
                                      s_a.data_ptr(), *args[1:], step, 1, n_a.data_ptr(), st), 'adamw_step')
        hip.check(l.ecgvit_adamw_step_spans(b[0].data_ptr(), b[1].data_ptr(), b[2].data_ptr(), b[3].data_ptr(), lo_b.data_ptr(), spans.data_ptr(),
                                            1, count, s_b.data_ptr(), *args[1:], step, 1, n_b.data_ptr(), st), 'adamw_step_spans')
        torch.cuda.synchronize()
        for x_, y_ in zip(a, b):
            assert torch.equal(x_, y_), step
        assert torch.equal(lo_a, lo_b) and torch.equal(n_a, n_b)


def test_span_kernels_touch_their_spans_only():
    """three spans at three step offsets: elements outside are untouched, each span equals the whole-buffer kernel over its own range
    at its own step, and the norm is that of the spans"""
    l, st = hip.lib(), hip.stream()
    count = 300_000
    rows = [[16, 1000, 0], [4096, 70_001, -1], [200_000, 99_999, -2]]
    step = 3
    p, g, m, v = _buffers(count, 7)
    p0, m0, v0 = p.clone(), m.clone(), v.clone()
    spans = torch.tensor(rows, dtype=torch.int64, device='cuda')
    total = sum(r[1] for r in rows)
    ws = torch.empty(l.ecgvit_sumsq_spans_workspace(3), dtype=torch.uint8, device='cuda')
    s = torch.empty(1, device='cuda')
    n = torch.empty(2, device='cuda')
    hip.check(l.ecgvit_sumsq_spans(g.data_ptr(), spans.data_ptr(), 3, total, s.data_ptr(), ws.data_ptr(), st), 'sumsq_spans')
    ref = sum(float((g[o:o + c].double() ** 2).sum()) for o, c, _ in rows)
    torch.cuda.synchronize()
    assert abs(float(s) - ref) <= 1e-5 * ref
    hip.check(l.ecgvit_adamw_step_spans(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), None, spans.data_ptr(), 3, total, s.data_ptr(),
                                        1.0, 1.0, 3e-4, 0.9, 0.999, 1e-8, 1e-2, step, 1, n.data_ptr(), st), 'adamw_step_spans')
    inside = torch.zeros(count, dtype=torch.bool, device='cuda')
    for o, c, k in rows:
        inside[o:o + c] = True
        pr, mr, vr = p0[o:o + c].clone(), m0[o:o + c].clone(), v0[o:o + c].clone()
        nr = torch.empty(2, device='cuda')
        hip.check(l.ecgvit_adamw_step(pr.data_ptr(), g[o:o + c].data_ptr(), mr.data_ptr(), vr.data_ptr(), None, c, s.data_ptr(), 1.0, 1.0, 3e-4,
                                      0.9, 0.999, 1e-8, 1e-2, step + k, 1, nr.data_ptr(), st), 'adamw_step')
        torch.cuda.synchronize()
        assert torch.equal(p[o:o + c], pr) and torch.equal(m[o:o + c], mr) and torch.equal(v[o:o + c], vr), (o, c, k)
    out = ~inside
    assert torch.equal(p[out], p0[out]) and torch.equal(m[out], m0[out]) and torch.equal(v[out], v0[out])
    assert abs(float(n[0]) - math.sqrt(ref)) <= 1e-5 * math.sqrt(ref) and float(n[1]) == 1.0


def test_autograd_surface_skips_frozen_products():
    """EcgVit.forward + loss.backward with a frozen trunk: frozen .grad stays None, the head's gradients equal the full pass's"""
    torch.manual_seed(5)
    conf = _conf(drop=0.0)
    m = E.EcgVit(config=conf, compute_dtype=BF16).cuda().train()
    x, y = E.workload.synthetic_batch(8, length=2000, seed=3)
    x, y = x.cuda(), y.cuda()
    m(sample_values=x, labels=y).loss.backward()
    full = {n: p.grad.clone() for n, p in m.named_parameters()}
    m.zero_grad(set_to_none=True)
    freeze(m, top_blocks(1, 3))
    m(sample_values=x, labels=y).loss.backward()
    for n, p in m.named_parameters():
        if p.requires_grad:
            assert torch.equal(p.grad, full[n]), n
        else:
            assert p.grad is None, n


@pytest.fixture(scope='module')
def nccl_group():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    os.environ['MASTER_ADDR'], os.environ['MASTER_PORT'] = '127.0.0.1', str(port)
    dist.init_process_group('nccl', rank=0, world_size=1, device_id=torch.device('cuda', 0))
    yield None
    dist.destroy_process_group()


def _ddp_run(steps, **kw):
    torch.manual_seed(5)
    m = E.EcgVit(config=_conf(), compute_dtype=BF16).cuda().train()
    freeze(m, top_blocks(1, 3))
    x, y = E.workload.synthetic_batch(24, length=2000, seed=3)
    x, y = x.cuda(), y.cuda()
    st = E.HipTrainStep(m, dict(n_step=20, warmup_ratio=0.0), **kw)
    torch.manual_seed(99)
    losses = [float(st.step(x, y)[0]) for _ in range(steps)]
    st.finish()
    torch.cuda.synchronize()
    return losses, m._pflat.clone(), st.grad_norm()


def test_rccl_path_with_frozen_layers_equals_plain_step(nccl_group):
    ref_l, ref_p, ref_n = _ddp_run(3)
    for kw in (dict(overlap_allreduce=True), dict(overlap_allreduce=False)):
        l, p, n = _ddp_run(3, single_rank_collectives=True, **kw)
        assert l == ref_l and torch.equal(p, ref_p) and n == ref_n, kw
