"""-m gpu: gradient accumulation over micro-batches in the fused train step (HipTrainStep.step / step_masked(..., micro_batch_size=)).

One optimiser step over ceil(B/m) forward + backward passes equals the unsplit step up to f32 summation order (dropout 0): the folded
gradient buffer, the loss, the clip norm and the logits, on the f32 and bf16 engines, with frozen parameters, per-record lengths, loss
weights, the masked objective, fp8_linear and the RCCL exchange.  micro_batch_size >= B is the unsplit path itself.  The engine's pool holds
the activations of m records; the exchange issues as many all-reduces per optimiser step as without micro-batches; a NaN in a later
micro-batch reaches the non-finite check.  Each test prints what it observed."""
import math
import os
import socket

import pytest
import torch
import torch.distributed as dist

from hiputil import max_err, rel_err
from oracle import vit_oracle as O
import ecg_representation_learning_amd as E
from ecg_representation_learning_amd import hip

pytestmark = pytest.mark.gpu
F32, BF16 = torch.float32, torch.bfloat16


def _conf(d=256, h=4, f=512, ly=3, length=2000, drop=0.0):
    return E.EcgVitConfig(max_signal_length=length, patch_size=20, hidden_size=d, num_hidden_layers=ly, num_attention_heads=h,
                          intermediate_size=f, hidden_dropout_prob=drop, attention_probs_dropout_prob=drop)


F32_CONF = dict(d=64, h=2, f=128, ly=3, length=400)


def freeze(model, trainable):
    for n, p in model.named_parameters():
        p.requires_grad_(bool(trainable(n)))


def linear_probe(n):
    return n.startswith('vit.mlp_head.')


def top2(n):
    return linear_probe(n) or n.startswith(('vit.transformer.layers.1.', 'vit.transformer.layers.2.'))


def _cos(a, b):
    a, b = a.double().flatten(), b.double().flatten()
    return float(a @ b / (a.norm() * b.norm() + 1e-30))


def _mask(model, trainable):
    """boolean mask of the flat buffer over the trainable parameters (None: all)"""
    out = torch.zeros(model._layout.total, dtype=torch.bool, device='cuda')
    for n, (o, _, c) in model._layout.entries.items():
        if trainable is None or trainable(n):
            out[o:o + c] = True
    return out


def _run(conf, dtype, mb, B=24, steps=3, seed=5, trainable=None, lengths=None, loss_weight=None, fp8=False, masked=False, step_kw=None, x=None):
    """`steps` fused steps on a fresh model from the same weights -> per step (loss, logits | pred, trainable gradients, grad norm), params"""
    torch.manual_seed(seed)
    m = E.EcgVit(config=conf, compute_dtype=dtype, fp8_linear=fp8)
    m.loss_weight = loss_weight
    if x is None:
        x, y = E.workload.synthetic_batch(B, length=conf.max_signal_length, seed=3)
    else:
        y = E.workload.synthetic_batch(B, length=conf.max_signal_length, seed=3)[1]
    model = E.MaskedEcgVit(m, mask_ratio=0.5) if masked else m
    model.cuda().train()
    if trainable is not None:
        freeze(m, trainable)
    idx = model.random_mask_indices(B, generator=torch.Generator().manual_seed(8)) if masked else None
    st = E.HipTrainStep(model, dict(n_step=20, warmup_ratio=0.0), sync_nonfinite=True, **(step_kw or {}))
    sel = _mask(m, trainable)
    torch.manual_seed(99)
    out = []
    for _ in range(steps):
        if masked:
            loss, o = st.step_masked(x.cuda(), idx, micro_batch_size=mb)
        else:
            loss, o = st.step(x.cuda(), y.cuda(), lengths=lengths, micro_batch_size=mb)
        out.append((float(loss), o.float().clone(), m._gflat[sel].clone(), st.grad_norm()))
    st.finish()
    torch.cuda.synchronize()
    return out, m._pflat.clone(), m, st


def _compare(ref, got, tag, loss_tol, grad_tol, norm_tol, out_tol):
    """observed worst errors over the steps; asserts the bounds"""
    worst = dict(loss=0.0, grad=0.0, norm=0.0, out=0.0)
    for i, ((l0, o0, g0, n0), (l1, o1, g1, n1)) in enumerate(zip(ref, got)):
        worst['loss'] = max(worst['loss'], abs(l1 - l0) / abs(l0))
        worst['grad'] = max(worst['grad'], rel_err(g1, g0))
        worst['norm'] = max(worst['norm'], abs(n1 - n0) / n0)
        worst['out'] = max(worst['out'], rel_err(o1, o0))
    print(f'{tag}: loss {worst["loss"]:.2e}  grad rel-L2 {worst["grad"]:.2e}  grad_norm {worst["norm"]:.2e}  out rel-L2 {worst["out"]:.2e}')
    assert worst['loss'] <= loss_tol and worst['grad'] <= grad_tol and worst['norm'] <= norm_tol and worst['out'] <= out_tol, (tag, worst)
    return worst


def test_f32_micro_batches_equal_the_plain_step():
    conf = _conf(**F32_CONF)
    ref, p_ref, _, _ = _run(conf, F32, None)
    for mb in (24, 8, 5):
        got, p, _, _ = _run(conf, F32, mb)
        _compare(ref, got, f'f32 mb={mb}', 1e-6, 1e-5, 1e-5, 1e-5)
        print(f'  params rel-L2 {rel_err(p, p_ref):.2e}')


def test_f32_micro_batches_match_the_oracle_on_the_whole_batch():
    """OracleTrainer (torch autograd + clip_grad_norm_ + AdamW) on all 24 records at once vs the fused step at micro_batch_size 5"""
    conf = _conf(**F32_CONF)
    torch.manual_seed(21)
    ref = O.OracleEcgVit(config=conf)
    ref.train()
    m = E.EcgVit(config=conf, compute_dtype=F32)
    m.load_state_dict(ref.state_dict())
    m.cuda().train()
    x, y = O.synthetic_batch(24, length=400, seed=4)
    tr_ref = O.OracleTrainer(ref, n_step=10)
    st = E.HipTrainStep(m, dict(n_step=10), sync_nonfinite=True)
    worst_l = worst_n = 0.0
    for it in range(3):
        out = tr_ref.step(x, y)
        loss, _ = st.step(x.cuda(), y.cuda(), micro_batch_size=5)
        worst_l = max(worst_l, abs(float(loss) - float(out.loss)) / float(out.loss))
        gn = float(tr_ref.last_grad_norm)
        worst_n = max(worst_n, abs(st.grad_norm() - gn) / gn)
    ours = m.state_dict()
    worst_p = max(max_err(ours[k], v) for k, v in ref.state_dict().items())
    print(f'oracle: loss {worst_l:.2e}  grad_norm {worst_n:.2e}  params max-abs {worst_p:.2e}')
    assert worst_l < 1e-4 and worst_n < 1e-4 and worst_p < 3e-6


@pytest.mark.parametrize('h', [4, 2], ids=['dh64', 'dh128'])
def test_bf16_micro_batches_equal_the_plain_step(h):
    conf = _conf(h=h)
    ref, p_ref, m0, _ = _run(conf, BF16, None)
    assert m0._engine().saved['cls_only_last']
    for mb in (8, 5):
        got, p, m1, _ = _run(conf, BF16, mb)
        assert m1._engine().saved['cls_only_last'] and m1._engine().saved['B'] == 24 - (23 // mb) * mb   # the last slice: pruned last block too
        w = _compare(ref, got, f'bf16 dh{256 // h} mb={mb}', 2e-3, 2e-2, 2e-3, 2e-2)
        cos = min(_cos(a[2], b[2]) for a, b in zip(ref, got))
        print(f'  gradient cosine {cos:.6f}  params rel-L2 {rel_err(p, p_ref):.2e}')
        assert cos >= 0.9998 and w['loss'] <= 2e-3


def _plain_path(dtype, masked):
    conf = _conf(**F32_CONF) if dtype == F32 else _conf()
    ref, p_ref, _, st0 = _run(conf, dtype, None, masked=masked)
    assert st0.gacc is None
    for mb in (24, 100):
        got, p, _, st = _run(conf, dtype, mb, masked=masked)
        assert st.gacc is None   # no accumulator: the unsplit path ran
        assert all(a[0] == b[0] and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]) and a[3] == b[3] for a, b in zip(ref, got)), mb
        assert torch.equal(p, p_ref), mb
    print(f'{dtype}{" masked" if masked else ""}: micro_batch_size 24 and 100 bit-identical to None over 3 steps')


@pytest.mark.parametrize('dtype', [F32, BF16])
def test_micro_batch_at_least_the_batch_is_the_plain_path(dtype):
    _plain_path(dtype, masked=False)


@pytest.mark.parametrize('dtype', [F32, BF16])
def test_masked_micro_batch_at_least_the_batch_is_the_plain_path(dtype):
    """the same for `step_masked`: loss, reconstruction, gradients, grad norm and parameters"""
    _plain_path(dtype, masked=True)


@pytest.mark.parametrize('setup', ['linear_probe', 'top2'])
def test_frozen_parameters_with_micro_batches(setup):
    trainable = {'linear_probe': linear_probe, 'top2': top2}[setup]
    conf = _conf(**F32_CONF)
    ref, p_ref, m0, _ = _run(conf, F32, None, trainable=trainable)
    got, p, m1, st = _run(conf, F32, 5, trainable=trainable)
    _compare(ref, got, f'frozen {setup} mb=5', 1e-6, 1e-5, 1e-5, 1e-5)
    torch.manual_seed(5)
    init = E.EcgVit(config=conf, compute_dtype=F32).state_dict()
    ours = m1.state_dict()
    frozen = [n for n in m1._param_names if not trainable(n)]
    assert frozen and all(torch.equal(ours[n].cpu(), init[n]) for n in frozen)
    # the accumulator outside the trainable spans is never touched by a step: fill it with a sentinel and take one more step
    spans = st._spans
    out = torch.ones(m1._layout.total, dtype=torch.bool, device='cuda')
    for o, c, _ in spans[0].tolist():   # (a span also covers the zero padding between consecutive trainable parameters)
        out[o:o + c] = False
    assert not bool((out & _mask(m1, trainable)).any())
    st.gacc.fill_(-7.0)
    x, y = E.workload.synthetic_batch(24, length=400, seed=3)
    st.step(x.cuda(), y.cuda(), micro_batch_size=5)
    torch.cuda.synchronize()
    assert bool((st.gacc[out] == -7.0).all()) and not bool((st.gacc[~out] == -7.0).all())
    # the kernel over the frozen span table, every mode: elements outside the spans keep the sentinel in both buffers
    l, s = hip.lib(), hip.stream()
    g = torch.randn_like(m1._gflat)
    acc = torch.randn_like(m1._gflat)
    g[out], acc[out] = 3.0, -5.0
    g0, acc0 = g.clone(), acc.clone()
    inside = ~out
    for mode in (hip.ACC_INIT, hip.ACC_ADD, hip.ACC_FOLD):
        hip.check(l.ecgvit_grad_accumulate(acc.data_ptr(), g.data_ptr(), spans[0].data_ptr(), spans[1], spans[2], mode, 1.0, s), 'grad_accumulate')
    torch.cuda.synchronize()
    assert bool((g[out] == 3.0).all()) and bool((acc[out] == -5.0).all())
    assert torch.equal(acc[inside], g0[inside] + g0[inside]) and torch.equal(g[inside], g0[inside] + acc[inside])
    print(f'frozen {setup}: {len(frozen)} frozen tensors bit-identical; {int(out.sum())} elements outside the spans untouched')


@pytest.mark.parametrize('dtype', [F32, BF16])
def test_lengths_and_loss_weight_with_micro_batches(dtype):
    conf = _conf(**F32_CONF) if dtype == F32 else _conf()
    L = conf.max_signal_length
    g = torch.Generator().manual_seed(4)
    lengths = (torch.randint(1, L // 20 + 1, (24,), generator=g) * 20)
    lengths[::5] = L
    assert int((lengths < L).sum()) >= 12
    kw = dict(lengths=lengths, loss_weight=[0.3, 2.0])
    ref, _, _, _ = _run(conf, dtype, None, **kw)
    got, _, _, _ = _run(conf, dtype, 7, **kw)
    if dtype == F32:
        _compare(ref, got, 'lengths + loss_weight f32 mb=7', 1e-6, 1e-5, 1e-5, 1e-5)
    else:
        _compare(ref, got, 'lengths + loss_weight bf16 mb=7', 2e-3, 2e-2, 2e-3, 2e-2)
        cos = min(_cos(a[2], b[2]) for a, b in zip(ref, got))
        print(f'  gradient cosine {cos:.6f}')
        assert cos >= 0.9998


@pytest.mark.parametrize('dtype', [F32, BF16])
def test_masked_step_with_micro_batches(dtype):
    conf = _conf(**F32_CONF) if dtype == F32 else _conf()
    ref, _, _, _ = _run(conf, dtype, None, masked=True)
    got, _, _, _ = _run(conf, dtype, 5, masked=True)
    assert got[0][1].shape == ref[0][1].shape
    if dtype == F32:
        _compare(ref, got, 'masked f32 mb=5', 1e-6, 1e-5, 1e-5, 1e-5)
    else:
        _compare(ref, got, 'masked bf16 mb=5', 2e-3, 2e-2, 2e-3, 2e-2)
        cos = min(_cos(a[2], b[2]) for a, b in zip(ref, got))
        print(f'  gradient cosine {cos:.6f}')
        assert cos >= 0.9998


def test_dropout_draws_a_seed_per_micro_batch():
    """the second micro-batch holds the first one's records: with one seed per step they would be dropped alike"""
    conf = _conf(drop=0.1)
    x, _ = E.workload.synthetic_batch(8, length=2000, seed=3)
    x = torch.cat([x, x])
    got, _, _, _ = _run(conf, BF16, 8, B=16, steps=1, x=x)
    logits = got[0][1]
    diff = float((logits[:8] - logits[8:]).abs().max())
    print(f'dropout 0.1: max |logit difference| between the two copies of the same records {diff:.3e}')
    assert diff > 1e-3


@pytest.mark.parametrize('dtype', [F32, BF16])
def test_pool_holds_the_micro_batch_only(dtype):
    conf = _conf(**F32_CONF) if dtype == F32 else _conf()

    def pool_bytes(B, mb):
        _, _, m, st = _run(conf, dtype, mb, B=B, steps=1)
        eng = m._engine()
        assert eng._pool_B == min(B, mb or B)
        return sum(t.numel() * t.element_size() for t in eng._pool.values()), st

    micro, st = pool_bytes(24, 8)
    plain, _ = pool_bytes(8, None)
    whole, _ = pool_bytes(24, None)
    print(f'{dtype}: pool after a B=24, micro_batch_size=8 step {micro} B; plain B=8 step {plain} B; plain B=24 step {whole} B; '
          f'accumulator {st.gacc.numel() * 4} B')
    assert micro == plain and micro < whole


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


def test_rccl_path_with_micro_batches(nccl_group, monkeypatch):
    conf = _conf()
    ref, p_ref, _, _ = _run(conf, BF16, 6)                 # no collectives
    plain, _, _, _ = _run(conf, BF16, None)
    _compare(plain, ref, 'bf16 mb=6 vs unsplit', 2e-3, 2e-2, 2e-3, 2e-2)
    for kw in (dict(overlap_allreduce=True), dict(overlap_allreduce=False)):
        got, p, _, _ = _run(conf, BF16, 6, step_kw=dict(single_rank_collectives=True, **kw))
        assert all(a[0] == b[0] and torch.equal(a[2], b[2]) and a[3] == b[3] for a, b in zip(ref, got)) and torch.equal(p, p_ref), kw
        got, p, _, _ = _run(conf, BF16, 6, step_kw=dict(single_rank_collectives=True, grad_comm_dtype=BF16, **kw))
        w = _compare(ref, got, f'rccl bf16 wire {kw}', 2e-3, 1e-2, 1e-2, 2e-2)
        assert float((p - p_ref).norm() / p_ref.norm()) < 1e-3
    # all-reduces of one optimiser step (after a first step: the frozen-set agreement runs once), with and without 4 micro-batches
    calls = []
    real = dist.all_reduce
    monkeypatch.setattr(dist, 'all_reduce', lambda *a, **k: calls.append(1) or real(*a, **k))
    counts = {}
    for overlap in (True, False):
        for mb in (None, 6):
            torch.manual_seed(5)
            m = E.EcgVit(config=conf, compute_dtype=BF16).cuda().train()
            x, y = E.workload.synthetic_batch(24, length=2000, seed=3)
            st = E.HipTrainStep(m, dict(n_step=20), single_rank_collectives=True, overlap_allreduce=overlap)
            st.step(x.cuda(), y.cuda(), micro_batch_size=mb)
            calls.clear()
            st.step(x.cuda(), y.cuda(), micro_batch_size=mb)
            counts[(overlap, mb)] = len(calls)
    print(f'all-reduce calls per optimiser step (overlap, micro_batch_size): {counts}')
    assert counts[(True, None)] == counts[(True, 6)] > 1 and counts[(False, None)] == counts[(False, 6)] == 1


def test_nan_in_a_later_micro_batch_raises_and_keeps_the_parameters():
    conf = _conf(**F32_CONF)
    torch.manual_seed(5)
    m = E.EcgVit(config=conf, compute_dtype=F32).cuda().train()
    x, y = E.workload.synthetic_batch(24, length=400, seed=3)
    st = E.HipTrainStep(m, dict(n_step=20), sync_nonfinite=True)
    st.step(x.cuda(), y.cuda(), micro_batch_size=8)
    before = m._pflat.clone()
    x[10, 3, 17] = float('nan')   # a record of the second micro-batch
    with pytest.raises(RuntimeError, match='non-finite'):
        st.step(x.cuda(), y.cuda(), micro_batch_size=8)
    torch.cuda.synchronize()
    print(f'NaN in record 10 (micro-batch 2 of 3): RuntimeError raised, parameters bit-identical: {torch.equal(m._pflat, before)}')
    assert torch.equal(m._pflat, before)


def test_fp8_linear_with_micro_batches():
    """B = 20 at 251 tokens: 5020 rows unsplit (8-bit kernels, bf16 copies dropped); micro-batches of 12 and 8 records run 3012 rows (8-bit
    kernels) and 2008 rows (below the 2048-row gate: bf16 kernels)"""
    conf = _conf(d=512, h=8, f=1024, ly=2, length=5000)
    ref, _, m0, _ = _run(conf, BF16, None, B=20, steps=2, fp8=True)
    got, _, m1, _ = _run(conf, BF16, 12, B=20, steps=2, fp8=True)
    assert len(m1._engine()._f8_seen) >= 8   # the 8-bit path ran (the first micro-batch's 3012 rows)
    for (l0, o0, g0, n0), (l1, o1, g1, n1) in zip(ref, got):
        cos = _cos(g0, g1)
        print(f'fp8_linear mb=12: loss {l1:.5f} vs {l0:.5f} (rel {abs(l1 - l0) / l0:.2e}); gradient cosine {cos:.5f}; logits rel-L2 {rel_err(o1, o0):.2e}')
        assert math.isfinite(l1) and abs(l1 - l0) / l0 < 3e-2 and cos > 0.97
