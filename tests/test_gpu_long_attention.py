"""-m gpu: the fused bf16 attention for records of 513 to 2048 tokens (dh = 64).

Above 512 tokens the forward runs the streamed persistent kernel with an item per (record, head, 512-query block) -- or, below an item per CU,
the split one-item kernel -- and the backward runs one persistent launch per 256-key window (up to eight), each adding its dQ to the previous
ones' bf16 dQ in `dqkv`.  Held here: outputs, LSE and dQ / dK / dV against fp64; the two forward forms bit for bit; the dropout mask of the
forward and the backward; records past 4 GiB of `qkv`; the 8-bit emitting forward; the CLS-row kernels; and the small model's supervised,
pruned, masked and fp8 steps against the CPU oracle at 1 251 / 1 250 tokens.
"""
import pytest
import torch

import fp8_ref
from hiputil import rel_err, max_err, dev, tools_lib, export_dropout_masks, assert_engine_tensors_carry_masks, _attn_prob_mult_bf16
from oracle import vit_oracle as O
import ecg_representation_learning_amd as E
from ecg_representation_learning_amd import hip
from ecg_representation_learning_amd.hip import lib, check, ptr, stream

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
DH = 64


def _attn_ref(qkv, B, N, h, dh, scale, mask=None):
    d = h * dh
    q, k, v = (qkv[:, i * d:(i + 1) * d].reshape(B, N, h, dh).permute(0, 2, 1, 3) for i in range(3))
    s = q @ k.transpose(-1, -2) * scale
    p = torch.softmax(s, -1)
    lse = torch.logsumexp(s, -1)
    pd = p if mask is None else p * mask
    o = (pd @ v).permute(0, 2, 1, 3).reshape(B * N, d)
    return o, lse, p


def _fwd(fn_lib, qkv, B, N, h, p, seed):
    d = h * DH
    out = torch.full((B * N, d), float('nan'), device='cuda', dtype=BF16)
    lse = torch.full((B * h * N,), float('nan'), device='cuda')
    check(fn_lib.ecgvit_attention_fwd(ptr(qkv), ptr(out), ptr(lse), B, N, h, DH, DH ** -0.5, p, seed, hip.BF16, stream()), 'attention_fwd')
    return out, lse


def _bwd(qkv, out, do, lse, B, N, h, p, seed):
    dqkv = torch.full((B * N, 3 * h * DH), float('nan'), device='cuda', dtype=BF16)
    check(lib().ecgvit_attention_bwd(ptr(qkv), ptr(out), ptr(do), ptr(lse), ptr(dqkv), B, N, h, DH, DH ** -0.5, p, seed, hip.BF16, stream()),
          'attention_bwd')
    return dqkv


def _check_vs_fp64(qkv, do, out, lse, dqkv, B, N, h, recs, mask=None, tag=''):
    """records `recs` of the kernel's results against the fp64 reference on the GPU (mask: [len(recs), h, N, N] multipliers or None)"""
    d = h * DH
    pick = lambda t, w: t.view(B, N, w)[recs].reshape(len(recs) * N, w)
    qr = pick(qkv, 3 * d).double().requires_grad_(True)
    o_ref, lse_ref, _ = _attn_ref(qr, len(recs), N, h, DH, DH ** -0.5, mask=mask)
    o = pick(out, d)
    assert torch.isfinite(o.float()).all()
    eo, mo = rel_err(o, o_ref), max_err(o, o_ref)
    el = max_err(lse.view(B, h, N)[recs], lse_ref)
    o_ref.backward(pick(do, d).double())
    g = pick(dqkv, 3 * d)
    assert torch.isfinite(g.float()).all()
    eg = [rel_err(g[:, i * d:(i + 1) * d], qr.grad[:, i * d:(i + 1) * d]) for i in range(3)]
    print(f'[long attention {tag} N={N} windows={(N + 255) // 256}] out rel {eo:.2e} max {mo:.2e}, lse max {el:.2e}, '
          f'dQ {eg[0]:.2e}, dK {eg[1]:.2e}, dV {eg[2]:.2e}')
    # (test_gpu_ops' bounds, the maximum one bf16 ulp wider: it is taken over up to 6.3 M elements here -- 0.3 M there -- at the same relative error)
    assert mo < 3e-2 and eo < 1e-2, (eo, mo)
    assert el < 2e-3, el
    assert max(eg) < 2e-2, eg
    return eg


# (B, h, N): one item up to more than 2 x 256 CUs' worth; a one-key last window (513, 769, 1025), exact multiples (2048), odd item counts
SHAPES = [(1, 1, 513), (2, 3, 626), (3, 2, 769), (40, 8, 1025), (64, 8, 1251), (5, 4, 2047), (33, 16, 2048), (67, 8, 1251)]


@pytest.mark.parametrize('B,h,N', SHAPES)
def test_long_attention_fwd_bwd_vs_fp64(B, h, N):
    g = torch.Generator(device='cuda').manual_seed(B * 7919 + N)
    d = h * DH
    qkv = (torch.randn(B * N, 3 * d, device='cuda', generator=g) * 1.5).to(BF16)
    do = torch.randn(B * N, d, device='cuda', generator=g).to(BF16)
    out, lse = _fwd(lib(), qkv, B, N, h, 0.0, 0)
    dqkv = _bwd(qkv, out, do, lse, B, N, h, 0.0, 0)
    for _ in range(2):   # repeated launches: bit-identical (a ring or hand-off race would show)
        o2, l2 = _fwd(lib(), qkv, B, N, h, 0.0, 0)
        assert torch.equal(o2.view(torch.int16), out.view(torch.int16)) and torch.equal(l2, lse)
        assert torch.equal(_bwd(qkv, out, do, lse, B, N, h, 0.0, 0).view(torch.int16), dqkv.view(torch.int16))
    recs = sorted({0, B // 2, B - 1})
    _check_vs_fp64(qkv, do, out, lse, dqkv, B, N, h, recs, tag=f'B={B} h={h}')


@pytest.mark.parametrize('B,h,N,p', [(40, 8, 1025, 0.1), (67, 8, 1251, 0.1), (33, 16, 2048, 0.1), (64, 8, 1251, 0.0), (9, 4, 626, 0.1), (130, 2, 700, 0.3)])
def test_long_forward_stream_equals_one_item_kernel(B, h, N, p):
    """the streamed form (item = record, head, 512-query block) against the split one-item kernel (tools variant 0): output, LSE and with them the
    dropout mask BIT-IDENTICAL, the 8-bit emitting entry point too (e4m3 copy, amax)"""
    tl = tools_lib()
    g = torch.Generator(device='cuda').manual_seed(N + B)
    d = h * DH
    qkv = (torch.randn(B * N, 3 * d, device='cuda', generator=g) * 1.3).to(BF16)
    q8s = torch.full((1,), 0.004, device='cuda')
    res = {}
    try:
        for variant in (0, -1):
            tl.ecgvit_tools_attn_fwd_variant(variant)
            out, lse = _fwd(tl, qkv, B, N, h, p, 4321)
            o8 = torch.full((B * N, d), 0x7F, device='cuda', dtype=torch.uint8)
            am = torch.zeros(1, device='cuda')
            out2 = torch.full((B * N, d), float('nan'), device='cuda', dtype=BF16)
            lse2 = torch.full((B * h * N,), float('nan'), device='cuda')
            check(tl.ecgvit_attention_fwd_q8(ptr(qkv), ptr(out2), ptr(lse2), B, N, h, DH, DH ** -0.5, p, 4321, ptr(o8), ptr(q8s), ptr(am), stream()),
                  'attention_fwd_q8')
            torch.cuda.synchronize()
            res[variant] = (out, lse, out2, lse2, o8, am)
    finally:
        tl.ecgvit_tools_attn_fwd_variant(-1)
    a, b = res[0], res[-1]
    assert torch.isfinite(a[0].float()).all()
    for i in (0, 2):
        assert torch.equal(a[i].view(torch.int16), b[i].view(torch.int16)), i
    assert torch.equal(a[1], b[1]) and torch.equal(a[3], b[3])
    assert torch.equal(b[2].view(torch.int16), b[0].view(torch.int16)) and torch.equal(b[3], b[1])
    assert torch.equal(a[4], b[4]) and float(a[5]) == float(b[5]) == float(b[0].float().abs().max())


def test_long_dropout_mask_same_in_forward_and_backward():
    """N = 1251: the mask observed through the forward kernel (one-hot V windows, `_attn_prob_mult_bf16`) at the quantised keep rate, and the
    forward and backward against fp64 under that mask -- once with the one-item forward (B h small) and once with the streamed one"""
    N, p, seed = 1251, 0.1, 31
    for B, h in ((1, 2), (86, 3)):
        mult = _attn_prob_mult_bf16(B, h, N, p, seed)
        keep = float((mult != 0).double().mean())
        want = 1.0 - round(256 * p) / 256.0
        sigma = (want * (1 - want) / mult.numel()) ** 0.5
        print(f'[long mask B={B} h={h}] keep {keep:.5f}, want {want:.5f} (+-{sigma:.1e})')
        assert abs(keep - want) < 6 * sigma + 1e-4, (keep, want)
        g = torch.Generator(device='cuda').manual_seed(5)
        d = h * DH
        qkv = (torch.randn(B * N, 3 * d, device='cuda', generator=g) * 1.2).to(BF16)
        do = torch.randn(B * N, d, device='cuda', generator=g).to(BF16)
        out, lse = _fwd(lib(), qkv, B, N, h, p, seed)
        dqkv = _bwd(qkv, out, do, lse, B, N, h, p, seed)
        recs = [0] if B == 1 else [0, B - 1]
        _check_vs_fp64(qkv, do, out, lse, dqkv, B, N, h, recs, mask=mult[recs].to('cuda', torch.float64), tag=f'dropout {p} B={B} h={h}')


def test_long_records_past_4_gib_of_qkv():
    """p = 0: one record's outputs are bit-identical whether it runs in a batch of 2 or as the last record of a batch whose qkv exceeds 4 GiB
    (per-record 64-bit bases); the backward's dQ / dK / dV of that record too"""
    N, h = 1251, 16
    d = h * DH
    Bbig = (1 << 32) // (N * 3 * d * 2) + 2
    assert Bbig * N * 3 * d * 2 > (1 << 32)
    g = torch.Generator(device='cuda').manual_seed(11)
    small = (torch.randn(2 * N, 3 * d, device='cuda', generator=g)).to(BF16)
    dos = torch.randn(2 * N, d, device='cuda', generator=g).to(BF16)
    o_s, l_s = _fwd(lib(), small, 2, N, h, 0.0, 0)
    g_s = _bwd(small, o_s, dos, l_s, 2, N, h, 0.0, 0)
    big = torch.randn(Bbig * N, 3 * d, device='cuda', generator=g).to(BF16)
    big[(Bbig - 2) * N:] = small
    dob = torch.randn(Bbig * N, d, device='cuda', generator=g).to(BF16)
    dob[(Bbig - 2) * N:] = dos
    o_b, l_b = _fwd(lib(), big, Bbig, N, h, 0.0, 0)
    g_b = _bwd(big, o_b, dob, l_b, Bbig, N, h, 0.0, 0)
    torch.cuda.synchronize()
    assert torch.equal(o_b[(Bbig - 2) * N:].view(torch.int16), o_s.view(torch.int16))
    assert torch.equal(l_b.view(Bbig, h * N)[Bbig - 2:].flatten(), l_s)
    assert torch.equal(g_b[(Bbig - 2) * N:].view(torch.int16), g_s.view(torch.int16))
    del big, dob, o_b, l_b, g_b
    torch.cuda.empty_cache()


def test_long_q8_forward_1251():
    """the 8-bit emitting forward at N = 1251: the e4m3 copy equals quantising the bf16 output as stored; the amax is max |out|"""
    B, h, N = 24, 12, 1251
    d = h * DH
    g = torch.Generator(device='cuda').manual_seed(3)
    qkv = (torch.randn(B * N, 3 * d, device='cuda', generator=g) * 1.3).to(BF16)
    for p in (0.0, 0.1):
        out = torch.empty(B * N, d, device='cuda', dtype=BF16)
        lse = torch.empty(B * h * N, device='cuda')
        o8 = torch.empty(B * N, d, device='cuda', dtype=torch.uint8)
        sc = torch.full((1,), 0.0035, device='cuda')
        am = torch.zeros(1, device='cuda')
        check(lib().ecgvit_attention_fwd_q8(ptr(qkv), ptr(out), ptr(lse), B, N, h, DH, DH ** -0.5, p, 8, ptr(o8), ptr(sc), ptr(am), stream()),
              'attention_fwd_q8')
        assert bool(fp8_ref.accepts(o8, out, sc, fp8_ref.E4M3).all()), (p, fp8_ref.describe_refused(o8, out, sc, fp8_ref.E4M3))
        assert float(am) == float(out.float().abs().max())
        o_plain, l_plain = _fwd(lib(), qkv, B, N, h, p, 8)
        assert torch.equal(o_plain.view(torch.int16), out.view(torch.int16)) and torch.equal(l_plain, lse)
    # the 8-bit backward stays at N <= 512: the caller quantises dqkv itself
    dq8 = torch.empty(B * N, 3 * d, device='cuda', dtype=torch.uint8)
    r = lib().ecgvit_attention_bwd_q8(ptr(qkv), ptr(out), ptr(out), ptr(lse), ptr(torch.empty(B * N, 3 * d, device='cuda', dtype=BF16)), B, N, h, DH,
                                      DH ** -0.5, 0.0, 8, ptr(dq8), ptr(sc), ptr(am), stream())
    assert r == 1   # ECGVIT_EINVAL


@pytest.mark.parametrize('N', [626, 1251, 2048])
@pytest.mark.parametrize('p', [0.0, 0.1])
def test_long_cls_kernels_match_row0_of_full_kernels(N, p):
    B, h = 4, 6
    d = h * DH
    g = torch.Generator(device='cuda').manual_seed(N)
    qkv = (torch.randn(B * N, 3 * d, device='cuda', generator=g) * 0.7).to(BF16)
    out, lse = _fwd(lib(), qkv, B, N, h, p, 77)
    oc = torch.empty(B, d, device='cuda', dtype=BF16)
    lc = torch.empty(B * h, device='cuda')
    check(lib().ecgvit_attention_cls_fwd(ptr(qkv), ptr(oc), ptr(lc), B, N, h, DH, DH ** -0.5, p, 77, hip.BF16, stream()), 'attention_cls_fwd')
    o_ref, l_ref = out.view(B, N, d)[:, 0].float(), lse.view(B * h, N)[:, 0]
    eo, el = rel_err(oc.float(), o_ref), float(((lc - l_ref).abs() / l_ref.abs()).max())
    dO = torch.zeros(B, N, d, device='cuda')
    dO[:, 0] = torch.randn(B, d, device='cuda', generator=g)
    dO = dO.to(BF16).view(B * N, d)
    dqkv = _bwd(qkv, out, dO, lse, B, N, h, p, 77)
    dq2 = torch.full((B * N, 3 * d), float('nan'), device='cuda', dtype=BF16)
    dqc = torch.empty(B, d, device='cuda', dtype=BF16)
    oc0, dOc, lc0 = out.view(B, N, d)[:, 0].contiguous(), dO.view(B, N, d)[:, 0].contiguous(), lse.view(B * h, N)[:, 0].contiguous()
    check(lib().ecgvit_attention_cls_bwd(ptr(qkv), ptr(oc0), ptr(dOc), ptr(lc0), ptr(dq2), ptr(dqc), B, N, h, DH, DH ** -0.5, p, 77, hip.BF16, stream()),
          'attention_cls_bwd')
    full, mine = dqkv.float().view(B, N, 3 * d), dq2.float().view(B, N, 3 * d)
    assert bool(torch.isnan(mine[..., :d]).all())
    ek, ev, eq = rel_err(mine[..., d:2 * d], full[..., d:2 * d]), rel_err(mine[..., 2 * d:], full[..., 2 * d:]), rel_err(dqc.float(), full[:, 0, :d])
    print(f'[long cls N={N} p={p}] fwd rel {eo:.2e}, lse {el:.2e}; bwd dK {ek:.2e}, dV {ev:.2e}, dQ[row 0] {eq:.2e}')
    assert eo < 4e-3 and el <= 1e-6, (eo, el)
    assert ek < 1e-2 and ev < 1e-2 and eq < 1e-2, (ek, ev, eq)


# ---------------------------------------------------------------------------------------------------------------- model level (d 128, h 2, 2 layers)
def _conf(**kw):
    return E.EcgVitConfig(**{**dict(max_signal_length=5000, patch_size=4, hidden_size=128, num_hidden_layers=2, num_attention_heads=2,
                                    intermediate_size=256, hidden_dropout_prob=0.1, attention_probs_dropout_prob=0.1), **kw})


def _cos(a, b):
    a, b = a.double().cpu().flatten(), b.double().cpu().flatten()
    return float((a @ b) / (a.norm() * b.norm() + 1e-30))


def test_long_supervised_step_vs_cpu_oracle_with_injected_masks():
    torch.set_num_threads(min(32, torch.get_num_threads()))
    B = 4
    conf = _conf()
    torch.manual_seed(5)
    ref = O.OracleEcgVit(config=conf).train()
    m = E.EcgVit(config=conf, compute_dtype=BF16)
    m.load_state_dict(ref.state_dict())
    m.cuda().train()
    x, y = O.synthetic_batch(B, length=5000, seed=23)
    out = m(sample_values=x.cuda(), labels=y.cuda())
    eng = m._engine()
    assert eng.N == 1251
    masks = export_dropout_masks(eng)
    assert_engine_tensors_carry_masks(eng, masks)
    out.loss.backward()
    O.inject_dropout(ref.vit, masks)
    o_ref = ref(sample_values=x, labels=y)
    o_ref.loss.backward()
    lerr = abs(float(out.loss.detach()) - float(o_ref.loss.detach())) / float(o_ref.loss.detach())
    pr = dict(ref.named_parameters())
    g16 = torch.cat([p.grad.flatten() for _, p in m.named_parameters()])
    gref = torch.cat([pr[k].grad.flatten() for k, _ in m.named_parameters()])
    worst = min(_cos(p.grad, pr[k].grad) for k, p in m.named_parameters())
    print(f'[long supervised bf16, N=1251, dropout 0.1] loss rel {lerr:.2e}, logits max {max_err(out.logits, o_ref.logits):.2e}, '
          f'gradient cosine {_cos(g16, gref):.5f}, worst tensor {worst:.5f}')
    assert lerr < 2e-3, lerr
    assert max_err(out.logits, o_ref.logits) < 0.05
    assert _cos(g16, gref) > 0.999
    for k, p in m.named_parameters():
        assert _cos(p.grad, pr[k].grad) > 0.99, (k, _cos(p.grad, pr[k].grad))


def test_long_masked_step_vs_cpu_oracle_with_injected_masks():
    torch.set_num_threads(min(32, torch.get_num_threads()))
    B = 4
    conf = _conf()
    n = 5000 // conf.patch_size
    torch.manual_seed(6)
    ref = O.OracleMaskedEcgVit(O.OracleEcgVit(config=conf)).train()
    mm = E.MaskedEcgVit(E.EcgVit(config=conf, compute_dtype=BF16), mask_ratio=0.5)
    mm.load_state_dict(ref.state_dict(), strict=True)
    mm.cuda().train()
    x, _ = O.synthetic_batch(B, length=5000, seed=29)
    idx = mm.random_mask_indices(B, generator=torch.Generator().manual_seed(4))
    enc = mm.encoder
    step = E.HipTrainStep(mm, dict(n_step=10, learning_rate=0.0, weight_decay=0.0))
    loss, pred = step.step_masked(x.cuda(), idx)
    step.finish()
    eng = enc._engine()
    assert eng.T == n == 1250 and eng.saved['masked']
    masks = export_dropout_masks(eng)
    assert_engine_tensors_carry_masks(eng, masks)
    O.inject_dropout(ref.encoder.vit, masks)
    o_ref = ref(x, idx)
    o_ref.loss.backward()
    lerr = abs(float(loss) - float(o_ref.loss.detach())) / float(o_ref.loss.detach())
    names = {'mask_token': 'pretrain.mask_token', 'to_pixels.weight': 'pretrain.to_pixels.weight', 'to_pixels.bias': 'pretrain.to_pixels.bias'}
    got, want = [], []
    for k, q in ref.named_parameters():
        gk = enc._layout.view(enc._gflat, names.get(k, k[len('encoder.'):] if k.startswith('encoder.') else k))
        if q.grad is None:
            assert float(gk.abs().max()) == 0.0, k
            continue
        got.append(gk.flatten())
        want.append(q.grad.flatten())
        assert _cos(gk, q.grad) > 0.95, (k, _cos(gk, q.grad))
    print(f'[long masked bf16, n=1250, dropout 0.1] loss rel {lerr:.2e}, pred rel {rel_err(pred.float().view(B, n // 2, -1), o_ref.logits):.2e}, '
          f'gradient cosine {_cos(torch.cat(got), torch.cat(want)):.5f}')
    assert lerr < 2e-2, lerr
    assert rel_err(pred.float().view(B, n // 2, -1), o_ref.logits) < 3e-2
    assert _cos(torch.cat(got), torch.cat(want)) > 0.98


def _fused_step(conf, ref, prune, x, y):
    m = E.EcgVit(config=conf, compute_dtype=BF16)
    m.load_state_dict(ref.state_dict())
    m.cuda().train()
    step = E.HipTrainStep(m, dict(n_step=10, learning_rate=0.0, weight_decay=0.0))
    eng = m._engine()
    fwd = eng.forward
    eng.forward = lambda *a_, **k: fwd(*a_, **{**k, 'cls_only_last': prune and k.get('cls_only_last', False)})
    torch.manual_seed(42)
    loss, logits = step.step(x.cuda(), y.cuda())
    step.finish()
    assert eng.saved['cls_only_last'] == prune
    return float(loss), logits.clone(), m._gflat.clone()


def test_long_pruned_fused_step_matches_full_step():
    B = 4
    conf = _conf()
    torch.manual_seed(5)
    ref = O.OracleEcgVit(config=conf).train()
    x, y = O.synthetic_batch(B, length=5000, seed=31)
    l0, lg0, g0 = _fused_step(conf, ref, False, x, y)
    l1, lg1, g1 = _fused_step(conf, ref, True, x, y)
    lrel = abs(l1 - l0) / abs(l0)
    print(f'[long pruned vs full] loss rel {lrel:.2e}, logits max {max_err(lg1, lg0):.2e}, gradient cosine {_cos(g1, g0):.6f}')
    assert lrel < 2e-3 and max_err(lg1, lg0) < 5e-3 and _cos(g1, g0) > 0.9999


def test_long_fp8_linear_first_and_steady_pass_vs_cpu_oracle():
    torch.set_num_threads(min(32, torch.get_num_threads()))
    # (the large layer shape, d 1024, 16 heads, f 4096, as test_gpu_fp8: the block Linears the 8-bit kernels take)
    conf = _conf(hidden_size=1024, num_attention_heads=16, intermediate_size=4096, hidden_dropout_prob=0., attention_probs_dropout_prob=0.)
    torch.manual_seed(77)
    ref = O.OracleEcgVit(config=conf).train()
    m8 = E.EcgVit(config=conf, compute_dtype=BF16, fp8_linear=True)
    m8.load_state_dict(ref.state_dict())
    m8.cuda().train()
    x, y = O.synthetic_batch(4, length=5000, seed=77)
    o_ref = ref(sample_values=x, labels=y)
    o_ref.loss.backward()
    l = hip.lib()
    fired = {'ecgvit_attention_fwd_q8': 0, 'ecgvit_attention_bwd_q8': 0}
    saved = {k: getattr(l, k) for k in fired}

    def counting(name):
        def wrapped(*a):
            fired[name] += 1
            return saved[name](*a)
        return wrapped

    def hold(o, tag):
        lref = float(o_ref.loss.detach())
        assert abs(float(o.loss.detach()) - lref) / lref < 3e-2, (tag, float(o.loss.detach()), lref)
        assert float((o.logits.detach().cpu() - o_ref.logits.detach()).abs().max()) < 0.2, tag
        gref = torch.cat([p.grad.flatten() for p in ref.parameters()]).double()
        g8 = torch.cat([p.grad.flatten() for p in m8.parameters()]).double().cpu()
        assert torch.isfinite(g8).all(), tag
        cos = float((g8 @ gref) / (g8.norm() * gref.norm()))
        worst = min(_cos(p.grad, q.grad) for p, q in zip(m8.parameters(), ref.parameters()))
        print(f'[long fp8 {tag}] loss rel {abs(float(o.loss.detach()) - lref) / lref:.2e}, gradient cosine {cos:.5f}, worst tensor {worst:.5f}')
        assert cos > 0.97 and worst > 0.90, (tag, cos, worst)
    for k in fired:
        setattr(l, k, counting(k))
    try:
        o8 = m8(sample_values=x.cuda(), labels=y.cuda())
        o8.loss.backward()
        assert len(m8._engine()._f8_seen) == 16
        hold(o8, 'first pass')
        for p in m8.parameters():
            p.grad = None
        o8s = m8(sample_values=x.cuda(), labels=y.cuda())
        o8s.loss.backward()
        torch.cuda.synchronize()
    finally:
        for k, fn in saved.items():
            setattr(l, k, fn)
    assert fired['ecgvit_attention_fwd_q8'] > 0 and fired['ecgvit_attention_bwd_q8'] == 0, fired   # (the 8-bit backward is gated to N <= 512)
    hold(o8s, 'steady state')


def test_long_attention_probs_equal_f32_path():
    conf = _conf(hidden_dropout_prob=0., attention_probs_dropout_prob=0.)
    torch.manual_seed(9)
    ref = O.OracleEcgVit(config=conf).eval()
    x, _ = O.synthetic_batch(2, length=5000, seed=3)
    probs = {}
    for dt in (torch.float32, BF16):
        m = E.EcgVit(config=conf, compute_dtype=dt)
        m.load_state_dict(ref.state_dict())
        m.cuda().eval()
        with torch.no_grad():
            m(sample_values=x.cuda())
        probs[dt] = [m._engine().attention_probs(i).float().cpu() for i in range(2)]
    for i in range(2):
        a, b = probs[BF16][i], probs[torch.float32][i]
        assert a.shape == (2, 2, 1251, 1251)
        assert torch.allclose(a.sum(-1), torch.ones(2, 2, 1251), atol=2e-2)
        print(f'[long attention_probs layer {i}] rel {rel_err(a, b):.2e}, max {max_err(a, b):.2e}')
        assert rel_err(a, b) < 3e-2 and max_err(a, b) < 2e-2
