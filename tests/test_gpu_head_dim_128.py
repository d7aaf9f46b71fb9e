"""-m gpu: the fused bf16 attention for 128-wide heads (dh = 128, the uniform form of attn_varlen_kernels.h).

Held here: outputs, LSE and dQ / dK / dV against fp64 at 1 to 2048 tokens, repeated launches bit for bit; the dropout mask of the dh = 128 forward
equal to the dh = 64 kernel's (`hiputil._attn_prob_mult_bf16`) and the forward / backward under it; the CLS-row kernels against row 0 of the full
ones; `ecgvit_attention_probs`; records past 2^31 elements of `qkv`; and the small model's supervised, masked, pruned and fp8 steps against the
CPU oracle.  Bounds are those of tests/test_gpu_long_attention.py.
"""
import pytest
import torch

from hiputil import rel_err, max_err, export_dropout_masks, assert_engine_tensors_carry_masks, _attn_prob_mult_bf16
from oracle import vit_oracle as O
import ecg_representation_learning_amd as E
from ecg_representation_learning_amd import hip
from ecg_representation_learning_amd.hip import lib, check, ptr, stream

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
DH = 128
SCALE = DH ** -0.5


def _attn_ref(qkv, B, N, h, dh, scale, mask=None):
    d = h * dh
    q, k, v = (qkv[:, i * d:(i + 1) * d].reshape(B, N, h, dh).permute(0, 2, 1, 3) for i in range(3))
    s = q @ k.transpose(-1, -2) * scale
    p = torch.softmax(s, -1)
    lse = torch.logsumexp(s, -1)
    pd = p if mask is None else p * mask
    o = (pd @ v).permute(0, 2, 1, 3).reshape(B * N, d)
    return o, lse, p


def _fwd(qkv, B, N, h, p, seed):
    out = torch.full((B * N, h * DH), float('nan'), device='cuda', dtype=BF16)
    lse = torch.full((B * h * N,), float('nan'), device='cuda')
    check(lib().ecgvit_attention_fwd(ptr(qkv), ptr(out), ptr(lse), B, N, h, DH, SCALE, p, seed, hip.BF16, stream()), 'attention_fwd')
    return out, lse


def _bwd(qkv, out, do, lse, B, N, h, p, seed):
    dqkv = torch.full((B * N, 3 * h * DH), float('nan'), device='cuda', dtype=BF16)
    check(lib().ecgvit_attention_bwd(ptr(qkv), ptr(out), ptr(do), ptr(lse), ptr(dqkv), B, N, h, DH, SCALE, p, seed, hip.BF16, stream()), 'attention_bwd')
    return dqkv


def _check_vs_fp64(qkv, do, out, lse, dqkv, B, N, h, recs, mask=None, tag=''):
    d = h * DH
    pick = lambda t, w: t.view(B, N, w)[recs].reshape(len(recs) * N, w)
    qr = pick(qkv, 3 * d).double().requires_grad_(True)
    o_ref, lse_ref, _ = _attn_ref(qr, len(recs), N, h, DH, SCALE, mask=mask)
    o = pick(out, d)
    assert torch.isfinite(o.float()).all()
    eo, mo = rel_err(o, o_ref), max_err(o, o_ref)
    el = max_err(lse.view(B, h, N)[recs], lse_ref)
    o_ref.backward(pick(do, d).double())
    g = pick(dqkv, 3 * d)
    assert torch.isfinite(g.float()).all()
    # (N = 1: softmax over one key, dQ and dK are exactly 0 -- held to an absolute bound there)
    eg = [rel_err(g[:, i * d:(i + 1) * d], qr.grad[:, i * d:(i + 1) * d]) if float(qr.grad[:, i * d:(i + 1) * d].norm()) > 0
          else max_err(g[:, i * d:(i + 1) * d], qr.grad[:, i * d:(i + 1) * d]) for i in range(3)]
    print(f'[dh 128 attention {tag} N={N}] out rel {eo:.2e} max {mo:.2e}, lse max {el:.2e}, dQ {eg[0]:.2e}, dK {eg[1]:.2e}, dV {eg[2]:.2e}')
    assert mo < 3e-2 and eo < 1e-2, (eo, mo)
    assert el < 2e-3, el
    assert max(eg) < 2e-2, eg


# (B, h, N): tile / window / block edges (31, 33, 256, 257, 512, 513, 1025), one-item launches and item counts above the CU count (256)
SHAPES = [(1, 1, 1), (3, 2, 31), (2, 3, 33), (64, 8, 251), (5, 2, 256), (4, 3, 257), (128, 8, 501), (3, 2, 512), (2, 1, 513), (9, 4, 1025),
          (40, 8, 1251), (2, 3, 2047), (17, 8, 2048)]


@pytest.mark.parametrize('B,h,N', SHAPES)
def test_h128_attention_fwd_bwd_vs_fp64(B, h, N):
    g = torch.Generator(device='cuda').manual_seed(B * 7919 + N)
    d = h * DH
    qkv = (torch.randn(B * N, 3 * d, device='cuda', generator=g) * 1.5).to(BF16)
    do = torch.randn(B * N, d, device='cuda', generator=g).to(BF16)
    out, lse = _fwd(qkv, B, N, h, 0.0, 0)
    dqkv = _bwd(qkv, out, do, lse, B, N, h, 0.0, 0)
    o2, l2 = _fwd(qkv, B, N, h, 0.0, 0)   # repeated launches: bit-identical
    assert torch.equal(o2.view(torch.int16), out.view(torch.int16)) and torch.equal(l2, lse)
    assert torch.equal(_bwd(qkv, out, do, lse, B, N, h, 0.0, 0).view(torch.int16), dqkv.view(torch.int16))
    _check_vs_fp64(qkv, do, out, lse, dqkv, B, N, h, sorted({0, B // 2, B - 1}), tag=f'B={B} h={h}')


def _prob_mult_h128(B, h, T, p, seed):
    """the multipliers the dh = 128 forward applies, observed as `_attn_prob_mult_bf16` observes the dh = 64 kernel's: Q = K = 0 (every probability
    1/T), V = one-hot of (key - 128 w) over the keys of window w exposes P~[q, 128 w + j] as output column j.  (B, h, T, T) f32"""
    d = h * DH
    inv = 256.0 / (256.0 - round(256 * p))
    mult = torch.zeros(B, h, T, T)
    for w in range((T + DH - 1) // DH):
        qkv = torch.zeros(B, T, 3, h, DH)
        k = torch.arange(DH * w, min(T, DH * w + DH))
        qkv[:, k, 2, :, k - DH * w] = 1.0
        out, _ = _fwd(qkv.reshape(B * T, 3 * d).to(BF16).cuda(), B, T, h, p, seed)
        o = (out.float().cpu().view(B, T, h, DH).permute(0, 2, 1, 3) * T)[..., :len(k)]
        assert bool(((o == 0) | ((o - inv).abs() < 2e-2 * inv)).all())
        mult[..., DH * w:DH * w + len(k)] = (o != 0).float() * inv
    return mult


@pytest.mark.parametrize('N,p', [(251, 0.1), (1251, 0.3)])
def test_h128_dropout_mask_equals_dh64_kernel_and_fwd_bwd_under_it(N, p):
    B, h, seed = 2, 3, 31
    mult = _prob_mult_h128(B, h, N, p, seed)
    assert torch.equal(mult, _attn_prob_mult_bf16(B, h, N, p, seed))   # the mask does not depend on dh
    g = torch.Generator(device='cuda').manual_seed(5)
    d = h * DH
    qkv = (torch.randn(B * N, 3 * d, device='cuda', generator=g) * 1.2).to(BF16)
    do = torch.randn(B * N, d, device='cuda', generator=g).to(BF16)
    out, lse = _fwd(qkv, B, N, h, p, seed)
    dqkv = _bwd(qkv, out, do, lse, B, N, h, p, seed)
    _check_vs_fp64(qkv, do, out, lse, dqkv, B, N, h, [0, 1], mask=mult.to('cuda', torch.float64), tag=f'dropout {p}')


@pytest.mark.parametrize('N,p', [(1, 0.0), (251, 0.0), (251, 0.1), (1251, 0.1), (2048, 0.0)])
def test_h128_cls_kernels_match_row0_of_full_kernels(N, p):
    B, h = 4, 3
    d = h * DH
    g = torch.Generator(device='cuda').manual_seed(N)
    qkv = (torch.randn(B * N, 3 * d, device='cuda', generator=g) * 0.7).to(BF16)
    out, lse = _fwd(qkv, B, N, h, p, 77)
    oc = torch.empty(B, d, device='cuda', dtype=BF16)
    lc = torch.empty(B * h, device='cuda')
    check(lib().ecgvit_attention_cls_fwd(ptr(qkv), ptr(oc), ptr(lc), B, N, h, DH, SCALE, p, 77, hip.BF16, stream()), 'attention_cls_fwd')
    o_ref, l_ref = out.view(B, N, d)[:, 0].float(), lse.view(B * h, N)[:, 0]
    eo, el = rel_err(oc.float(), o_ref), float(((lc - l_ref).abs() / l_ref.abs().clamp_min(1e-3)).max())
    dO = torch.zeros(B, N, d, device='cuda')
    dO[:, 0] = torch.randn(B, d, device='cuda', generator=g)
    dO = dO.to(BF16).view(B * N, d)
    dqkv = _bwd(qkv, out, dO, lse, B, N, h, p, 77)
    dq2 = torch.full((B * N, 3 * d), float('nan'), device='cuda', dtype=BF16)
    dqc = torch.empty(B, d, device='cuda', dtype=BF16)
    oc0, dOc, lc0 = out.view(B, N, d)[:, 0].contiguous(), dO.view(B, N, d)[:, 0].contiguous(), lse.view(B * h, N)[:, 0].contiguous()
    check(lib().ecgvit_attention_cls_bwd(ptr(qkv), ptr(oc0), ptr(dOc), ptr(lc0), ptr(dq2), ptr(dqc), B, N, h, DH, SCALE, p, 77, hip.BF16, stream()),
          'attention_cls_bwd')
    full, mine = dqkv.float().view(B, N, 3 * d), dq2.float().view(B, N, 3 * d)
    assert bool(torch.isnan(mine[..., :d]).all())
    err = rel_err if N > 1 else max_err   # (N = 1: dK and dQ are exactly 0; the full kernels leave rounding residue there)
    ek, ev, eq = err(mine[..., d:2 * d], full[..., d:2 * d]), rel_err(mine[..., 2 * d:], full[..., 2 * d:]), err(dqc.float(), full[:, 0, :d])
    print(f'[dh 128 cls N={N} p={p}] fwd rel {eo:.2e}, lse {el:.2e}; bwd dK {ek:.2e}, dV {ev:.2e}, dQ[row 0] {eq:.2e}')
    assert eo < 4e-3 and el <= 1e-5, (eo, el)
    assert ek < 1e-2 and ev < 1e-2 and eq < 1e-2, (ek, ev, eq)


@pytest.mark.parametrize('N', [251, 1251])
def test_h128_attention_probs_vs_fp64(N):
    B, h = 2, 2
    d = h * DH
    g = torch.Generator(device='cuda').manual_seed(N)
    qkv = (torch.randn(B * N, 3 * d, device='cuda', generator=g) * 1.5).to(BF16)
    _, lse = _fwd(qkv, B, N, h, 0.0, 0)
    probs = torch.empty(B * h * N * N, device='cuda')
    check(lib().ecgvit_attention_probs(ptr(qkv), ptr(lse), ptr(probs), B, N, h, DH, SCALE, hip.BF16, stream()), 'attention_probs')
    _, _, p_ref = _attn_ref(qkv.double(), B, N, h, DH, SCALE)
    pr = probs.view(B, h, N, N)
    print(f'[dh 128 attention_probs N={N}] rel {rel_err(pr, p_ref):.2e}, max {max_err(pr, p_ref):.2e}')
    assert rel_err(pr, p_ref) < 1e-2 and max_err(pr, p_ref) < 1e-2


def test_h128_qkv_past_2_31_elements():
    """d = 1024 (h 8), N = 2048: qkv of B = 350 records holds 2.2e9 elements; the first and the last record against fp64"""
    N, h, B = 2048, 8, 350
    d = h * DH
    assert B * N * 3 * d > 2 ** 31
    g = torch.Generator(device='cuda').manual_seed(11)
    qkv = torch.randn(B * N, 3 * d, device='cuda', generator=g, dtype=BF16)
    do = torch.randn(B * N, d, device='cuda', generator=g, dtype=BF16)
    out, lse = _fwd(qkv, B, N, h, 0.0, 0)
    dqkv = _bwd(qkv, out, do, lse, B, N, h, 0.0, 0)
    torch.cuda.synchronize()
    for r in (0, B - 1):
        _check_vs_fp64(qkv, do, out, lse, dqkv, B, N, h, [r], tag=f'record {r} of {B}')
    del qkv, do, out, lse, dqkv
    torch.cuda.empty_cache()


# ---------------------------------------------------------------------------------------------------------------- model level (d 256, h 2, 2 layers)
def _conf(L, **kw):
    return E.EcgVitConfig(**{**dict(max_signal_length=L, patch_size=4, hidden_size=256, num_hidden_layers=2, num_attention_heads=2,
                                    intermediate_size=512, hidden_dropout_prob=0.1, attention_probs_dropout_prob=0.1), **kw})


def _cos(a, b):
    a, b = a.double().cpu().flatten(), b.double().cpu().flatten()
    return float((a @ b) / (a.norm() * b.norm() + 1e-30))


@pytest.mark.parametrize('L', [1000, 5000])
@pytest.mark.parametrize('p', [0.0, 0.1])
def test_h128_supervised_step_vs_cpu_oracle(L, p):
    torch.set_num_threads(min(32, torch.get_num_threads()))
    B = 4
    conf = _conf(L, hidden_dropout_prob=p, attention_probs_dropout_prob=p)
    torch.manual_seed(5)
    ref = O.OracleEcgVit(config=conf).train()
    m = E.EcgVit(config=conf, compute_dtype=BF16)
    m.load_state_dict(ref.state_dict())
    m.cuda().train()
    x, y = O.synthetic_batch(B, length=L, seed=23)
    out = m(sample_values=x.cuda(), labels=y.cuda())
    eng = m._engine()
    assert eng.dh == 128 and eng.N == L // 4 + 1
    if p > 0:
        masks = export_dropout_masks(eng)
        assert_engine_tensors_carry_masks(eng, masks)
        O.inject_dropout(ref.vit, masks)
    out.loss.backward()
    o_ref = ref(sample_values=x, labels=y)
    o_ref.loss.backward()
    lerr = abs(float(out.loss.detach()) - float(o_ref.loss.detach())) / float(o_ref.loss.detach())
    pr = dict(ref.named_parameters())
    g16 = torch.cat([q.grad.flatten() for _, q in m.named_parameters()])
    gref = torch.cat([pr[k].grad.flatten() for k, _ in m.named_parameters()])
    worst = min(_cos(q.grad, pr[k].grad) for k, q in m.named_parameters())
    print(f'[dh 128 supervised N={eng.N} dropout {p}] loss rel {lerr:.2e}, logits max {max_err(out.logits, o_ref.logits):.2e}, '
          f'gradient cosine {_cos(g16, gref):.5f}, worst tensor {worst:.5f}')
    assert lerr < 2e-3, lerr
    assert max_err(out.logits, o_ref.logits) < 0.05
    assert _cos(g16, gref) > 0.999
    for k, q in m.named_parameters():
        assert _cos(q.grad, pr[k].grad) > 0.99, (k, _cos(q.grad, pr[k].grad))


@pytest.mark.parametrize('L', [1000, 5000])
@pytest.mark.parametrize('p', [0.0, 0.1])
def test_h128_masked_step_vs_cpu_oracle(L, p):
    torch.set_num_threads(min(32, torch.get_num_threads()))
    B = 4
    conf = _conf(L, hidden_dropout_prob=p, attention_probs_dropout_prob=p)
    n = L // conf.patch_size
    torch.manual_seed(6)
    ref = O.OracleMaskedEcgVit(O.OracleEcgVit(config=conf)).train()
    mm = E.MaskedEcgVit(E.EcgVit(config=conf, compute_dtype=BF16), mask_ratio=0.5)
    mm.load_state_dict(ref.state_dict(), strict=True)
    mm.cuda().train()
    x, _ = O.synthetic_batch(B, length=L, seed=29)
    idx = mm.random_mask_indices(B, generator=torch.Generator().manual_seed(4))
    enc = mm.encoder
    step = E.HipTrainStep(mm, dict(n_step=10, learning_rate=0.0, weight_decay=0.0))
    loss, pred = step.step_masked(x.cuda(), idx)
    step.finish()
    eng = enc._engine()
    assert eng.dh == 128 and eng.T == n and eng.saved['masked']
    if p > 0:
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
        assert _cos(gk, q.grad) > 0.99, (k, _cos(gk, q.grad))
    pe = rel_err(pred.float().view(B, n // 2, -1), o_ref.logits)
    print(f'[dh 128 masked n={n} dropout {p}] loss rel {lerr:.2e}, pred rel {pe:.2e}, gradient cosine {_cos(torch.cat(got), torch.cat(want)):.5f}')
    assert lerr < 2e-3, lerr
    assert pe < 3e-2
    assert _cos(torch.cat(got), torch.cat(want)) > 0.999


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


@pytest.mark.parametrize('L', [1000, 5000])
def test_h128_pruned_fused_step_matches_full_step(L):
    B = 4
    conf = _conf(L)
    torch.manual_seed(5)
    ref = O.OracleEcgVit(config=conf).train()
    x, y = O.synthetic_batch(B, length=L, seed=31)
    l0, lg0, g0 = _fused_step(conf, ref, False, x, y)
    l1, lg1, g1 = _fused_step(conf, ref, True, x, y)
    lrel = abs(l1 - l0) / abs(l0)
    print(f'[dh 128 pruned vs full L={L}] loss rel {lrel:.2e}, logits max {max_err(lg1, lg0):.2e}, gradient cosine {_cos(g1, g0):.6f}')
    assert lrel < 2e-3 and max_err(lg1, lg0) < 5e-3 and _cos(g1, g0) > 0.9999


def test_h128_fp8_linear_first_and_steady_pass_vs_cpu_oracle():
    torch.set_num_threads(min(32, torch.get_num_threads()))
    # d 1024, 8 heads, f 4096, N 501; B 5 -> 2 505 rows: the block Linears run the 8-bit products
    conf = _conf(2000, hidden_size=1024, num_attention_heads=8, intermediate_size=4096, hidden_dropout_prob=0., attention_probs_dropout_prob=0.)
    torch.manual_seed(77)
    ref = O.OracleEcgVit(config=conf).train()
    m8 = E.EcgVit(config=conf, compute_dtype=BF16, fp8_linear=True)
    m8.load_state_dict(ref.state_dict())
    m8.cuda().train()
    x, y = O.synthetic_batch(5, length=2000, seed=77)
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
        print(f'[dh 128 fp8 {tag}] loss rel {abs(float(o.loss.detach()) - lref) / lref:.2e}, gradient cosine {cos:.5f}, worst tensor {worst:.5f}')
        assert cos > 0.97 and worst > 0.90, (tag, cos, worst)
    for k in fired:
        setattr(l, k, counting(k))
    try:
        o8 = m8(sample_values=x.cuda(), labels=y.cuda())
        o8.loss.backward()
        assert m8._engine().dh == 128 and m8._engine().N == 501
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
    assert fired == {'ecgvit_attention_fwd_q8': 0, 'ecgvit_attention_bwd_q8': 0}, fired   # no 8-bit emission at dh = 128
    hold(o8s, 'steady state')


def test_h128_q8_entry_points_still_reject():
    B, N, h = 2, 251, 2
    d = h * DH
    qkv = torch.zeros(B * N, 3 * d, device='cuda', dtype=BF16)
    out = torch.empty(B * N, d, device='cuda', dtype=BF16)
    lse = torch.empty(B * h * N, device='cuda')
    b8 = torch.empty(B * N, 3 * d, device='cuda', dtype=torch.uint8)
    sc, am = torch.ones(1, device='cuda'), torch.zeros(1, device='cuda')
    assert lib().ecgvit_attention_fwd_q8(ptr(qkv), ptr(out), ptr(lse), B, N, h, DH, SCALE, 0.0, 1, ptr(b8), ptr(sc), ptr(am), stream()) == 1
    assert lib().ecgvit_attention_bwd_q8(ptr(qkv), ptr(out), ptr(out), ptr(lse), ptr(qkv), B, N, h, DH, SCALE, 0.0, 1, ptr(b8), ptr(sc), ptr(am),
                                         stream()) == 1
    for dh in (32, 256):   # every other head dim: ECGVIT_EINVAL
        assert lib().ecgvit_attention_fwd(ptr(qkv), ptr(out), ptr(lse), B, N, 2 * DH // dh, dh, dh ** -0.5, 0.0, 1, hip.BF16, stream()) == 1
