"""-m gpu: variable-length records (attention_varlen.hip, `lengths=` / narrower batches through engine, model, train step and evaluator).

Held here: the attnv_* kernels against fp64 record by record at each record's own length (dh 64 and 128, 1 to 2048 tokens), exact zeros in the
padded rows, valid outputs independent of what the padded rows hold, repeated launches bit for bit; their dropout mask equal to the uniform
kernel's on the valid region; the CLS forms against row 0 of the full ones; the f32 masked softmax; and the model against the CPU oracle run
record by record (mixed lengths) or on the same narrower input.
"""
import pytest
import torch

from hiputil import rel_err, max_err, _attn_prob_mult_bf16
from oracle import vit_oracle as O
import ecg_representation_learning_amd as E
from ecg_representation_learning_amd.hip import lib, check, ptr, stream

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16


def _lengths_for(B, N, seed):
    g = torch.Generator().manual_seed(seed)
    nt = torch.randint(1, N + 1, (B,), generator=g)
    nt[0] = 1
    nt[-1] = N
    return nt.to(torch.int32)


def _vfwd(qkv, nt, B, N, h, dh, p=0.0, seed=0):
    out = torch.full((B * N, h * dh), float('nan'), device='cuda', dtype=BF16)
    lse = torch.full((B * h * N,), float('nan'), device='cuda')
    check(lib().ecgvit_attention_varlen_fwd(ptr(qkv), ptr(out), ptr(lse), ptr(nt), B, N, h, dh, dh ** -0.5, p, seed, stream()), 'attention_varlen_fwd')
    return out, lse


def _vbwd(qkv, out, do, lse, nt, B, N, h, dh, p=0.0, seed=0):
    dqkv = torch.full((B * N, 3 * h * dh), float('nan'), device='cuda', dtype=BF16)
    check(lib().ecgvit_attention_varlen_bwd(ptr(qkv), ptr(out), ptr(do), ptr(lse), ptr(dqkv), ptr(nt), B, N, h, dh, dh ** -0.5, p, seed, stream()),
          'attention_varlen_bwd')
    return dqkv


def _ref(qkv, n, h, dh):
    d = h * dh
    q, k, v = (qkv[:, i * d:(i + 1) * d].reshape(n, h, dh).permute(1, 0, 2) for i in range(3))
    s = q @ k.transpose(-1, -2) * dh ** -0.5
    o = (torch.softmax(s, -1) @ v).permute(1, 0, 2).reshape(n, d)
    return o, torch.logsumexp(s, -1)


def _bits(t):
    return t.view(torch.int16) if t.dtype == BF16 else t.view(torch.int32)


@pytest.mark.parametrize('dh', [64, 128])
@pytest.mark.parametrize('N', [41, 251, 501, 1251, 2048])
def test_varlen_attention_vs_fp64_per_record(dh, N):
    B, h = 5, 2
    d = h * dh
    nt = _lengths_for(B, N, N + dh)
    ntd = nt.cuda()
    g = torch.Generator(device='cuda').manual_seed(N * 3 + dh)
    qkv = (torch.randn(B * N, 3 * d, device='cuda', generator=g) * 1.5).to(BF16)
    do = torch.randn(B * N, d, device='cuda', generator=g).to(BF16)
    out, lse = _vfwd(qkv, ntd, B, N, h, dh)
    dqkv = _vbwd(qkv, out, do, lse, ntd, B, N, h, dh)
    o2, l2 = _vfwd(qkv, ntd, B, N, h, dh)
    assert torch.equal(_bits(o2), _bits(out)) and torch.equal(_bits(l2), _bits(lse))
    assert torch.equal(_bits(_vbwd(qkv, out, do, lse, ntd, B, N, h, dh)), _bits(dqkv))
    # padded rows of qkv / dout refilled with other finite values: valid outputs bit-identical
    pad = torch.ones(B, N, dtype=torch.bool)
    for b in range(B):
        pad[b, :int(nt[b])] = False
    pad = pad.view(-1).cuda()
    qkv2, do2 = qkv.clone(), do.clone()
    qkv2[pad] = (torch.randn(int(pad.sum()), 3 * d, device='cuda', generator=g) * 3).to(BF16)
    do2[pad] = torch.randn(int(pad.sum()), d, device='cuda', generator=g).to(BF16)
    o3, l3 = _vfwd(qkv2, ntd, B, N, h, dh)
    assert torch.equal(_bits(o3), _bits(out)) and torch.equal(_bits(l3), _bits(lse))
    assert torch.equal(_bits(_vbwd(qkv2, o3, do2, l3, ntd, B, N, h, dh)), _bits(dqkv))
    for b in range(B):
        n = int(nt[b])
        rows = slice(b * N, b * N + n)
        assert bool((out[b * N + n:(b + 1) * N] == 0).all()) and bool((dqkv[b * N + n:(b + 1) * N] == 0).all())
        qr = qkv[rows].double().requires_grad_(True)
        o_ref, lse_ref = _ref(qr, n, h, dh)
        o_ref.backward(do[rows].double())
        eo, el = rel_err(out[rows], o_ref), max_err(lse.view(B, h, N)[b, :, :n], lse_ref)
        gg, gr = dqkv[rows], qr.grad
        eg = [rel_err(gg[:, i * d:(i + 1) * d], gr[:, i * d:(i + 1) * d]) if float(gr[:, i * d:(i + 1) * d].norm()) > 0
              else max_err(gg[:, i * d:(i + 1) * d], gr[:, i * d:(i + 1) * d]) for i in range(3)]
        print(f'[varlen dh {dh} N={N} n={n}] out rel {eo:.2e}, lse max {el:.2e}, dQ {eg[0]:.2e} dK {eg[1]:.2e} dV {eg[2]:.2e}')
        assert eo < 1e-2 and el < 2e-3 and max(eg) < 2e-2, (n, eo, el, eg)


@pytest.mark.parametrize('dh', [64, 128])
def test_varlen_full_lengths_match_uniform_kernel(dh):
    """dh = 128: the uniform entry points run the same kernel text (uniform form), so forward and backward agree bit for bit; dh = 64: the
    tuned uniform kernels, within bf16 tolerance"""
    B, h, N = 3, 2, 251
    d = h * dh
    g = torch.Generator(device='cuda').manual_seed(11)
    qkv = torch.randn(B * N, 3 * d, device='cuda', generator=g).to(BF16)
    do = torch.randn(B * N, d, device='cuda', generator=g).to(BF16)
    nt = torch.full((B,), N, dtype=torch.int32, device='cuda')
    out, lse = _vfwd(qkv, nt, B, N, h, dh)
    ou = torch.empty_like(out)
    lu = torch.empty_like(lse)
    check(lib().ecgvit_attention_fwd(ptr(qkv), ptr(ou), ptr(lu), B, N, h, dh, dh ** -0.5, 0.0, 0, 1, stream()), 'attention_fwd')
    assert max_err(out, ou) < 2e-2 and max_err(lse, lu) < 1e-3
    dqkv = _vbwd(qkv, out, do, lse, nt, B, N, h, dh)
    du = torch.empty_like(dqkv)
    check(lib().ecgvit_attention_bwd(ptr(qkv), ptr(ou), ptr(do), ptr(lu), ptr(du), B, N, h, dh, dh ** -0.5, 0.0, 0, 1, stream()), 'attention_bwd')
    assert rel_err(dqkv, du) < 2e-2
    if dh == 128:
        assert torch.equal(_bits(out), _bits(ou)) and torch.equal(_bits(lse), _bits(lu))
        assert torch.equal(_bits(dqkv), _bits(du))


@pytest.mark.parametrize('dh', [64, 128])
def test_varlen_dropout_mask_is_the_uniform_kernels_on_the_valid_region(dh):
    """Q = K = 0 (every valid probability 1/n), V one-hot of (key - dh w) over window w: output column j of row q exposes the multiplier of key
    dh w + j; held against the uniform kernel's multipliers for the batch N (`_attn_prob_mult_bf16`)"""
    B, h, N, p, seed = 2, 2, 251, 0.1, 17
    d = h * dh
    nt = torch.tensor([97, 200], dtype=torch.int32)
    want = _attn_prob_mult_bf16(B, h, N, p, seed)
    inv = 256.0 / (256.0 - round(256 * p))
    for w in range((N + dh - 1) // dh):
        qkv = torch.zeros(B, N, 3, h, dh)
        k = torch.arange(dh * w, min(N, dh * w + dh))
        qkv[:, k, 2, :, k - dh * w] = 1.0
        out, _ = _vfwd(qkv.reshape(B * N, 3 * d).to(BF16).cuda(), nt.cuda(), B, N, h, dh, p, seed)
        o = out.float().cpu().view(B, N, h, dh).permute(0, 2, 1, 3)
        for b in range(B):
            n = int(nt[b])
            kk = k[k < n]
            if not len(kk):
                continue
            got = o[b, :, :n, :len(kk)] * n
            assert bool(((got == 0) | ((got - inv).abs() < 2e-2 * inv)).all())
            assert torch.equal((got != 0).float() * inv, want[b, :, :n, kk])


@pytest.mark.parametrize('dh', [64, 128])
@pytest.mark.parametrize('N,p', [(41, 0.0), (251, 0.1), (1251, 0.0), (2048, 0.1)])
def test_varlen_cls_kernels_match_row0_of_full_kernels(dh, N, p):
    B, h = 4, 2
    d = h * dh
    nt = _lengths_for(B, N, 7 * N).cuda()
    g = torch.Generator(device='cuda').manual_seed(N)
    qkv = torch.randn(B * N, 3 * d, device='cuda', generator=g).to(BF16)
    out, lse = _vfwd(qkv, nt, B, N, h, dh, p, 5)
    oc = torch.empty(B, d, device='cuda', dtype=BF16)
    lc = torch.empty(B * h, device='cuda')
    check(lib().ecgvit_attention_varlen_cls_fwd(ptr(qkv), ptr(oc), ptr(lc), ptr(nt), B, N, h, dh, dh ** -0.5, p, 5, stream()), 'cls_fwd')
    assert max_err(oc, out.view(B, N, d)[:, 0]) < 2e-2 and max_err(lc, lse.view(B, h, N)[:, :, 0].reshape(-1)) < 1e-3
    doc = torch.randn(B, d, device='cuda', generator=g).to(BF16)
    do = torch.zeros(B, N, d, device='cuda', dtype=BF16)
    do[:, 0] = doc
    dfull = _vbwd(qkv, out, do.view(B * N, d), lse, nt, B, N, h, dh, p, 5)
    dq = torch.empty(B, d, device='cuda', dtype=BF16)
    dcls = torch.full((B * N, 3 * d), float('nan'), device='cuda', dtype=BF16)
    check(lib().ecgvit_attention_varlen_cls_bwd(ptr(qkv), ptr(oc), ptr(doc), ptr(lc), ptr(dcls), ptr(dq), ptr(nt), B, N, h, dh, dh ** -0.5, p, 5,
                                                stream()), 'cls_bwd')
    assert rel_err(dcls[:, d:], dfull[:, d:]) < 2e-2 and rel_err(dq, dfull.view(B, N, 3 * d)[:, 0, :d]) < 2e-2
    for b in range(B):
        n = int(nt[b])
        assert bool((dcls[b * N + n:(b + 1) * N, d:] == 0).all())


def test_f32_masked_softmax_vs_torch():
    B, h, N = 3, 2, 37
    nt = torch.tensor([1, 20, 37], dtype=torch.int32)
    S = torch.randn(B, h, N, N, device='cuda')
    want = torch.zeros_like(S)
    for b in range(B):
        n = int(nt[b])
        want[b, :, :n, :n] = torch.softmax(S[b, :, :n, :n], -1)
    check(lib().ecgvit_softmax_rows_varlen(ptr(S), ptr(nt.cuda()), B, h, N, N, stream()), 'softmax_rows_varlen')
    assert max_err(S, want) < 1e-6
    for b in range(B):
        n = int(nt[b])
        assert bool((S[b, :, n:] == 0).all()) and bool((S[b, :, :, n:] == 0).all())


# ------------------------------------------------------------------------------------------------ model level
def _conf(d, h, L, P=4, layers=2, drop=0.0):
    return E.EcgVitConfig(max_signal_length=L, patch_size=P, hidden_size=d, num_hidden_layers=layers, num_attention_heads=h, intermediate_size=2 * d,
                          hidden_dropout_prob=drop, attention_probs_dropout_prob=drop)


def _pair(conf, dtype, K=7, seed=3, reduction='mean', weight=None):
    torch.manual_seed(seed)
    ref = O.OracleEcgVit(num_class=K, config=conf, loss_reduction=reduction)
    ref.loss_weight = weight
    m = E.EcgVit(num_class=K, config=conf, loss_reduction=reduction, compute_dtype=dtype)
    m.load_state_dict(ref.state_dict())
    m.loss_weight = weight
    m.cuda().train()
    ref.train()
    return ref, m


def _grads(m):
    return {k: p.grad.detach().cpu().clone() for k, p in m.named_parameters() if p.grad is not None}


def _oracle_per_record(ref, x, y, lengths, reduction):
    """record-by-record oracle at each record's own length: logits, loss (mean: sum of per-record BCE terms / (B K)), gradients"""
    B, K = y.shape
    ref.zero_grad()
    logits, terms = [], []
    for b in range(B):
        ref.loss_reduction = 'none'
        o = ref(sample_values=x[b:b + 1, :, :int(lengths[b])], labels=y[b:b + 1])
        logits.append(o.logits.detach())
        terms.append(o.loss)
    t = torch.cat(terms)
    loss = t.sum() / (B * K) if reduction == 'mean' else t
    (loss if reduction == 'mean' else loss.sum()).backward()
    ref.loss_reduction = reduction
    return torch.cat(logits), loss.detach(), {k: p.grad.detach().clone() for k, p in ref.named_parameters() if p.grad is not None}


def _check(tag, m_logits, m_loss, gm, r_logits, r_loss, gr, tol):
    el = rel_err(m_logits, r_logits)
    ell = rel_err(m_loss, r_loss)
    worst = max(rel_err(gm[k], gr[k]) for k in gr if float(gr[k].norm()) > 0)
    print(f'[{tag}] logits rel {el:.2e}, loss rel {ell:.2e}, worst gradient rel {worst:.2e}')
    assert el < tol[0] and ell < tol[0] and worst < tol[1], (el, ell, worst)
    for k in gr:
        if float(gr[k].norm()) == 0:
            assert float(gm[k].abs().max()) == 0.0, k


TOL = {torch.float32: (1e-4, 1e-4), BF16: (3e-2, 6e-2)}


@pytest.mark.parametrize('dtype', [torch.float32, BF16])
@pytest.mark.parametrize('d,h,N', [(128, 2, 251), (256, 2, 251), (128, 2, 1251), (256, 2, 1251)])
def test_mixed_lengths_vs_oracle_per_record(dtype, d, h, N):
    L = 4 * (N - 1)
    ref, m = _pair(_conf(d, h, L), dtype)
    B = 4
    x, y = O.synthetic_batch(B, length=L, num_class=7, seed=N)
    lengths = torch.tensor([L, 4, L // 2, 4 * 97])
    out = m(sample_values=x.cuda(), labels=y.cuda(), lengths=lengths)
    out.loss.backward()
    r_logits, r_loss, gr = _oracle_per_record(ref, x, y, lengths, 'mean')
    _check(f'mixed {dtype} d={d} h={h} N={N}', out.logits, out.loss, _grads(m), r_logits, r_loss, gr, TOL[dtype])


@pytest.mark.parametrize('dtype', [torch.float32, BF16])
def test_mixed_lengths_reduction_none_and_weighted(dtype):
    L = 1000
    ref, m = _pair(_conf(128, 2, L), dtype, reduction='none', weight=[1.0, 3.0])
    B = 3
    x, y = O.synthetic_batch(B, length=L, num_class=7, seed=9)
    lengths = torch.tensor([400, 1000, 8]).cuda()   # device lengths
    out = m(sample_values=x.cuda(), labels=y.cuda(), lengths=lengths)
    out.loss.sum().backward()
    r_logits, r_loss, gr = _oracle_per_record(ref, x, y, lengths.cpu(), 'none')   # (the oracle applies loss_weight inside its terms)
    _check(f'none + weight {dtype}', out.logits, out.loss, _grads(m), r_logits, r_loss, gr, TOL[dtype])


@pytest.mark.parametrize('dtype', [torch.float32, BF16])
def test_narrower_uniform_batch_vs_oracle_and_pos_rows_zero(dtype):
    L = 1000
    ref, m = _pair(_conf(128, 2, L), dtype)
    x, y = O.synthetic_batch(3, length=L, num_class=7, seed=4)
    m(sample_values=x.cuda(), labels=y.cuda()).loss.backward()   # a full-width pass first: its position rows must not leak
    m.zero_grad(set_to_none=True)
    xs = x[:, :, :600].contiguous()
    out = m(sample_values=xs.cuda(), labels=y.cuda())
    out.loss.backward()
    o_ref = ref(sample_values=xs, labels=y)
    o_ref.loss.backward()
    gr = {k: p.grad.detach().clone() for k, p in ref.named_parameters() if p.grad is not None}
    gm = _grads(m)
    _check(f'narrower {dtype}', out.logits, out.loss, gm, o_ref.logits, o_ref.loss, gr, TOL[dtype])
    pos = gm['vit.pos_embedding'].view(-1, 128)
    assert pos.shape[0] == 251 and bool((pos[151:] == 0).all()) and float(pos[:151].abs().max()) > 0


@pytest.mark.parametrize('dtype', [torch.float32, BF16])
def test_full_lengths_bit_identical_and_nan_past_lengths(dtype):
    L = 1000
    _, m = _pair(_conf(128, 2, L), dtype)
    m.eval()
    x, y = O.synthetic_batch(3, length=L, num_class=7, seed=8)
    x, y = x.cuda(), y.cuda()

    def run(xx, lengths):
        m.zero_grad(set_to_none=True)
        o = m(sample_values=xx, labels=y, lengths=lengths)
        o.loss.backward()
        return o.logits.clone(), o.loss.clone(), torch.cat([p.grad.flatten() for p in m.parameters() if p.grad is not None])

    a = run(x, None)
    b = run(x, torch.full((3,), L))
    assert all(torch.equal(u, v) for u, v in zip(a, b))
    lengths = torch.tensor([L, 400, 4])
    xz, xn = x.clone(), x.clone()
    for i, n in enumerate(lengths.tolist()):
        xz[i, :, n:] = 0.0
        xn[i, :, n:] = float('nan')
    c, dd = run(xz, lengths), run(xn, lengths)
    assert all(torch.equal(u, v) for u, v in zip(c, dd))
    assert all(bool(torch.isfinite(u).all()) for u in c)


def _step_model(conf, ref, dtype):
    m = E.EcgVit(num_class=7, config=conf, compute_dtype=dtype)
    m.load_state_dict(ref.state_dict())
    return m.cuda().train()


@pytest.mark.parametrize('dtype', [torch.float32, BF16])
def test_train_step_with_lengths_matches_module_path_and_oracle(dtype):
    L, B = 1000, 4
    conf = _conf(128, 2, L)
    torch.manual_seed(2)
    ref = O.OracleEcgVit(num_class=7, config=conf)
    x, y = O.synthetic_batch(B, length=L, num_class=7, seed=12)
    lengths = torch.tensor([1000, 200, 604, 4])
    # one step without an update: the step's gradients (bf16: the pruned last block) against the module path's
    m1 = _step_model(conf, ref, dtype)
    step = E.HipTrainStep(m1, dict(n_step=10, learning_rate=0.0, weight_decay=0.0))
    loss1, logits1 = step.step(x.cuda(), y.cuda(), lengths=lengths)
    step.finish()
    g1 = m1._gflat.clone()
    if dtype == BF16:
        assert m1._engine().saved['cls_only_last']
    m2 = _step_model(conf, ref, dtype)
    out = m2(sample_values=x.cuda(), labels=y.cuda(), lengths=lengths)
    out.loss.backward()
    g2 = m2._gflat.clone()
    tol = 1e-5 if dtype == torch.float32 else 5e-3
    l1, l2 = float(loss1), float(out.loss.detach())
    print(f'[step vs module {dtype}] loss {abs(l1 - l2):.2e}, gradient rel {rel_err(g1, g2):.2e}')
    assert abs(l1 - l2) <= tol * abs(l2) and max_err(logits1, out.logits) < 10 * tol
    assert rel_err(g1, g2) < (1e-5 if dtype == torch.float32 else 2e-2)
    # three AdamW steps against the oracle's (record-by-record gradients)
    m3 = _step_model(conf, ref, dtype)
    step = E.HipTrainStep(m3, dict(n_step=10, learning_rate=1e-3, weight_decay=1e-2, schedule='constant', warmup_ratio=0.0))
    opt = torch.optim.AdamW(ref.parameters(), lr=1e-3, weight_decay=1e-2)
    for _ in range(3):
        step.step(x.cuda(), y.cuda(), lengths=lengths)
        _oracle_per_record(ref, x, y, lengths, 'mean')
        torch.nn.utils.clip_grad_norm_(ref.parameters(), 1.0)
        opt.step()
    step.finish()
    pm = dict(m3.named_parameters())
    worst = max(rel_err(pm[k].detach(), p.detach()) for k, p in ref.named_parameters())
    print(f'[3 AdamW steps with lengths {dtype}] worst parameter rel {worst:.2e}')
    assert worst < (1e-4 if dtype == torch.float32 else 2e-2), worst


def test_evaluator_with_lengths_matches_per_batch_calls():
    L = 1000
    _, m = _pair(_conf(128, 2, L), BF16)
    x, y = O.synthetic_batch(10, length=L, num_class=7, seed=21)
    x, y = x.cuda(), y.cuda()
    lengths = torch.tensor([1000, 400, 8, 1000, 996, 4, 600, 1000, 12, 300])
    ev = E.HipEvaluator(m, eval_batch_size=4)
    res = ev.evaluate(x, y, return_predictions=True, lengths=lengths)
    m.eval()
    with torch.no_grad():
        want = torch.cat([m(sample_values=x[s:s + 4], labels=y[s:s + 4], lengths=lengths[s:s + 4]).logits for s in range(0, 10, 4)])
    assert torch.equal(res['predictions']['logits'], want)


def test_attention_rollout_of_a_shorter_record():
    L = 1000
    _, m = _pair(_conf(128, 2, L), torch.float32)
    x, _ = O.synthetic_batch(1, length=L, num_class=7, seed=5)
    logits, res = m.attention_rollout(x[0, :, :600].cuda())
    assert res.shape == (2, 150) and bool(torch.isfinite(res).all())
    m(sample_values=x.cuda(), lengths=torch.tensor([400]))
    with pytest.raises(RuntimeError, match='lengths'):
        m.attention_probs(0)
