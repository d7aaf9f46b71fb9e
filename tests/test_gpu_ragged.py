"""-m gpu: ragged batches -- records concatenated along time, (C, S) + lengths, every kernel over the packed token rows only.

Held here: the packed attention kernels (attnr_*, the attnv_* bodies on a packed row base) bit for bit against the padded varlen kernels on
the valid rows, dropout included, and against fp64 per record; the packed patch gather and the ragged embedding forward / backward against
restatements (dpos reproducible bit for bit); the model, the fused train step (micro-batches, frozen parameters) and the evaluator on a
ragged batch against the padded `lengths=` path and the CPU oracle record by record; dropout runs reproducible; the activation pool bounded
by the padded pass; and the refusals.
"""
import pytest
import torch

from hiputil import rel_err, max_err
from oracle import vit_oracle as O
import ecg_representation_learning_amd as E
from ecg_representation_learning_amd.hip import lib, check, ptr, stream
from test_gpu_varlen import _conf, _pair, _grads, _oracle_per_record, _check, TOL

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
P4 = 4   # patch size of the gather / embedding cases


def _ntok(B, N, seed):
    g = torch.Generator().manual_seed(seed)
    nt = torch.randint(1, N + 1, (B,), generator=g)
    nt[0] = 1      # a record of one token (its CLS row alone)
    nt[-1] = N     # one of full width
    return nt.to(torch.int32)


def _offsets(nt):
    return (torch.cumsum(nt.long(), 0) - nt.long()).to(torch.int32)


def _pack_rows(t, nt, N):
    """valid rows of a padded [B N, ...] tensor, packed"""
    return torch.cat([t[b * N:b * N + int(n)] for b, n in enumerate(nt.tolist())])


def _close(got, want, rel=2e-2, floor=1e-3):
    """relative error below `rel`, with an absolute floor per element for references that are (near) zero -- e.g. dK of a one-token record"""
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    return float((got - want).norm()) <= rel * float(want.norm()) + floor * want.numel() ** 0.5


def _ragged(x, lengths):
    return torch.cat([x[b, :, :int(n)] for b, n in enumerate(lengths.tolist())], dim=1).contiguous()


# ------------------------------------------------------------------------------------------------ packed attention
@pytest.mark.parametrize('p', [0.0, 0.1])
@pytest.mark.parametrize('dh', [64, 128])
@pytest.mark.parametrize('N', [41, 251, 501, 1251, 2048])
def test_packed_attention_equals_padded_varlen(N, dh, p):
    B, h = 5, 2
    d = h * dh
    sc, seed = dh ** -0.5, 1234 + N
    nt = _ntok(B, N, N + dh)
    ntd, offd = nt.cuda(), _offsets(nt).cuda()
    M = int(nt.sum())
    g = torch.Generator(device='cuda').manual_seed(N * dh)
    qkv = torch.randn(B * N, 3 * d, device='cuda', generator=g).to(BF16)
    do = torch.randn(B * N, d, device='cuda', generator=g).to(BF16)
    # padded reference
    out = torch.empty(B * N, d, device='cuda', dtype=BF16)
    lse = torch.empty(B * h * N, device='cuda')
    check(lib().ecgvit_attention_varlen_fwd(ptr(qkv), ptr(out), ptr(lse), ptr(ntd), B, N, h, dh, sc, p, seed, stream()), 'varlen_fwd')
    dqkv = torch.empty(B * N, 3 * d, device='cuda', dtype=BF16)
    check(lib().ecgvit_attention_varlen_bwd(ptr(qkv), ptr(out), ptr(do), ptr(lse), ptr(dqkv), ptr(ntd), B, N, h, dh, sc, p, seed, stream()),
          'varlen_bwd')
    # packed
    pq, pdo = _pack_rows(qkv, nt, N).contiguous(), _pack_rows(do, nt, N).contiguous()
    po = torch.full((M, d), float('nan'), device='cuda', dtype=BF16)
    plse = torch.full((B * h * N,), float('nan'), device='cuda')
    check(lib().ecgvit_attention_ragged_fwd(ptr(pq), ptr(po), ptr(plse), ptr(ntd), ptr(offd), B, N, h, dh, sc, p, seed, stream()), 'ragged_fwd')
    pdq = torch.full((M, 3 * d), float('nan'), device='cuda', dtype=BF16)
    check(lib().ecgvit_attention_ragged_bwd(ptr(pq), ptr(po), ptr(pdo), ptr(plse), ptr(pdq), ptr(ntd), ptr(offd), B, N, h, dh, sc, p, seed,
                                            stream()), 'ragged_bwd')
    torch.cuda.synchronize()
    assert torch.equal(po, _pack_rows(out, nt, N))
    assert torch.equal(pdq, _pack_rows(dqkv, nt, N))
    valid = torch.cat([torch.arange(bh * N, bh * N + int(nt[bh // h])) for bh in range(B * h)]).cuda()
    assert torch.equal(plse[valid], lse[valid])
    # CLS forms
    oc = torch.empty(B, d, device='cuda', dtype=BF16)
    lc = torch.empty(B * h, device='cuda')
    check(lib().ecgvit_attention_varlen_cls_fwd(ptr(qkv), ptr(oc), ptr(lc), ptr(ntd), B, N, h, dh, sc, p, seed, stream()), 'varlen_cls_fwd')
    poc = torch.full((B, d), float('nan'), device='cuda', dtype=BF16)
    plc = torch.full((B * h,), float('nan'), device='cuda')
    check(lib().ecgvit_attention_ragged_cls_fwd(ptr(pq), ptr(poc), ptr(plc), ptr(ntd), ptr(offd), B, N, h, dh, sc, p, seed, stream()), 'ragged_cls_fwd')
    doc = torch.randn(B, d, device='cuda', generator=g).to(BF16)
    dkv = torch.zeros(B * N, 3 * d, device='cuda', dtype=BF16)
    dqc = torch.empty(B, d, device='cuda', dtype=BF16)
    check(lib().ecgvit_attention_varlen_cls_bwd(ptr(qkv), ptr(oc), ptr(doc), ptr(lc), ptr(dkv), ptr(dqc), ptr(ntd), B, N, h, dh, sc, p, seed, stream()),
          'varlen_cls_bwd')
    pdkv = torch.zeros(M, 3 * d, device='cuda', dtype=BF16)
    pdqc = torch.full((B, d), float('nan'), device='cuda', dtype=BF16)
    check(lib().ecgvit_attention_ragged_cls_bwd(ptr(pq), ptr(poc), ptr(doc), ptr(plc), ptr(pdkv), ptr(pdqc), ptr(ntd), ptr(offd), B, N, h, dh, sc, p,
                                                seed, stream()), 'ragged_cls_bwd')
    torch.cuda.synchronize()
    assert torch.equal(poc, oc) and torch.equal(plc, lc)
    assert torch.equal(pdqc, dqc) and torch.equal(pdkv, _pack_rows(dkv, nt, N))
    if p == 0.0 and N <= 501:   # fp64, record by record: out, lse, dQ / dK / dV, and the CLS forms
        offs = _offsets(nt).tolist()
        for b, n in enumerate(nt.tolist()):
            r0 = offs[b]
            q64 = pq[r0:r0 + n].double().cpu().requires_grad_(True)
            q, k, v = (q64[:, i * d:(i + 1) * d].reshape(n, h, dh).permute(1, 0, 2) for i in range(3))
            s = q @ k.transpose(-1, -2) * sc
            o = (torch.softmax(s, -1) @ v).permute(1, 0, 2).reshape(n, d)
            assert max_err(po[r0:r0 + n], o) < 2e-2, (b, n)
            got_lse = torch.stack([plse[(b * h + hd) * N:(b * h + hd) * N + n] for hd in range(h)])
            assert max_err(got_lse, torch.logsumexp(s, -1)) < 1e-3, (b, n)
            g, = torch.autograd.grad(o, q64, pdo[r0:r0 + n].double().cpu(), retain_graph=True)
            for part in range(3):
                cols = slice(part * d, (part + 1) * d)
                assert _close(pdq[r0:r0 + n, cols], g[:, cols]), (b, n, 'qkv'[part])
            assert max_err(poc[b], o[0]) < 2e-2 and max_err(plc[b * h:(b + 1) * h], torch.logsumexp(s, -1)[:, 0]) < 1e-3
            do1 = torch.zeros(n, d, dtype=torch.float64)
            do1[0] = doc[b].double().cpu()
            g1, = torch.autograd.grad(o, q64, do1)
            assert _close(pdqc[b], g1[0, :d]), (b, n, 'cls dq')
            assert _close(pdkv[r0:r0 + n, d:], g1[:, d:]), (b, n, 'cls dkv')


# ------------------------------------------------------------------------------------------------ patch gather and embedding
def test_packed_patch_gather_equals_valid_rows_of_varlen_gather():
    B, C, L = 4, 12, 1000
    lengths = torch.tensor([1000, 4, 400, 596])
    nt = (lengths // P4 + 1).to(torch.int32)
    x = torch.randn(B, C, L, device='cuda')
    n = L // P4
    padded = torch.empty(B * n, C * P4, device='cuda', dtype=BF16)
    check(lib().ecgvit_patch_gather_varlen(ptr(x), ptr(padded), ptr(nt.cuda()), B, C, L, P4, C * P4, E.hip.BF16, stream()), 'patch_gather_varlen')
    xr = _ragged(x, lengths)
    S = xr.shape[1]
    packed = torch.full((S // P4, C * P4), float('nan'), device='cuda', dtype=BF16)
    check(lib().ecgvit_patch_gather(ptr(xr), ptr(packed), 1, C, S, P4, C * P4, E.hip.BF16, stream()), 'patch_gather')
    want = torch.cat([padded[b * n:b * n + int(l) // P4] for b, l in enumerate(lengths.tolist())])
    assert torch.equal(packed, want)


@pytest.mark.parametrize('pe', [0.0, 0.1])
def test_ragged_embedding_forward_backward(pe):
    B, d, Nmax = 5, 128, 251
    nt = _ntok(B, 120, 5)
    off = _offsets(nt)
    ntd, offd = nt.cuda(), off.cuda()
    M, N = int(nt.sum()), int(nt.max())
    g = torch.Generator(device='cuda').manual_seed(11)
    tok = torch.randn(M - B, d, device='cuda', generator=g).to(BF16)
    cls = torch.randn(d, device='cuda', generator=g)
    pos = torch.randn(Nmax, d, device='cuda', generator=g)
    X = torch.full((M, d), float('nan'), device='cuda', dtype=BF16)
    check(lib().ecgvit_embed_finish_ragged(ptr(tok), ptr(cls), ptr(pos), ptr(X), ptr(ntd), ptr(offd), B, N, d, pe, 77, E.hip.BF16, stream()),
          'embed_finish_ragged')
    want = torch.empty(M, d, device='cuda')
    for b, n in enumerate(nt.tolist()):
        r0 = int(off[b])
        want[r0] = cls + pos[0]
        want[r0 + 1:r0 + n] = tok[r0 - b:r0 - b + n - 1].float() + pos[1:n]
    if pe == 0.0:
        assert max_err(X, want.to(BF16)) == 0.0
    else:   # kept elements scaled by 1 / (1 - p'), dropped ones exactly 0
        kept = X != 0
        frac = float(kept.float().mean())
        assert 0.85 < frac < 0.95
        assert rel_err(X[kept].float(), (want[kept] * 256.0 / (256.0 - round(256 * pe))).to(BF16).float()) < 1e-2
    dX = torch.randn(M, d, device='cuda', generator=g).to(BF16)

    def bwd():
        dtok = torch.full((M - B, d), float('nan'), device='cuda', dtype=BF16)
        dcls = torch.full((d,), float('nan'), device='cuda')
        dpos = torch.full((Nmax, d), float('nan'), device='cuda')
        check(lib().ecgvit_embed_bwd_ragged(ptr(dX), ptr(dtok), ptr(dcls), ptr(dpos), ptr(ntd), ptr(offd), B, N, d, pe, 77, E.hip.BF16, stream()),
              'embed_bwd_ragged')
        torch.cuda.synchronize()
        return dtok, dcls, dpos

    dtok, dcls, dpos = bwd()
    dtok2, dcls2, dpos2 = bwd()
    assert torch.equal(dpos[:N], dpos2[:N]) and torch.equal(dcls, dcls2) and torch.equal(dtok, dtok2)   # deterministic, bit for bit
    assert bool(torch.isnan(dpos[N:]).all())   # rows past the widest record are not touched
    if pe == 0.0:
        wpos = torch.zeros(N, d, device='cuda', dtype=torch.float64)
        for b, n in enumerate(nt.tolist()):
            r0 = int(off[b])
            wpos[:n] += dX[r0:r0 + n].double()
            assert torch.equal(dtok[r0 - b:r0 - b + n - 1], dX[r0 + 1:r0 + n])
        assert max_err(dpos[:N], wpos) < 1e-4 and torch.equal(dcls, dpos[0])
    else:   # the backward drops what the forward dropped (the same packed element index)
        Xz = torch.empty(M, d, device='cuda', dtype=BF16)
        ones = torch.ones(M - B, d, device='cuda', dtype=BF16)
        check(lib().ecgvit_embed_finish_ragged(ptr(ones), ptr(torch.zeros(d, device='cuda')), ptr(torch.zeros(Nmax, d, device='cuda')), ptr(Xz),
                                               ptr(ntd), ptr(offd), B, N, d, pe, 77, E.hip.BF16, stream()), 'embed_finish_ragged')
        for b, n in enumerate(nt.tolist()):
            r0 = int(off[b])
            dropped = Xz[r0 + 1:r0 + n] == 0
            assert bool((dtok[r0 - b:r0 - b + n - 1][dropped] == 0).all())


# ------------------------------------------------------------------------------------------------ model level
MIX = torch.tensor([1000, 4, 500, 388])


def test_model_forward_ragged_vs_padded_lengths_and_oracle():
    L = 1000
    ref, m = _pair(_conf(128, 2, L), BF16)
    x, y = O.synthetic_batch(4, length=L, num_class=7, seed=31)
    xr = _ragged(x, MIX).cuda()
    out = m(sample_values=xr, labels=y.cuda(), lengths=MIX)
    out.loss.backward()
    gr_rag = _grads(m)
    assert m._engine().saved['ragged'].M == int(MIX.sum()) // 4 + 4
    m.zero_grad(set_to_none=True)
    pad = m(sample_values=x.cuda(), labels=y.cuda(), lengths=MIX)
    print(f'[ragged vs padded lengths=] logits {max_err(out.logits, pad.logits):.2e}, loss {abs(float(out.loss.detach()) - float(pad.loss.detach())):.2e}')
    assert max_err(out.logits, pad.logits) < 2e-2 and abs(float(out.loss.detach()) - float(pad.loss.detach())) < 2e-3 * abs(float(pad.loss.detach()))
    r_logits, r_loss, gr = _oracle_per_record(ref, x, y, MIX, 'mean')
    _check('ragged vs oracle', out.logits, out.loss, gr_rag, r_logits, r_loss, gr, TOL[BF16])


def test_model_ragged_narrower_than_max_signal_length():
    """every record shorter than max_signal_length: the pass runs at the widest record's N < N_max, and the position-embedding gradient rows
    past it are exactly zero (after a full-width pass wrote them)"""
    L = 1000
    ref, m = _pair(_conf(128, 2, L), BF16)
    x, y = O.synthetic_batch(3, length=L, num_class=7, seed=33)
    m(sample_values=x.cuda(), labels=y.cuda()).loss.backward()   # a full-width pass first: its position rows must not leak
    m.zero_grad(set_to_none=True)
    lengths = torch.tensor([600, 40, 360])   # widest 600 samples: N = 151 of 251
    out = m(sample_values=_ragged(x, lengths).cuda(), labels=y.cuda(), lengths=lengths)
    out.loss.backward()
    assert m._engine().N == 151
    gm = _grads(m)
    r_logits, r_loss, gr = _oracle_per_record(ref, x, y, lengths, 'mean')
    _check('ragged narrower', out.logits, out.loss, gm, r_logits, r_loss, gr, TOL[BF16])
    pos = gm['vit.pos_embedding'].view(-1, 128)
    assert pos.shape[0] == 251 and bool((pos[151:] == 0).all()) and float(pos[:151].abs().max()) > 0
    m.zero_grad(set_to_none=True)
    xs = x[:, :, :600].contiguous().cuda()   # the padded lengths= pass over the same records at width 600
    pad = m(sample_values=xs, labels=y.cuda(), lengths=lengths)
    pad.loss.backward()
    gp = _grads(m)
    print(f'[ragged narrower vs padded lengths=] logits {max_err(out.logits, pad.logits):.2e}, '
          f'pos grad {rel_err(gm["vit.pos_embedding"], gp["vit.pos_embedding"]):.2e}')
    assert max_err(out.logits, pad.logits) < 2e-2
    assert abs(float(out.loss.detach()) - float(pad.loss.detach())) < 2e-3 * abs(float(pad.loss.detach()))
    assert rel_err(gm['vit.pos_embedding'], gp['vit.pos_embedding']) < 2e-2


@pytest.mark.parametrize('N', [251, 1251])
def test_model_ragged_mixed_lengths_vs_oracle_per_record(N):
    L = 4 * (N - 1)
    ref, m = _pair(_conf(256, 2, L), BF16)
    x, y = O.synthetic_batch(4, length=L, num_class=7, seed=N)
    lengths = torch.tensor([L, 4, L // 2, 4 * 97])
    out = m(sample_values=_ragged(x, lengths).cuda(), labels=y.cuda(), lengths=lengths.cuda())   # device lengths
    out.loss.backward()
    r_logits, r_loss, gr = _oracle_per_record(ref, x, y, lengths, 'mean')
    _check(f'ragged N={N}', out.logits, out.loss, _grads(m), r_logits, r_loss, gr, TOL[BF16])


def test_model_ragged_reduction_none_and_weighted():
    L = 1000
    ref, m = _pair(_conf(128, 2, L), BF16, reduction='none', weight=[1.0, 3.0])
    x, y = O.synthetic_batch(3, length=L, num_class=7, seed=9)
    lengths = torch.tensor([400, 1000, 8])
    out = m(sample_values=_ragged(x, lengths).cuda(), labels=y.cuda(), lengths=lengths)
    out.loss.sum().backward()
    r_logits, r_loss, gr = _oracle_per_record(ref, x, y, lengths, 'none')
    _check('ragged none + weight', out.logits, out.loss, _grads(m), r_logits, r_loss, gr, TOL[BF16])


def _models(conf, n, seed=2):
    torch.manual_seed(seed)
    ref = O.OracleEcgVit(num_class=7, config=conf)
    ms = []
    for _ in range(n):
        m = E.EcgVit(num_class=7, config=conf, compute_dtype=BF16)
        m.load_state_dict(ref.state_dict())
        ms.append(m.cuda().train())
    return ms


ARGS = dict(n_step=10, learning_rate=1e-3, weight_decay=1e-2, schedule='constant', warmup_ratio=0.0)


def test_train_step_ragged_vs_padded_lengths_step():
    L, B = 1000, 6
    conf = _conf(128, 2, L)
    x, y = O.synthetic_batch(B, length=L, num_class=7, seed=12)
    lengths = torch.tensor([1000, 200, 604, 4, 1000, 52])
    xr = _ragged(x, lengths).cuda()
    m_pad, m_rag, m_mb = _models(conf, 3)
    res = {}
    for tag, m, xx, mb in (('pad', m_pad, x.cuda(), None), ('rag', m_rag, xr, None), ('mb', m_mb, xr, 4)):
        step = E.HipTrainStep(m, dict(ARGS))
        loss, logits = step.step(xx, y.cuda(), lengths=lengths, micro_batch_size=mb)
        res[tag] = (float(loss), logits.clone(), step.grad_norm(), m._pflat.clone())
        step.finish()
    for tag in ('rag', 'mb'):
        l, lg, gn, pf = res[tag]
        lp, lgp, gnp, pfp = res['pad']
        print(f'[{tag} vs pad] loss {abs(l - lp):.2e}, logits {max_err(lg, lgp):.2e}, grad norm {abs(gn - gnp) / gnp:.2e}, params {rel_err(pf, pfp):.2e}')
        assert abs(l - lp) <= 5e-3 * abs(lp) and max_err(lg, lgp) < 5e-2
        assert abs(gn - gnp) <= 2e-2 * gnp and rel_err(pf, pfp) < 2e-2
    # micro-batches of a ragged batch against the unsplit ragged step
    l, lg, gn, pf = res['mb']
    lr, lgr, gnr, pfr = res['rag']
    print(f'[mb vs unsplit ragged] logits {max_err(lg, lgr):.2e}, grad norm {abs(gn - gnr) / gnr:.2e}, params {rel_err(pf, pfr):.2e}')
    assert max_err(lg, lgr) < 1e-2 and abs(l - lr) <= 1e-3 * abs(lr) and abs(gn - gnr) <= 1e-2 * gnr and rel_err(pf, pfr) < 1e-2


def test_train_step_ragged_with_frozen_parameters():
    L = 1000
    conf = _conf(128, 2, L)
    x, y = O.synthetic_batch(4, length=L, num_class=7, seed=13)
    lengths = MIX
    m_pad, m_rag = _models(conf, 2)
    trainable = lambda n: n.startswith('vit.mlp_head.') or n.startswith('vit.transformer.layers.1.')
    out = {}
    for tag, m, xx in (('pad', m_pad, x.cuda()), ('rag', m_rag, _ragged(x, lengths).cuda())):
        for n, p in m.named_parameters():
            p.requires_grad_(bool(trainable(n)))
        before = {n: p.detach().clone() for n, p in m.named_parameters()}
        step = E.HipTrainStep(m, dict(ARGS))
        step.step(xx, y.cuda(), lengths=lengths)
        step.step(xx, y.cuda(), lengths=lengths)
        step.finish()
        after = {n: p.detach().clone() for n, p in m.named_parameters()}
        for n in after:
            if not trainable(n):
                assert torch.equal(after[n], before[n]), n   # frozen: bit-identical
        assert any(not torch.equal(after[n], before[n]) for n in after if trainable(n))
        out[tag] = after
    worst = max(rel_err(out['rag'][n], out['pad'][n]) for n in out['pad'])
    assert worst < 2e-2, worst


def test_evaluator_ragged_equals_per_batch_calls():
    L = 1000
    _, m = _pair(_conf(128, 2, L), BF16)
    x, y = O.synthetic_batch(10, length=L, num_class=7, seed=21)
    lengths = torch.tensor([1000, 400, 8, 1000, 996, 4, 600, 1000, 12, 300])
    xr, y = _ragged(x, lengths).cuda(), y.cuda()
    res = E.HipEvaluator(m, eval_batch_size=4).evaluate(xr, y, return_predictions=True, lengths=lengths)
    m.eval()
    offs = [0] + torch.cumsum(lengths, 0).tolist()
    with torch.no_grad():
        want = torch.cat([m(sample_values=xr[:, offs[s]:offs[min(s + 4, 10)]].contiguous(), labels=y[s:s + 4], lengths=lengths[s:s + 4]).logits
                          for s in range(0, 10, 4)])
    assert torch.equal(res['predictions']['logits'], want)


def test_dropout_ragged_steps_reproducible_and_pool_bounded():
    L, B = 1000, 4
    conf = _conf(128, 2, L, drop=0.1)
    x, y = O.synthetic_batch(B, length=L, num_class=7, seed=41)
    m1, m2, m_pad = _models(conf, 3)
    runs = []
    for m in (m1, m2):
        torch.manual_seed(5)
        step = E.HipTrainStep(m, dict(ARGS))
        loss, logits = step.step(_ragged(x, MIX).cuda(), y.cuda(), lengths=MIX)
        step.finish()
        runs.append((loss.clone(), logits.clone(), m._pflat.clone()))
    assert all(torch.equal(a, b) for a, b in zip(*runs))
    assert all(bool(torch.isfinite(t).all()) for t in runs[0])
    # the pool: steps of equal B and different S re-slice the same slabs, never more than a padded full-width step of the same B holds
    step = E.HipTrainStep(m1, dict(ARGS))
    eng = m1._engine()
    slabs = {k: (v.data_ptr(), v.numel()) for k, v in eng._pool.items()}
    for lens in (torch.tensor([4, 8, 12, 16]), torch.tensor([1000, 1000, 1000, 996]), torch.tensor([400, 4, 1000, 60])):
        step.step(_ragged(x, lens).cuda(), y.cuda(), lengths=lens)
        assert {k: (v.data_ptr(), v.numel()) for k, v in eng._pool.items()} == slabs
    step.finish()
    sp = E.HipTrainStep(m_pad, dict(ARGS))
    sp.step(x.cuda(), y.cuda())
    sp.finish()
    pad_pool = m_pad._engine()._pool
    assert all(v.numel() <= pad_pool[k].numel() for k, v in eng._pool.items() if k in pad_pool and not k.startswith('cls_'))


def test_refusals():
    L = 1000
    x, y = O.synthetic_batch(2, length=L, num_class=7, seed=3)
    lengths = torch.tensor([1000, 400])
    xr = _ragged(x, lengths).cuda()
    _, m = _pair(_conf(128, 2, L), BF16)
    m(sample_values=xr, labels=y.cuda(), lengths=lengths)
    with pytest.raises(RuntimeError, match='ragged'):
        m.attention_probs(0)
    with pytest.raises(ValueError, match='needs lengths'):
        m(sample_values=xr, labels=y.cuda())
    with pytest.raises(ValueError, match='sum'):
        m(sample_values=xr, labels=y.cuda(), lengths=torch.tensor([1000, 396]))
    _, m32 = _pair(_conf(128, 2, L), torch.float32)
    with pytest.raises(ValueError, match='bf16'):
        m32(sample_values=xr, labels=y.cuda(), lengths=lengths)
    mm = E.MaskedEcgVit(m).cuda().train()
    with pytest.raises(ValueError, match='ragged'):
        mm(sample_values=xr, mask_idx=mm.random_mask_indices(2))
    with pytest.raises(ValueError, match='ragged'):
        E.HipTrainStep(mm, dict(ARGS)).step_masked(xr, mm.random_mask_indices(2))
    fconf = E.EcgVitConfig(max_signal_length=L, patch_size=4, hidden_size=256, num_hidden_layers=2, num_attention_heads=4, intermediate_size=512,
                           hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    mf = E.EcgVit(num_class=7, config=fconf, compute_dtype=BF16, fp8_linear=True).cuda().train()
    with pytest.raises(ValueError, match='fp8_linear'):
        mf(sample_values=xr, labels=y.cuda(), lengths=lengths)
