"""-m gpu: pooled representations -- `ecgvit_pool_records` against fp64 with its derived bound, its layout / batch invariance bit for bit,
`EcgVit.encode` as the classifier's input, its eval semantics, the mean pool against the CPU oracle, records alone / ragged / raw records,
`HipEncoder`, and `HipProbeStep` against the frozen-encoder `HipTrainStep`.

Bounds: 1e-4 (f32 engine) and 2e-2 (bf16 engine) relative L2 are the project's; the kernel's own bound is derived below; the ragged-versus-
`lengths=` bound is the one tests/test_gpu_ragged.py holds ragged-versus-padded logits to (maximum error 2e-2)."""
import pytest
import torch
import torch.nn.functional as F

from hiputil import rel_err, max_err
from oracle import vit_oracle as O
import ecg_representation_learning_amd as E
from ecg_representation_learning_amd import hip
from ecg_representation_learning_amd.hip import lib, check, ptr, stream

pytestmark = pytest.mark.gpu
F32, BF16 = torch.float32, torch.bfloat16
TOL = {F32: 1e-4, BF16: 2e-2}
K, LMAX, PATCH = 7, 600, 20
LENGTHS = [600, 40, 300, 20, 580, 200]


# ------------------------------------------------------------------------------------------------ the kernel
def _pool(x, B, N, d, mode, n_tok=None, tok_off=None, gamma=None, beta=None):
    out = torch.full((B, d), float('nan'), device='cuda')
    check(lib().ecgvit_pool_records(ptr(x), ptr(out), ptr(n_tok), ptr(tok_off), B, N, d, mode, ptr(gamma), ptr(beta), 1e-5, hip.code(x.dtype),
                                    stream()), 'pool_records')
    return out


def _rows(B, N, d, dtype, nt, seed):
    """(padded [B * N, d] with NaN in every row at or past n_tok[b], packed = the valid rows, tok_off) on the device"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, N, d, generator=g).to(dtype)
    for b, n in enumerate(nt):
        x[b, n:] = float('nan')
    packed = torch.cat([x[b, :n] for b, n in enumerate(nt)])
    off = torch.tensor([sum(nt[:b]) for b in range(B)], dtype=torch.int32)
    return x.view(B * N, d).cuda(), packed.cuda(), off.cuda()


def _check_against_fp64(tag, out, rows, nt, mode):
    """rows: per record its valid rows (host).  |out - fp64 mean| <= n * 2^-24 * max|x|: an f32 sum of n terms in any order is within
    (n - 1) u sum|x_i| of the exact sum (u = 2^-24), the division by n adds at most u |mean|, and bf16 -> f32 is exact.  mode 0 reads one row."""
    assert not bool(torch.isnan(out).any()), f'{tag}: a row at or past n_tok was read'
    for b, r in enumerate(rows):
        r = r.double()
        want = r[0] if mode == 0 else r.mean(0)
        n = 1 if mode == 0 else nt[b]
        err, bound = max_err(out[b], want), n * 2.0 ** -24 * float(r.abs().max())
        assert err <= bound, (tag, b, n, err, bound)
        if mode == 0:
            assert torch.equal(out[b].cpu(), r[0].float()), (tag, b)   # exact, f32 and bf16 alike


@pytest.mark.parametrize('d', [72, 768, 2048])
@pytest.mark.parametrize('dtype', [F32, BF16])
def test_pool_records_vs_fp64(d, dtype):
    B, N = 5, 37
    nt = [37, 2, 1, 19, 36]
    padded, packed, off = _rows(B, N, d, dtype, nt, seed=d)
    ntd = torch.tensor(nt, dtype=torch.int32, device='cuda')
    valid = [padded[b * N:b * N + n].cpu() for b, n in enumerate(nt)]
    full = torch.randn(B * N, d, generator=torch.Generator().manual_seed(d + 1)).to(dtype).cuda()
    g = torch.Generator().manual_seed(d + 2)
    gamma, beta = torch.randn(d, generator=g).cuda(), torch.randn(d, generator=g).cuda()
    worst = 0.0
    for mode in (0, 1):
        raw = {}
        for base, (x, o) in dict(padded=(padded, None), packed=(packed, off)).items():
            raw[base] = _pool(x, B, N, d, mode, ntd, o)
            _check_against_fp64(f'{base} mode {mode}', raw[base], valid, nt, mode)
            ln = _pool(x, B, N, d, mode, ntd, o, gamma, beta)
            want = F.layer_norm(raw[base].cpu(), (d,), gamma.cpu(), beta.cpu(), 1e-5)
            worst = max(worst, rel_err(ln, want))
            assert rel_err(ln, want) < 2e-6, (base, mode, rel_err(ln, want))   # tests/test_gpu_ops.py: ecgvit_layernorm_fwd, f32
        out = _pool(full, B, N, d, mode)                                        # n_tok = NULL: every record holds N rows
        _check_against_fp64(f'full mode {mode}', out, [full[b * N:(b + 1) * N].cpu() for b in range(B)], [N] * B, mode)
    print(f'[pool d={d} {dtype}] LayerNorm rel {worst:.2e}')


@pytest.mark.parametrize('dtype', [F32, BF16])
def test_pool_records_long_records(dtype):
    B, N, d = 2, 2049, 768
    nt = [2049, 1000]
    padded, packed, off = _rows(B, N, d, dtype, nt, seed=5)
    ntd = torch.tensor(nt, dtype=torch.int32, device='cuda')
    valid = [padded[b * N:b * N + n].cpu() for b, n in enumerate(nt)]
    a = _pool(padded, B, N, d, 1, ntd)
    _check_against_fp64('long padded', a, valid, nt, 1)
    assert torch.equal(a, _pool(packed, B, N, d, 1, ntd, off))
    full = torch.randn(B * N, d, generator=torch.Generator().manual_seed(6)).to(dtype).cuda()
    _check_against_fp64('long full', _pool(full, B, N, d, 1), [full[:N].cpu(), full[N:].cpu()], [N, N], 1)


@pytest.mark.parametrize('d', [72, 768])
@pytest.mark.parametrize('dtype', [F32, BF16])
def test_pool_records_layout_and_batch_invariance(d, dtype):
    B, N = 5, 37
    nt = [37, 2, 1, 19, 36]
    padded, packed, off = _rows(B, N, d, dtype, nt, seed=100 + d)
    ntd = torch.tensor(nt, dtype=torch.int32, device='cuda')
    g = torch.Generator().manual_seed(d)
    gamma, beta = torch.randn(d, generator=g).cuda(), torch.randn(d, generator=g).cuda()
    for mode in (0, 1):
        for gb in ((None, None), (gamma, beta)):
            a = _pool(padded, B, N, d, mode, ntd, None, *gb)
            assert torch.equal(a, _pool(packed, B, N, d, mode, ntd, off, *gb))     # packed rows == padded rows, bit for bit
            assert torch.equal(a, _pool(padded, B, N, d, mode, ntd, None, *gb))     # two launches
            for b, n in enumerate(nt):                                              # the record alone (B = 1), at another row base
                alone = padded[b * N:b * N + n].clone()
                assert torch.equal(a[b:b + 1], _pool(alone, 1, N, d, mode, ntd[b:b + 1].clone(), None, *gb)), (mode, b)
                assert torch.equal(a[b:b + 1], _pool(alone, 1, n, d, mode, None, None, *gb)), (mode, b)   # n_tok = NULL at N = n


# ------------------------------------------------------------------------------------------------ the model
def _conf(p=0.0):
    return E.EcgVitConfig(max_signal_length=LMAX, patch_size=PATCH, hidden_size=128, num_hidden_layers=2, num_attention_heads=2,
                          intermediate_size=256, hidden_dropout_prob=p, attention_probs_dropout_prob=p)


def _model(dtype, p=0.0, seed=3, state=None):
    torch.manual_seed(seed)
    m = E.EcgVit(num_class=K, config=_conf(p), compute_dtype=dtype)
    if state is not None:
        m.load_state_dict(state)
    return m.cuda().eval()


def _batch(B=6, seed=1, width=LMAX):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, 12, width, generator=g).cuda()


def _ragged(x, lengths):
    return torch.cat([x[b, :, :int(n)] for b, n in enumerate(lengths)], dim=1).contiguous()


@pytest.mark.parametrize('dtype', [F32, BF16])
def test_encode_is_the_classifiers_input(dtype):
    m, x = _model(dtype), _batch()
    with torch.no_grad():
        logits = m(x).logits
    z = m.encode(x)
    assert z.shape == (6, 128) and z.dtype == F32 and z.is_cuda and not z.requires_grad and z.grad_fn is None
    W, b = m.vit.mlp_head[1].weight.detach(), m.vit.mlp_head[1].bias.detach()
    err = rel_err(F.linear(z, W, b), logits)
    print(f'[encode -> logits {dtype}] rel {err:.2e}')
    assert err <= TOL[dtype]
    # norm=False is what the head's LayerNorm reads
    zr = m.encode(x, norm=False)
    ln = m.vit.mlp_head[0]
    assert rel_err(F.layer_norm(zr, (128,), ln.weight.detach(), ln.bias.detach(), 1e-5), z) <= 1e-5
    if dtype == BF16:
        assert m._engine().saved['cls_only_last']             # the pruned last block served pool='cls'
        m.encode(x, pool='mean')
        assert not m._engine().saved['cls_only_last']
    z2 = m.encode(x)
    z2.add_(1.0)                                               # a fresh tensor the caller owns
    assert torch.equal(m.encode(x), z)


def test_encode_overwrites_a_pending_backward():
    m, x = _model(BF16), _batch()
    y = (torch.rand(6, K, generator=torch.Generator().manual_seed(2)) < 0.3).float().cuda()
    out = m(x, labels=y)
    m.encode(x)
    with pytest.raises(RuntimeError, match='later forward overwrote'):
        out.loss.backward()


@pytest.mark.parametrize('dtype', [F32, BF16])
def test_encode_is_an_eval_pass(dtype):
    m, x = _model(dtype, p=0.1), _batch()
    lengths = torch.tensor(LENGTHS)
    for kw in (dict(), dict(pool='mean'), dict(lengths=lengths)):
        m.eval()
        want = m.encode(x, **kw)
        m.train()
        a, b = m.encode(x, **kw), m.encode(x, **kw)
        assert m.training
        assert torch.equal(a, b) and torch.equal(a, want), kw


@pytest.fixture(scope='module')
def oracle():
    torch.manual_seed(11)
    ref = O.OracleEcgVit(num_class=K, config=_conf()).eval()
    x = _batch(seed=4).cpu()
    with torch.no_grad():
        t = ref.vit.trunk(x.unsqueeze(-2))
        ln = ref.vit.mlp_head[0]
        feats = {('mean', False): t.mean(dim=1), ('mean', True): ln(t.mean(dim=1)), ('cls', False): t[:, 0], ('cls', True): ln(t[:, 0])}
    return ref.state_dict(), x, feats


@pytest.mark.parametrize('pool', ['mean', 'cls'])
def test_pools_against_the_oracle(oracle, pool):
    state, x, feats = oracle
    m = _model(F32, state=state)
    for norm in (False, True):
        err = rel_err(m.encode(x.cuda(), pool=pool, norm=norm), feats[(pool, norm)])
        print(f'[oracle pool={pool} norm={norm}] rel {err:.2e}')
        assert err <= 1e-4, (pool, norm, err)


@pytest.mark.parametrize('pool', ['cls', 'mean'])
@pytest.mark.parametrize('dtype', [F32, BF16])
def test_record_alone(dtype, pool):
    m, x = _model(dtype), _batch()
    lengths = torch.tensor(LENGTHS)
    z = m.encode(x, lengths=lengths, pool=pool)
    for b, n in enumerate(LENGTHS):
        alone = m.encode(x[b:b + 1, :, :n].contiguous(), pool=pool)
        err = rel_err(z[b:b + 1], alone)
        print(f'[alone {dtype} {pool} n={n}] rel {err:.2e}')
        assert err <= TOL[dtype], (b, n, err)
    if dtype == BF16:
        zr = m.encode(_ragged(x, LENGTHS), lengths=lengths, pool=pool)
        print(f'[ragged vs lengths {pool}] max {max_err(zr, z):.2e} rel {rel_err(zr, z):.2e}')
        assert zr.shape == z.shape and max_err(zr, z) < 2e-2


@pytest.mark.parametrize('form', ['padded', 'ragged'])
def test_raw_records_draw_no_timeout(form):
    raw = [579, 33, 300, 20, 555, 199]   # padded lengths 580, 40, 320, 40, 560, 200
    x = _batch(width=579)
    lengths = torch.tensor(raw)
    xs = _ragged(x, raw) if form == 'ragged' else x
    g = torch.Generator().manual_seed(9)
    mean, std = torch.randn(12, generator=g).tolist(), (torch.rand(12, generator=g) + 0.5).tolist()
    out = {}
    for timeout in (False, True):
        m = _model(BF16)
        m.set_input_transform(E.FusedInputTransform(mean, std, PATCH, timeout=timeout, per_record=True))
        m.train()
        rng = torch.get_rng_state()
        out[timeout] = m.encode(xs, lengths=lengths)
        assert torch.equal(torch.get_rng_state(), rng) and m.training   # no span was drawn
    assert torch.equal(out[True], out[False]) and bool(torch.isfinite(out[True]).all())


@pytest.mark.parametrize('form,dtype', [('padded', F32), ('padded', BF16), ('ragged', BF16)])
def test_hip_encoder_walks_the_set_in_record_order(form, dtype):
    n = 14
    g = torch.Generator().manual_seed(21)
    x = (0.5 * torch.randn(n, 12, LMAX, generator=g) + 0.3 * torch.arange(n).view(n, 1, 1)).cuda()   # a distinct offset per record
    lens = [PATCH * int(v) for v in torch.randint(1, LMAX // PATCH + 1, (n,), generator=g)]
    lens[0], lens[-1] = LMAX, PATCH
    lengths = torch.tensor(lens)
    xs = _ragged(x, lens) if form == 'ragged' else x
    m = _model(dtype)
    for pool in ('cls', 'mean'):
        whole = m.encode(xs, lengths=lengths, pool=pool)
        got = E.HipEncoder(m, batch_size=4, pool=pool).encode(xs, lengths=lengths)
        assert got.shape == (n, 128) and got.dtype == F32 and got.is_cuda
        err = rel_err(got, whole)
        print(f'[HipEncoder {form} {dtype} {pool}] rel {err:.2e} max {max_err(got, whole):.2e}')
        assert err <= TOL[dtype]
        if form == 'ragged':
            assert max_err(got, whole) < 2e-2
        nearest = torch.cdist(got.double(), whole.double()).argmin(dim=1).cpu()
        assert nearest.tolist() == list(range(n))               # row r is record r: a permutation would show
    if form == 'padded':                                         # without lengths, norm=False, the last chunk short
        got = E.HipEncoder(m, batch_size=4, norm=False).encode(x)
        assert rel_err(got, m.encode(x, norm=False)) <= TOL[dtype]


# ------------------------------------------------------------------------------------------------ the probe step
HEAD = 'vit.mlp_head.'


@pytest.mark.parametrize('dtype', [F32, BF16])
def test_probe_step_is_the_frozen_encoder_step(dtype):
    args = dict(n_step=10, warmup_ratio=0.2, learning_rate=1e-2)
    x = _batch()
    y = (torch.rand(6, K, generator=torch.Generator().manual_seed(8)) < 0.3).float().cuda()
    full = _model(dtype)
    probe = _model(dtype, state=full.state_dict())
    for m in (full, probe):
        m.loss_weight = [1.0, 2.0]
    for n, p in full.named_parameters():
        p.requires_grad_(n.startswith(HEAD))
    full.train()
    st_full, st_probe = E.HipTrainStep(full, args), E.HipProbeStep(probe, args)
    before = probe._pflat.clone()
    feats = probe.encode(x, norm=False)   # once: the cached features
    names = [n for n, _ in probe.named_parameters() if n.startswith(HEAD)]
    assert len(names) == 4

    def head_grad(m):
        return torch.cat([m._engine().G32[n].reshape(-1) for n in names]).double().cpu()
    for i in range(3):
        lf, zf = st_full.step(x, y)
        lp, zp = st_probe.step(feats, y)
        lf, lp = float(lf), float(lp)
        cos = float(F.cosine_similarity(head_grad(full), head_grad(probe), dim=0))
        gn_f, gn_p = st_full.grad_norm(), st_probe.grad_norm()
        print(f'[probe {dtype} step {i}] loss {lf:.6f} / {lp:.6f}, logits rel {rel_err(zp, zf):.2e}, grad cos {cos:.6f}, norm {gn_f:.5f} / {gn_p:.5f}')
        assert st_probe.get_last_lr() == st_full.get_last_lr() and st_probe.step_count == st_full.step_count == i + 1
        assert abs(lp - lf) <= TOL[dtype] * abs(lf)
        if dtype == F32:
            assert rel_err(zp, zf) <= 1e-4 and abs(gn_p - gn_f) <= 1e-4 * gn_f
        else:
            assert cos >= 0.98
    st_full.finish()
    st_probe.finish()
    worst = max(rel_err(dict(probe.named_parameters())[n], dict(full.named_parameters())[n]) for n in names)
    moved = min(rel_err(probe._layout.view(probe._pflat, n), probe._layout.view(before, n)) for n in names)
    print(f'[probe {dtype}] head tensors rel {worst:.2e} (moved by at least {moved:.2e})')
    assert moved > 1e-3                                            # the three steps did train the head
    assert worst <= TOL[dtype]
    lay = probe._layout
    for n, _ in probe.named_parameters():                          # the encoder: bit-identical
        if not n.startswith(HEAD):
            assert torch.equal(lay.view(probe._pflat, n), lay.view(before, n)), n
    with torch.no_grad():                                          # and the model serves the trained head
        assert rel_err(probe(x).logits, full(x).logits) <= TOL[dtype]


@pytest.mark.parametrize('dtype', [F32, BF16])
def test_probe_step_keeps_its_own_count_and_lr(dtype):
    """two consecutive probe steps: the optimiser update it shares with `HipTrainStep` counts the probe's steps and follows its schedule"""
    args = dict(n_step=10, warmup_ratio=0.2, learning_rate=1e-2)
    probe = _model(dtype)
    y = (torch.rand(6, K, generator=torch.Generator().manual_seed(8)) < 0.3).float().cuda()
    feats = probe.encode(_batch(), norm=False)
    st = E.HipProbeStep(probe, args)
    assert st.step_count == 0
    for _ in range(2):
        st.step(feats, y)
    st.finish()
    assert st.step_count == 2
    assert st.get_last_lr() == st.lr0 * st.mult(2) == 1e-2 * E.lr_multiplier('cosine', 2, 10)(2)
