"""-m gpu: attention rollout for whole batches -- the `ecgvit_rollout_*` entry points against float64 (padded rows never read, packed / padded /
alone bit-identical), the f32 engine against the oracle's per-record maps, the bf16 engine in every batch form against the closed form on its
own qkv / lse, the memory the batch form takes, and `HipRollout` over a resident set."""
import pytest
import torch

import ecg_representation_learning_amd as E
from ecg_representation_learning_amd import hip
from ecg_representation_learning_amd.hip import lib, check, ptr, stream
from oracle import vit_oracle as O
from hiputil import dev, max_err
from rollout_ref import rollout_reference, rollout_closed_form_qkv, lse_from_qkv, probs_from_qkv

pytestmark = pytest.mark.gpu
BF16, F32 = torch.bfloat16, torch.float32
P, L_MAX, C = 4, 1000, 12
LENGTHS = [1000, 400, 8, 4, 996, 516]        # 251, 101, 3, 2, 250, 130 tokens
RAW = [997, 399, 7, 3, 995, 515]             # raw sample counts that pad to LENGTHS
MEAN = [0.1 * (c - 5) for c in range(C)]
STD = [0.5 + 0.25 * c for c in range(C)]
NAN = float('nan')

# ---- bounds -------------------------------------------------------------------------------------------------------------------------
# C-ABI against float64 on the same bf16 qkv and a float64 lse: a lane adds at most N / 2 = 1024 weighted probabilities one after another in
# f32, worst case N 2^-24 = 1.2e-4 of the sum (the products are exact, the exponent's argument carries ~1e-6); held to 1e-4 of max(1, |r|).
ABI_TOL = 1e-4
# bf16 engine against the closed form on its own qkv / lse (maps in [0, 1]): 4 x the maximum measured over the cases below on the MI355X
# (profiles/r17_rollout.txt (d): 4.83e-7 -> 1.93e-6), rounded up to one digit; never above the worst case 1e-4 of 2049 f32 additions.
BF16_TOL = 2e-6
# bf16 engine against the reference loop on its own exported probabilities: those rows sum to 1 within 1e-3 (tests/test_gpu_model.py), the two
# normalisers of a layer pair are then each within 5e-4 of 2 -> at most 1e-3 of a map entry <= 1 (measured: 5.3e-7, profiles/r17_rollout.txt (d)).
BF16_PROBS_TOL = 1e-3


# =====================================================================================================================================
# 1. C-ABI, bf16, synthetic
# =====================================================================================================================================
def _abi_case(dh, h, N, n_tok, seed):
    """random bf16 qkv (padded rows NaN), lse in float64 from the same bf16 values (padded rows NaN), non-negative w (NaN past n), and the
    float64 c / r per record"""
    g = torch.Generator().manual_seed(seed)
    B = len(n_tok)
    scale = dh ** -0.5
    qkv = (torch.randn(B, N, 3 * h * dh, generator=g)).to(BF16)
    w = torch.rand(B, N, generator=g)
    lse = torch.full((B, h, N), NAN, dtype=torch.float64)
    c_ref, r_ref = torch.zeros(B, N, dtype=torch.float64), torch.zeros(B, N, dtype=torch.float64)
    for b, n in enumerate(n_tok):
        rows = qkv[b, :n].double()
        lse[b, :, :n] = lse_from_qkv(rows, h, dh, scale)
        A = probs_from_qkv(rows, lse[b, :, :n], h, dh, scale).mean(0)
        c_ref[b, :n] = A[0] / 2
        c_ref[b, 0] += 0.5
        r_ref[b, :n] = (w[b, :n].double() @ A + w[b, :n].double()) / 2
        qkv[b, n:] = NAN
        w[b, n:] = NAN
    return qkv, lse.float(), w, c_ref, r_ref, scale


def _run_abi(qkv_rows, lse, w, n_tok, tok_off, B, N, h, dh, scale):
    """-> (c, r) [B, N] from the two entry points; qkv_rows [rows, 3 h dh] bf16, lse [B, h, N], w [B, N], n_tok / tok_off int32 or None"""
    q, l, ww = dev(qkv_rows), dev(lse), dev(w)
    nt = None if n_tok is None else dev(torch.tensor(n_tok, dtype=torch.int32))
    to = None if tok_off is None else dev(torch.tensor(tok_off, dtype=torch.int32))
    c, r = torch.full((B, N), NAN, device='cuda'), torch.full((B, N), NAN, device='cuda')
    ws = torch.empty(lib().ecgvit_rollout_workspace(B, N, h), dtype=torch.uint8, device='cuda')
    check(lib().ecgvit_rollout_cls(ptr(q), ptr(l), None, ptr(c), ptr(nt), ptr(to), B, N, h, dh, scale, hip.BF16, stream()), 'rollout_cls')
    check(lib().ecgvit_rollout_colsum(ptr(q), ptr(l), None, ptr(ww), ptr(r), ptr(ws), ptr(nt), ptr(to), B, N, h, dh, scale, hip.BF16, stream()),
          'rollout_colsum')
    torch.cuda.synchronize()
    return c.cpu(), r.cpu()


@pytest.mark.parametrize('dh,h,N,n_tok', [
    (64, 2, 251, [251, 130, 129, 128, 3, 2, 1]),     # 130 / 129 / 128: both sides of a 128-key block; 3, 2, 1: the smallest records
    (128, 2, 251, [251, 130, 129, 128, 3, 2, 1]),
    (64, 1, 2048, [2048, 1]),
    (128, 1, 2048, [2048]),
    (64, 3, 51, None),                               # uniform: n_tok = NULL
])
def test_abi_bf16_against_float64_in_every_row_layout(dh, h, N, n_tok):
    uniform = n_tok is None
    counts = [N] * 3 if uniform else n_tok
    B = len(counts)
    qkv, lse, w, c_ref, r_ref, scale = _abi_case(dh, h, N, counts, seed=N + dh + h)
    c, r = _run_abi(qkv.view(B * N, -1), lse, w, None if uniform else counts, None, B, N, h, dh, scale)
    ec, er = float((c.double() - c_ref).abs().max()), float((r.double() - r_ref).abs().max())
    print(f'rollout abi dh={dh} h={h} N={N}: max |c - f64| = {ec:.2e}, max |r - f64| = {er:.2e} (max r {float(r_ref.max()):.2f})')
    assert torch.isfinite(c).all() and torch.isfinite(r).all()          # NaN rows of qkv / lse / w were never read
    assert ec < ABI_TOL and er < ABI_TOL * max(1.0, float(r_ref.max()))
    for b, n in enumerate(counts):                                        # entries at k >= n_tok[b] are written as 0
        assert not c[b, n:].any() and not r[b, n:].any()
    # the same records packed: bit-identical
    off = [sum(counts[:b]) for b in range(B)]
    packed = torch.cat([qkv[b, :n] for b, n in enumerate(counts)])
    cp, rp = _run_abi(packed, lse, w, counts, off, B, N, h, dh, scale)
    assert torch.equal(cp, c) and torch.equal(rp, r)
    # record 0 alone at B = 1 (with its count, and -- it fills N -- as a uniform batch): bit-identical again
    assert counts[0] == N
    for nt in ([N], None):
        c1, r1 = _run_abi(qkv[0], lse[:1], w[:1], nt, None, 1, N, h, dh, scale)
        assert torch.equal(c1[0], c[0]) and torch.equal(r1[0], r[0])
    # finish on two layers (c, r): each record's maximum becomes exactly 1, nothing past n_b - 1 is touched, a one-token record stays zeros
    maps = torch.stack([c[:, 1:], r[:, 1:]], dim=1).contiguous()
    md = dev(maps)
    nt = None if uniform else dev(torch.tensor(counts, dtype=torch.int32))
    check(lib().ecgvit_rollout_finish(ptr(md), ptr(nt), B, 2, N, stream()), 'rollout_finish')
    out = md.cpu()
    for b, n in enumerate(counts):
        if n == 1:
            assert not out[b].any()
            continue
        assert float(out[b, :, :n - 1].max()) == 1.0
        assert not out[b, :, n - 1:].any()
        assert max_err(out[b, :, :n - 1], maps[b, :, :n - 1].double() / maps[b, :, :n - 1].double().max()) < 1e-6


# =====================================================================================================================================
# engines and the oracle
# =====================================================================================================================================
def _conf(hidden):
    return E.EcgVitConfig(max_signal_length=L_MAX, patch_size=P, hidden_size=hidden, num_hidden_layers=3, num_attention_heads=2,
                          intermediate_size=2 * hidden, hidden_dropout_prob=0., attention_probs_dropout_prob=0.)


def _pair(hidden, dtype, seed=11):
    torch.manual_seed(seed)
    conf = _conf(hidden)
    ref = O.OracleEcgVit(config=conf)
    ref.eval()
    m = E.EcgVit(config=conf, compute_dtype=dtype)
    m.load_state_dict(ref.state_dict())
    m.cuda().train()   # (the rollout pass is an eval pass whatever the mode: checked below)
    return conf, ref, m


def _oracle_map(ref, rec):
    """the reference's map of ONE record (C, l) run alone at its own length: the Recorder's hook on every layer's softmax, then the loop"""
    got = []
    hooks = [attn.fn.attend.register_forward_hook(lambda mod, i, o: got.append(o[0].detach())) for attn, _ in ref.vit.transformer.layers]
    with torch.no_grad():
        logits = ref(sample_values=rec.unsqueeze(0)).logits[0]
    for hk in hooks:
        hk.remove()
    return logits, rollout_reference(torch.stack(got))


@pytest.fixture(scope='module')
def f32_case():
    """the f32 model, its six records, and the oracle's map of each record alone at full width and at LENGTHS (computed once, never changed)"""
    conf, ref, m = _pair(128, F32)
    x, _ = O.synthetic_batch(6, length=L_MAX, seed=3)
    full = [_oracle_map(ref, x[b]) for b in range(6)]
    cut = [_oracle_map(ref, x[b, :, :l]) for b, l in enumerate(LENGTHS)]
    return conf, m, x, full, cut


def _check_maps(out, want, counts, tol, what):
    """out: RolloutOutput; want: per record (logits | None, map (Ly, n_b)) float64"""
    assert out.patch_counts.dtype == torch.int64 and not out.patch_counts.is_cuda and out.patch_counts.tolist() == counts
    assert out.maps.dtype == F32 and out.maps.is_cuda and out.maps.shape == (len(counts), 3, max(counts))
    worst = 0.0
    for b, n in enumerate(counts):
        worst = max(worst, max_err(out.maps[b, :, :n], want[b][1]))
        assert not out.maps[b, :, n:].any(), (what, b)
        assert float(out.maps[b].max()) == 1.0, (what, b)
    print(f'rollout {what}: max |map - reference| = {worst:.2e}')
    assert worst < tol, (what, worst)
    return worst


def test_f32_engine_against_the_oracle(f32_case):
    conf, m, x, full, cut = f32_case
    xd = x.cuda()
    out = m.attention_rollout_batch(xd)
    assert m.training                                                   # left as it was
    _check_maps(out, full, [250] * 6, 1e-5, 'f32 full width')
    assert max_err(out.logits, torch.stack([f[0] for f in full])) < 1e-4
    m.eval()
    with torch.no_grad():
        assert torch.equal(out.logits, m(sample_values=xd).logits)
    logits0, map0 = m.attention_rollout(xd[0])                          # the existing one-record form
    assert max_err(out.maps[0], map0) < 1e-5 and max_err(out.logits[0], logits0) < 1e-5
    lens = torch.tensor(LENGTHS)
    out = m.attention_rollout_batch(xd, lengths=lens)
    _check_maps(out, cut, [l // P for l in LENGTHS], 1e-5, 'f32 lengths=')
    with torch.no_grad():
        assert torch.equal(out.logits, m(sample_values=xd, lengths=lens).logits)
    with pytest.raises(RuntimeError, match='per-record lengths'):
        m.attention_probs(0)


def _closed_forms(m, rows_of, counts):
    """per record the closed form on the engine's OWN qkv / lse of the pass it just ran; rows_of(b) = the record's first token row"""
    eng = m._engine()
    h, dh, N = eng.h, eng.dh, eng.T
    want = []
    for b, n in enumerate(counts):
        qkvs = [L['qkv'][rows_of(b):rows_of(b) + n + 1].float().cpu() for L in eng.act['layers']]
        lses = [L['lse'].view(-1, h, N)[b, :, :n + 1].cpu() for L in eng.act['layers']]
        want.append((None, rollout_closed_form_qkv(qkvs, lses, h, dh, eng.scale)))
    return want


@pytest.mark.parametrize('hidden', [128, 256])   # dh = 64, dh = 128
def test_bf16_engine_in_every_batch_form(hidden):
    conf, ref, m = _pair(hidden, BF16)
    x, _ = O.synthetic_batch(6, length=L_MAX, seed=3)
    xd = x.cuda()
    counts = [l // P for l in LENGTHS]
    # padded, full width: against the closed form on its own qkv / lse, and against the reference loop on its own exported probabilities
    out = m.attention_rollout_batch(xd)
    N = m._engine().T
    worst = _check_maps(out, _closed_forms(m, lambda b: b * N, [250] * 6), [250] * 6, BF16_TOL, f'bf16 d={hidden} padded')
    probs = torch.stack([m.attention_probs(i).cpu() for i in range(3)], dim=1)      # (B, Ly, h, N, N)
    e = max(max_err(out.maps[b], rollout_reference(probs[b])) for b in range(6))
    print(f'rollout bf16 d={hidden} padded: max |map - reference loop on the exported probabilities| = {e:.2e}')
    assert e < BF16_PROBS_TOL
    m.eval()
    with torch.no_grad():
        assert torch.equal(out.logits, m(sample_values=xd).logits)
    # lengths=
    lens = torch.tensor(LENGTHS)
    out_l = m.attention_rollout_batch(xd, lengths=lens)
    worst = max(worst, _check_maps(out_l, _closed_forms(m, lambda b: b * N, counts), counts, BF16_TOL, f'bf16 d={hidden} lengths='))
    with pytest.raises(RuntimeError, match='per-record lengths'):
        m.attention_probs(0)
    # ragged: the same records packed
    xr = torch.cat([x[b, :, :l] for b, l in enumerate(LENGTHS)], dim=1).contiguous().cuda()
    out_r = m.attention_rollout_batch(xr, lengths=lens)
    off = m._engine().saved['ragged'].tok_off.tolist()
    worst = max(worst, _check_maps(out_r, _closed_forms(m, lambda b: off[b], counts), counts, BF16_TOL, f'bf16 d={hidden} ragged'))
    e = max_err(out_r.maps, out_l.maps)
    print(f'rollout bf16 d={hidden}: max |ragged - lengths=| = {e:.2e}')
    assert e < BF16_TOL and max_err(out_r.logits, out_l.logits) < 5e-2
    with pytest.raises(RuntimeError, match='ragged'):
        m.attention_probs(0)
    # raw records under a per-record input transform, padded and ragged
    m.set_input_transform(E.FusedInputTransform(MEAN, STD, P, per_record=True))
    g = torch.Generator().manual_seed(9)
    recs = [torch.randn(C, l, generator=g) * 2 + 0.3 for l in RAW]
    xp = torch.full((6, C, 999), NAN)
    for b, r in enumerate(recs):
        xp[b, :, :r.shape[1]] = r
    raw = torch.tensor(RAW)
    out_p = m.attention_rollout_batch(xp.cuda(), lengths=raw)
    N = m._engine().T
    assert N == 251
    worst = max(worst, _check_maps(out_p, _closed_forms(m, lambda b: b * N, counts), counts, BF16_TOL, f'bf16 d={hidden} raw padded'))
    out_q = m.attention_rollout_batch(torch.cat(recs, dim=1).contiguous().cuda(), lengths=raw)
    off = m._engine().saved['ragged'].tok_off.tolist()
    worst = max(worst, _check_maps(out_q, _closed_forms(m, lambda b: off[b], counts), counts, BF16_TOL, f'bf16 d={hidden} raw ragged'))
    assert max_err(out_q.maps, out_p.maps) < BF16_TOL
    print(f'rollout bf16 d={hidden}: max over every form |map - closed form on own qkv / lse| = {worst:.2e}')


def test_refusals_after_other_forwards():
    conf, ref, m = _pair(128, BF16)
    x, _ = O.synthetic_batch(2, length=L_MAX, seed=3)
    eng = m._engine()
    eng.forward(x.cuda(), None, None, training=False, cls_only_last=True)
    with pytest.raises(RuntimeError, match='cls_only_last'):
        eng.attention_rollout_saved()
    mm = E.MaskedEcgVit(m).cuda()
    mm(x.cuda(), mm.random_mask_indices(2))
    with pytest.raises(RuntimeError, match='masked objective'):
        m._engine().attention_rollout_saved()


def test_batch_rollout_never_holds_a_score_matrix():
    """bf16, B = 16, N = 251, h = 2: the second call's peak above the resting allocation stays below ONE layer's (B, h, N, N) f32 tensor"""
    conf, ref, m = _pair(128, BF16)
    x, _ = O.synthetic_batch(16, length=L_MAX, seed=4)
    xd = x.cuda()
    out = m.attention_rollout_batch(xd)
    del out
    torch.cuda.synchronize()
    rest = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = m.attention_rollout_batch(xd)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - rest
    one_layer = 16 * 2 * 251 * 251 * 4
    print(f'rollout memory: peak above rest {peak} B, one layer of (B, h, N, N) f32 {one_layer} B')
    assert 0 < peak < one_layer
    assert out.maps.shape == (16, 3, 250)


def test_hip_rollout_walks_a_resident_set():
    conf, ref, m = _pair(128, BF16)
    lengths = [1000, 400, 8, 4, 996, 516, 200, 640, 12, 804]
    x, _ = O.synthetic_batch(10, length=L_MAX, seed=6)
    lens = torch.tensor(lengths)
    forms = [('padded', x.cuda(), lens),
             ('ragged', torch.cat([x[b, :, :l] for b, l in enumerate(lengths)], dim=1).contiguous().cuda(), lens)]
    for what, xs, ls in forms:
        logits, maps, counts = E.HipRollout(m, batch_size=4).rollout(xs, lengths=ls)
        assert counts.tolist() == [l // P for l in lengths] and maps.shape == (10, 3, 250) and logits.shape == (10, 71)
        parts = []
        for s in range(0, 10, 4):
            e = min(s + 4, 10)
            if xs.dim() == 2:
                a, b2 = sum(lengths[:s]), sum(lengths[:e])
                parts.append(m.attention_rollout_batch(xs[:, a:b2].contiguous(), lengths=ls[s:e]))
            else:
                parts.append(m.attention_rollout_batch(xs[s:e], lengths=ls[s:e]))
        assert torch.equal(logits, torch.cat([p.logits for p in parts])), what
        wide = torch.zeros_like(maps)
        for i, p in enumerate(parts):
            wide[4 * i:4 * i + p.maps.shape[0], :, :p.maps.shape[2]] = p.maps
        assert torch.equal(maps, wide), what
        assert [p.maps.shape[2] for p in parts] == [250, 249, 201], what     # each batch at its own widest record, the set padded to 250
    # raw records under a per-record transform: the same walk at the raw offsets
    m.set_input_transform(E.FusedInputTransform(MEAN, STD, P, per_record=True))
    g = torch.Generator().manual_seed(9)
    raw = [997, 400, 7, 3, 995, 515, 199, 640, 11, 801]
    recs = [torch.randn(C, l, generator=g) for l in raw]
    xr = torch.cat(recs, dim=1).contiguous().cuda()
    logits, maps, counts = E.HipRollout(m, batch_size=4).rollout(xr, lengths=torch.tensor(raw))
    assert counts.tolist() == [l // P + 1 for l in raw] and maps.shape == (10, 3, 250)
    one = m.attention_rollout_batch(torch.cat(recs[4:8], dim=1).contiguous().cuda(), lengths=torch.tensor(raw[4:8]))
    assert torch.equal(maps[4:8, :, :one.maps.shape[2]], one.maps) and torch.equal(logits[4:8], one.logits)
