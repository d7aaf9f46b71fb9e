"""
CPU tests that pin tests/attention_ref.py: the float64 restatement agrees with torch itself (autograd through softmax / logsumexp, with and
without dropout multipliers, uniform and per-record lengths, dh 64 and 128), and every committed constant C[name] sits >= 4x above the
bf16-staged restatement and <= 1/2 x below every applicable perturbation, for every case list tests/test_gpu_attention_ref.py runs.
"""
import pytest
import torch

import attention_ref as R
from attention_ref import C, F64, BF16, judge


# ===================================================================================================================== f64 against torch
def _torch_attention(qkv, do, B, N, h, dh, n_tok, mult):
    d = h * dh
    x = qkv.double().requires_grad_(True)
    q, k, v = (x[:, i * d:(i + 1) * d].reshape(B, N, h, dh).permute(0, 2, 1, 3) for i in range(3))
    s = q @ k.transpose(-1, -2) * float(torch.tensor(dh ** -0.5, dtype=torch.float32))
    valid = torch.ones(B, N, dtype=torch.bool) if n_tok is None else torch.arange(N)[None] < torch.tensor(n_tok)[:, None]
    s = s.masked_fill(~valid[:, None, None, :], float('-inf'))
    p = torch.softmax(s, -1)
    lse = torch.logsumexp(s, -1) * valid[:, None, :]
    o = ((p if mult is None else p * mult) @ v).permute(0, 2, 1, 3).reshape(B, N, d) * valid[:, :, None]
    o.backward(do.double().view(B, N, d))
    gq, gk, gv = (x.grad[:, i * d:(i + 1) * d].view(B, N, d) for i in range(3))
    return dict(out=o.detach(), lse=lse.detach(), dQ=gq, dK=gk, dV=gv, probs=(p * valid[:, None, :, None]).detach())


@pytest.mark.parametrize('dh', [64, 128])
@pytest.mark.parametrize('lengths', [None, [1, 33, 40]], ids=['uniform', 'varlen'])
@pytest.mark.parametrize('dropout', [False, True], ids=['p0', 'p0.1'])
@pytest.mark.parametrize('family', R.FAMILIES)
def test_f64_restatement_agrees_with_torch(dh, lengths, dropout, family):
    B, N, h = 3, 40, 2
    c = R.case(N, dh, B, h, family, lengths)
    qkv, do = R.case_inputs(c)
    mult = R.cpu_mult(B, h, N, 0.1, 5, range(B)) if dropout else None
    ref, mag = R.attention(qkv, do, B, N, h, dh, n_tok=lengths, mult=mult, probs=True)
    want = _torch_attention(qkv, do, B, N, h, dh, lengths, mult)
    for name in ('out', 'lse', 'dQ', 'dK', 'dV', 'probs'):
        err = float((ref[name] - want[name]).abs().max())
        assert err <= 1e-12 * max(1.0, float(want[name].abs().max())), (name, err)
        assert bool((mag[name] >= 0).all())
    # the CLS form is row 0 of the full form under a gradient that is zero off row 0
    do0 = do.view(B, N, h * dh).clone()
    do0[:, 1:] = 0
    want = _torch_attention(qkv, do0, B, N, h, dh, lengths, mult)
    cl, _ = R.attention(qkv, do0[:, 0].contiguous(), B, N, h, dh, n_tok=lengths, mult=mult, cls=True)
    for name, w in (('out', want['out'][:, 0]), ('lse', want['lse'][:, :, 0]), ('dQ', want['dQ'][:, 0]), ('dK', want['dK']), ('dV', want['dV'])):
        assert float((cl[name] - w).abs().max()) <= 1e-12 * max(1.0, float(w.abs().max())), name


def test_windowed_dq_is_the_same_sum_in_f64():
    c = R.case(513, 64, 1, 1, 'planted')
    qkv, do = R.case_inputs(c)
    a, _ = R.attention(qkv, do, 1, 513, 1, 64, dq_windows=True)
    b, _ = R.attention(qkv, do, 1, 513, 1, 64, dq_windows=False)
    assert float((a['dQ'] - b['dQ']).abs().max()) <= 1e-12 * float(b['dQ'].abs().max())


# ===================================================================================================================== calibration
def one_head(c, qkv, do):
    """full rows of 1025 tokens and more are calibrated on their first head (a CLS row costs nothing: it keeps its heads)"""
    if c['N'] < 1025 or c['h'] == 1 or c['cls']:
        return c, qkv, do
    h, dh = c['h'], c['dh']
    qkv = qkv.view(-1, 3, h, dh)[:, :, 0].reshape(-1, 3 * dh).contiguous()
    do = do.view(-1, h, dh)[:, 0].contiguous()
    return dict(c, h=1), qkv, do


def calibrate(c, recs, names, probs=False, forward_only=False):
    """(staged: {output: worst ratio}, perturbed: {perturbation: (best output, its ratio)}) over the records `recs` of a case"""
    qkv, do = R.case_inputs(c, recs)
    lengths = [c['lengths'][b] for b in recs] if c['lengths'] else None
    c1, qkv, do = one_head(c, qkv, do)
    B, N, h, dh = len(recs), c['N'], c1['h'], c['dh']
    kw = dict(n_tok=lengths, cls=c['cls'])
    mult = R.cpu_mult(c['B'], h, N, c['p'], 11, recs) if c['p'] else None
    ref, mag = R.attention(qkv, do, B, N, h, dh, mult=mult, probs=probs, **kw)
    st, _ = R.attention(qkv, do, B, N, h, dh, dtype=BF16, mult=mult, probs=probs, **kw)
    outputs = (('out', 'lse') if forward_only else ('out', 'lse', 'dQ', 'dK', 'dV')) + (('probs',) if probs else ())
    staged = {o: judge(o, st[o], ref[o], mag[o]) for o in outputs}
    perturbed = {}
    for name in names:
        if not any(R.applies(name, c, n) for n in (lengths or [N])):
            continue
        m2 = R.cpu_mult(c['B'], h, N, c['p'], 11, recs, c['lengths']) if name == 'mask_index_uses_n_tok' else mult
        pr, _ = R.attention(qkv, do, B, N, h, dh, mult=m2, perturb=name, **kw)
        held = [o for o in R.PERTURBATIONS[name] if o in outputs]
        perturbed[name] = max(((o, judge(o, pr[o], ref[o], mag[o])) for o in held), key=lambda t: t[1] / C[t[0]])
    return staged, perturbed


def check_constants(cases, names=tuple(R.PERTURBATIONS), **kw):
    """a uniform case is judged over the records the GPU test holds; a variable-length case one record at a time, so that every perturbation is
    shown to separate at every length it applies to, not only somewhere in the batch"""
    worst, nearest = {}, {}
    for c in cases:
        units = [[b] for b in R.case_records(c)] if c['lengths'] else [R.case_records(c)]
        for recs in units:
            staged, perturbed = calibrate(c, recs, names, **kw)
            cid = R.case_id(c) + (f"-n{c['lengths'][recs[0]]}" if c['lengths'] else '')
            print('CAL', cid, {k: round(v, 2) for k, v in staged.items()}, {k: (o, round(v, 1)) for k, (o, v) in perturbed.items()})
            for o, r in staged.items():
                worst[o] = max(worst.get(o, 0.0), r)
            for name, (o, r) in perturbed.items():
                if o not in nearest or r < nearest[o][1]:
                    nearest[o] = (name, r, cid)
    print('TABLE', {o: round(r, 2) for o, r in worst.items()}, nearest)
    for o, r in worst.items():
        assert r <= C[o] / 4, (o, r, C[o])
    for o, (name, r, cid) in nearest.items():
        assert r >= 2 * C[o], (o, name, r, cid, C[o])


def test_constants_uniform_dh64():
    check_constants([c for c in R.UNIFORM_CASES if c['dh'] == 64])


def test_constants_uniform_dh128():
    check_constants([c for c in R.UNIFORM_CASES if c['dh'] == 128])


def test_constants_many_items():
    check_constants(R.MANY_ITEM_CASES)


def test_constants_varlen():
    check_constants(R.VARLEN_CASES)


def test_constants_cls():
    check_constants(R.CLS_CASES)


def test_constants_dropout():
    check_constants(R.DROPOUT_CASES)


def test_constants_profiles_forward():
    """the C / 4 half of the rule only: the forward's perturbations drop one (query, key) pair and are held on the planted family (R.EDGE_PAIR),
    so none is held on the score profiles"""
    check_constants(R.PROFILE_CASES, names=(), forward_only=True)


def test_constants_probs():
    check_constants(R.PROBS_CASES, names=(), probs=True, forward_only=True)
