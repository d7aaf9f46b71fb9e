"""
The fused bf16 attention (csrc/attention.hip, csrc/attention_varlen.hip) through the C ABI, against the float64 restatement of
tests/attention_ref.py, element by element, in the units and with the constants that tests/test_attention_ref.py calibrates on the CPU.  Every
output is a slice of a larger buffer whose sentinel guard bands must come back bit-identical, and is pre-filled with NaN; the backward runs on
the `out` and `lse` the forward kernel left behind.  The fp64 reference runs on the device for at most three records of a uniform case (first,
middle, last) and for every record of a variable-length case (each length is a case of its own); NaN-freedom, the zeros of padded rows and the
guard bands are checked over the whole batch.  Each figure is printed (`RATIO case output value`) before it is asserted.
"""
import pytest
import torch

import attention_ref as R
from attention_ref import C, F32, F64, BF16, judge
from hiputil import ptr, check, stream, _attn_prob_mult_bf16, Guarded
from ecg_representation_learning_amd import hip
from ecg_representation_learning_amd.hip import lib

pytestmark = pytest.mark.gpu

SEED = 1234


class Figures:
    """prints every ratio of a case, then asserts them all"""

    def __init__(self, c):
        self.cid, self.bad = R.case_id(c), []

    def hold(self, name, got, ref, mag):
        r = judge(name, got, ref, mag)
        print(f'RATIO {self.cid} {name} {r:.4g}')
        if not r <= C[name]:
            self.bad.append((name, r, C[name]))

    def done(self):
        assert not self.bad, (self.cid, self.bad)


def run_case(c, probs=False, forward_only=False):
    B, N, h, dh, p = c['B'], c['N'], c['h'], c['dh'], c['p']
    d, scale = h * dh, dh ** -0.5
    recs = R.case_records(c)
    qkv_h, do_h = R.case_inputs(c)
    qkv, do = qkv_h.to(BF16).cuda(), do_h.to(BF16).cuda()
    lengths = c['lengths']
    nt = torch.tensor(lengths, dtype=torch.int32, device='cuda') if lengths else None
    mult = _attn_prob_mult_bf16(B, h, N, p, SEED) if p else None      # (dh = 64 probe: the contract gives both head widths the same bits)
    L = lib()
    nq = 1 if c['cls'] else N
    out, lse = Guarded(B * nq * d, BF16), Guarded(B * h * nq, F32)
    if c['cls'] and lengths:
        check(L.ecgvit_attention_varlen_cls_fwd(ptr(qkv), ptr(out.t), ptr(lse.t), ptr(nt), B, N, h, dh, scale, p, SEED, stream()), 'varlen_cls_fwd')
    elif c['cls']:
        check(L.ecgvit_attention_cls_fwd(ptr(qkv), ptr(out.t), ptr(lse.t), B, N, h, dh, scale, p, SEED, hip.BF16, stream()), 'cls_fwd')
    elif lengths:
        check(L.ecgvit_attention_varlen_fwd(ptr(qkv), ptr(out.t), ptr(lse.t), ptr(nt), B, N, h, dh, scale, p, SEED, stream()), 'varlen_fwd')
    else:
        check(L.ecgvit_attention_fwd(ptr(qkv), ptr(out.t), ptr(lse.t), B, N, h, dh, scale, p, SEED, hip.BF16, stream()), 'attention_fwd')
    got = dict(out=out.t.view(B, nq, d), lse=lse.t.view(B, h, nq))
    guarded = dict(out=out, lse=lse)
    if not forward_only:
        dqkv = Guarded(B * N * 3 * d, BF16)
        guarded['dqkv'] = dqkv
        if c['cls']:
            dq = Guarded(B * d, BF16)
            guarded['dq_cls'] = dq
            if lengths:
                check(L.ecgvit_attention_varlen_cls_bwd(ptr(qkv), ptr(out.t), ptr(do), ptr(lse.t), ptr(dqkv.t), ptr(dq.t), ptr(nt), B, N, h, dh, scale, p,
                                                        SEED, stream()), 'varlen_cls_bwd')
            else:
                check(L.ecgvit_attention_cls_bwd(ptr(qkv), ptr(out.t), ptr(do), ptr(lse.t), ptr(dqkv.t), ptr(dq.t), B, N, h, dh, scale, p, SEED, hip.BF16,
                                                 stream()), 'cls_bwd')
        elif lengths:
            check(L.ecgvit_attention_varlen_bwd(ptr(qkv), ptr(out.t), ptr(do), ptr(lse.t), ptr(dqkv.t), ptr(nt), B, N, h, dh, scale, p, SEED, stream()),
                  'varlen_bwd')
        else:
            check(L.ecgvit_attention_bwd(ptr(qkv), ptr(out.t), ptr(do), ptr(lse.t), ptr(dqkv.t), B, N, h, dh, scale, p, SEED, hip.BF16, stream()),
                  'attention_bwd')
        g3 = dqkv.t.view(B, N, 3, d)
        got.update(dQ=dq.t.view(B, 1, d) if c['cls'] else g3[:, :, 0], dK=g3[:, :, 1], dV=g3[:, :, 2])
        if c['cls']:
            assert bool(torch.isnan(g3[:, :, 0]).all()), 'the CLS backward touched the Q columns of dqkv'
    torch.cuda.synchronize()
    for name, gd in guarded.items():
        assert gd.bands_ok(), name
    for name, t in got.items():
        assert not bool(torch.isnan(t.float()).any()), f'{name}: an element was never written'
    if lengths:    # padded rows: exact zeros, their LSE exactly 0
        valid = torch.arange(N, device='cuda')[None] < nt[:, None]
        for name, t in got.items():
            if t.shape[1] == N and name != 'lse':
                assert bool((t[~valid] == 0).all()), f'{name}: a padded row is not zero'
        if not c['cls']:
            assert bool((got['lse'].permute(0, 2, 1)[~valid] == 0).all()), 'lse: a padded row is not 0'
    # ---- fp64 on the device, the records `recs`
    ridx = torch.tensor(recs, device='cuda')
    rq = qkv.view(B, N, 3 * d)[ridx].double().reshape(-1, 3 * d)
    rdo = do.view(B, nq, d)[ridx].double().reshape(-1, d)
    ref, mag = R.attention(rq, rdo, len(recs), N, h, dh, n_tok=[lengths[b] for b in recs] if lengths else None,
                           mult=None if mult is None else mult[recs].to('cuda', F64), cls=c['cls'], probs=probs)
    fig = Figures(c)
    for name, t in got.items():
        r = ref[name].view(len(recs), -1, d) if name != 'lse' else ref[name].view(len(recs), h, -1)
        fig.hold(name, t[ridx], r, mag[name])
    if probs:    # from the reference's LSE as a forward stores it (f32), so the figure is the export kernel's own
        lse_ref = torch.zeros(B, h, N, device='cuda')
        lse_ref[ridx] = ref['lse'].float()
        pr = Guarded(B * h * N * N, F32)
        check(L.ecgvit_attention_probs(ptr(qkv), ptr(lse_ref), ptr(pr.t), B, N, h, dh, scale, hip.BF16, stream()), 'attention_probs')
        torch.cuda.synchronize()
        assert pr.bands_ok(), 'probs'
        fig.hold('probs', pr.t.view(B, h, N, N)[ridx], ref['probs'], mag['probs'])
    fig.done()


@pytest.mark.parametrize('c', R.UNIFORM_CASES + R.MANY_ITEM_CASES, ids=R.case_id)
def test_uniform(c):
    """dh = 64: the one-item backward up to 128 tokens, the persistent backward with one, two and up to eight key windows, the forward's one-item
    and split forms, and with an item per CU (MANY_ITEM_CASES: 260 items at 300 tokens, 384 items of 512 queries at 1025) its streamed and
    512-query-block forms; dh = 128: the 128-query / 128-key blocks with 64-key windows"""
    run_case(c)


@pytest.mark.parametrize('c', R.VARLEN_CASES, ids=R.case_id)
def test_varlen(c):
    run_case(c)


@pytest.mark.parametrize('c', R.CLS_CASES, ids=R.case_id)
def test_cls_rows(c):
    """out_cls, lse_cls, dq_cls and the K and V parts of dqkv against row 0 of the fp64 reference"""
    run_case(c)


@pytest.mark.parametrize('c', R.DROPOUT_CASES, ids=R.case_id)
def test_dropout(c):
    """p = 0.1: the multipliers are read from the forward kernel itself, at the batch N, and go to the reference of both passes"""
    run_case(c)


@pytest.mark.parametrize('c', R.PROFILE_CASES, ids=R.case_id)
def test_forward_profiles(c):
    run_case(c, forward_only=True)


@pytest.mark.parametrize('c', R.PROBS_CASES, ids=R.case_id)
def test_probs(c):
    run_case(c, probs=True, forward_only=True)
