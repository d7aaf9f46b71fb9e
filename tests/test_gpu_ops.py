"""-m gpu: every C-ABI op against a CPU reference on the same seeded inputs (f32: <= 1e-5 relative, the noise of
accumulation order; bf16: inputs rounded to bf16 first, outputs within bf16 rounding; integer indexing: bit-exact)."""
import math

import numpy as np
import pytest
import torch

from hiputil import dev, rel_err, max_err, gelu, gelu_grad, lib, tools_lib, check, ptr, stream, hip
from oracle import vit_oracle as O

pytestmark = pytest.mark.gpu
F32, BF16 = torch.float32, torch.bfloat16


def test_fragment_layout_probe():
    """pins row_frag / tr_frag32 (ds_read_b64_tr_b16) / the 32x32 accumulator map with exact integers"""
    out = torch.zeros(4, 64, 16, device='cuda')
    check(tools_lib().ecgvit_probe_mfma_layout(ptr(out), stream()), 'probe')
    o = out.cpu().numpy()
    for lane in range(64):
        r, h = lane & 31, lane >> 5
        for j in range(8):
            assert o[0, lane, j] == 2 * (32 + r), ('row_frag row', lane, j)
            assert o[0, lane, 8 + j] == 16 + 8 * h + j, ('row_frag col', lane, j)
            assert o[1, lane, j] == 2 * (16 + 8 * (j >> 2) + 4 * h + (j & 3)) + 1, ('tr_frag row', lane, j, o[1, lane, j])
            assert o[1, lane, 8 + j] == 32 + r, ('tr_frag col', lane, j)
        for reg in range(16):
            assert o[2, lane, reg] == (reg & 3) + 8 * (reg >> 2) + 4 * h, ('acc row', lane, reg)
            assert o[3, lane, reg] == r, ('acc col', lane, reg)


# ----------------------------------------------------------------------------------------------------------- GEMM
def _gemm_ref(layout, A, B):
    A, B = A.double(), B.double()
    if layout == hip.GEMM_NT:
        return A @ B.T
    if layout == hip.GEMM_NN:
        return A @ B
    return A.T @ B


def _operands(layout, M, N, K, dtype, g):
    shA = (K, M) if layout == hip.GEMM_TN else (M, K)
    shB = (N, K) if layout == hip.GEMM_NT else (K, N)
    A = torch.randn(*shA, generator=g).to(dtype)
    B = torch.randn(*shB, generator=g).to(dtype)
    return A, B


@pytest.mark.parametrize('layout', [hip.GEMM_NT, hip.GEMM_NN, hip.GEMM_TN])
@pytest.mark.parametrize('shape', [(37, 29, 19), (128, 128, 16), (200, 96, 70), (1, 5, 3), (300, 260, 130)])
def test_gemm_f32_plain(layout, shape):
    M, N, K = shape
    g = torch.Generator().manual_seed(M * 1000 + N * 10 + layout)
    A, B = _operands(layout, M, N, K, F32, g)
    C = torch.full((M, N), float('nan'), device='cuda')
    hip.gemm(layout, dev(A), dev(B), C, M, N, K, A.shape[1], B.shape[1], N)
    assert rel_err(C, _gemm_ref(layout, A, B)) < 2e-6


def test_gemm_f32_epilogues():
    g = torch.Generator().manual_seed(5)
    M, N, K = 70, 40, 33
    A, B = _operands(hip.GEMM_NT, M, N, K, F32, g)
    bias, res = torch.randn(N, generator=g), torch.randn(M, N, generator=g)
    base = _gemm_ref(hip.GEMM_NT, A, B)
    # bias + gelu (aux = pre-activation) + residual, alpha
    C, aux = torch.zeros(M, N, device='cuda'), torch.zeros(M, N, device='cuda')
    hip.gemm(hip.GEMM_NT, dev(A), dev(B), C, M, N, K, K, K, N, epilogue=hip.EPI_BIAS | hip.EPI_GELU | hip.EPI_RESIDUAL,
             bias=dev(bias), residual=dev(res), ldr=N, aux=aux, ldaux=N, alpha=0.5)
    pre = 0.5 * base + bias.double()
    assert rel_err(aux, pre) < 2e-6
    assert rel_err(C, gelu(pre) + res.double()) < 2e-6
    # gelu backward multiply
    C2 = torch.zeros(M, N, device='cuda')
    hip.gemm(hip.GEMM_NT, dev(A), dev(B), C2, M, N, K, K, K, N, epilogue=hip.EPI_GELU_BWD, aux=dev(res), ldaux=N)
    assert rel_err(C2, base * gelu_grad(res)) < 2e-6
    # accumulate
    C3 = dev(res.clone())
    hip.gemm(hip.GEMM_NT, dev(A), dev(B), C3, M, N, K, K, K, N, epilogue=hip.EPI_ACCUM)
    assert rel_err(C3, base + res.double()) < 2e-6


def test_gemm_f32_batched_strided_heads():
    """the attention use: q/k/v column slices of a [B*N, 3d] buffer, 2-level batch (record, head), odd N"""
    g = torch.Generator().manual_seed(6)
    B, N, h, dh = 3, 41, 2, 16
    d = h * dh
    qkv = torch.randn(B * N, 3 * d, generator=g)
    S = torch.zeros(B * h * N * N, device='cuda')
    sq = (N * 3 * d, dh)
    hip.gemm(hip.GEMM_NT, dev(qkv), dev(qkv), S, N, N, dh, 3 * d, 3 * d, N, alpha=0.25, batch=(B, h), strideA=sq, strideB=sq,
             strideC=(h * N * N, N * N), b_off=d)
    q = qkv[:, :d].reshape(B, N, h, dh).permute(0, 2, 1, 3).double()
    k = qkv[:, d:2 * d].reshape(B, N, h, dh).permute(0, 2, 1, 3).double()
    v = qkv[:, 2 * d:].reshape(B, N, h, dh).permute(0, 2, 1, 3).double()
    ref = 0.25 * q @ k.transpose(-1, -2)
    assert rel_err(S.view(B, h, N, N), ref) < 2e-6
    out = torch.zeros(B * N, d, device='cuda')
    P = torch.softmax(ref, -1).float()
    hip.gemm(hip.GEMM_NN, dev(P.reshape(-1)), dev(qkv), out, N, dh, N, N, 3 * d, d, batch=(B, h), strideA=(h * N * N, N * N),
             strideB=sq, strideC=(N * d, dh), b_off=2 * d)
    ref_o = (P.double() @ v).permute(0, 2, 1, 3).reshape(B * N, d)
    assert rel_err(out, ref_o) < 2e-6
    dq = torch.zeros(B * N, 3 * d, device='cuda')
    hip.gemm(hip.GEMM_TN, dev(P.reshape(-1)), dev(qkv), dq, N, dh, N, N, 3 * d, 3 * d, batch=(B, h), strideA=(h * N * N, N * N),
             strideB=sq, strideC=sq, c_off=d)
    ref_k = (P.double().transpose(-1, -2) @ q).permute(0, 2, 1, 3).reshape(B * N, d)
    assert rel_err(dq[:, d:2 * d], ref_k) < 2e-6


@pytest.mark.parametrize('layout', [hip.GEMM_NT, hip.GEMM_NN, hip.GEMM_TN])
@pytest.mark.parametrize('shape', [(128, 128, 64), (300, 192, 128), (1000, 264, 240), (251, 768, 768), (64, 8, 8)])
@pytest.mark.parametrize('out_dtype', [BF16, F32])
def test_gemm_bf16_plain(layout, shape, out_dtype):
    M, N, K = shape
    if layout == hip.GEMM_TN:
        M = (M + 7) // 8 * 8
    g = torch.Generator().manual_seed(M + N + K + layout)
    A, B = _operands(layout, M, N, K, BF16, g)
    C = torch.full((M, N), float('nan'), device='cuda', dtype=out_dtype)
    hip.gemm(layout, dev(A), dev(B), C, M, N, K, A.shape[1], B.shape[1], N)
    ref = _gemm_ref(layout, A.float(), B.float())
    assert torch.isfinite(C.float()).all()
    assert rel_err(C, ref) < (4e-3 if out_dtype == BF16 else 2e-5)


def test_gemm_bf16_splitk_wgrad():
    g = torch.Generator().manual_seed(11)
    Mout, Nin, rows = 256, 240, 5021  # rows: ragged contraction (zero-filled tail), split-K over the workspace
    dY = torch.randn(rows, Mout, generator=g).to(BF16)
    X = torch.randn(rows, Nin, generator=g).to(BF16)
    need = hip.gemm_workspace_bytes(hip.GEMM_TN, BF16, Mout, Nin, rows)
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device='cuda')
    C = torch.full((Mout, Nin), float('nan'), device='cuda')
    hip.gemm(hip.GEMM_TN, dev(dY), dev(X), C, Mout, Nin, rows, Mout, Nin, Nin, workspace=ws)
    ref = dY.double().T @ X.double()
    assert rel_err(C, ref) < 2e-5
    C2 = torch.full((Mout, Nin), float('nan'), device='cuda')
    hip.gemm(hip.GEMM_TN, dev(dY), dev(X), C2, Mout, Nin, rows, Mout, Nin, Nin)  # no workspace: single pass
    assert rel_err(C2, ref) < 2e-5


def test_gemm_bf16_epilogues():
    g = torch.Generator().manual_seed(12)
    M, N, K = 260, 136, 128
    A, B = _operands(hip.GEMM_NT, M, N, K, BF16, g)
    bias = torch.randn(N, generator=g)
    res = torch.randn(M, N, generator=g).to(BF16)
    base = _gemm_ref(hip.GEMM_NT, A.float(), B.float())
    C = torch.zeros(M, N, device='cuda', dtype=BF16)
    aux = torch.zeros(M, N, device='cuda', dtype=BF16)
    hip.gemm(hip.GEMM_NT, dev(A), dev(B), C, M, N, K, K, K, N, epilogue=hip.EPI_BIAS | hip.EPI_GELU, bias=dev(bias), aux=aux, ldaux=N)
    pre = base + bias.double()
    assert rel_err(aux, pre) < 4e-3
    assert rel_err(C, gelu(aux.float().double().cpu())) < 4e-3  # GELU of the STORED (bf16) pre-activation
    C = torch.zeros(M, N, device='cuda', dtype=BF16)
    hip.gemm(hip.GEMM_NT, dev(A), dev(B), C, M, N, K, K, K, N, epilogue=hip.EPI_BIAS | hip.EPI_RESIDUAL, bias=dev(bias),
             residual=dev(res), ldr=N)
    assert rel_err(C, pre + res.double()) < 4e-3
    C = torch.zeros(M, N, device='cuda', dtype=BF16)
    hip.gemm(hip.GEMM_NT, dev(A), dev(B), C, M, N, K, K, K, N, epilogue=hip.EPI_GELU_BWD, aux=dev(res), ldaux=N)
    assert rel_err(C, base * gelu_grad(res.float())) < 4e-3


def test_gemm_asking_equals_running():
    """ecgvit_gemm returns ECGVIT_OK exactly when ecgvit_gemm_kernel names a kernel family, and a rejected call writes nothing: C and
    colsum_out keep their sentinel.  Several hundred descriptors of the route sweep (tests/gemm_cases.py) on real buffers, every pointer
    present (misaligned where the case says so), among them the f32 COLSUM products with N % 8 != 0 that used to run and then fail"""
    import ctypes
    import re
    import gemm_cases as G
    cases = [(label, c) for i, (label, c) in enumerate(G.cases())
             if not re.search(r'\b(A|B|C|bias|residual|aux|workspace|colsum_out|q8_out|q8_scale|q8_amax|scale_a|scale_b|workspace_bytes)=0\b', label)
             and (i % 12 == 0 or 'COLSUM 500x12x64' in label or ('COLSUM' in label and label.startswith('0:2>1')))]
    assert len(cases) > 300, len(cases)
    es = {G.F32: 4, G.BF16: 2, G.E4M3: 1, G.E5M2: 1}
    slack = 256

    def need(c):   # bytes each pointer's buffer must cover (rows past the logical ones: slack for tile-granular reads)
        c = {**dict.fromkeys([f for f, _ in G.hip.GemmDesc._fields_], 0), **c}   # (the sweep drops zero fields)
        M, N, K, t, o = c['M'], c['N'], c['K'], es.get(c['dtype'], 4), 4 if c['out_dtype'] == G.F32 else 2
        a_rows, b_rows = (K if c['layout'] == G.TN else M), (N if c['layout'] == G.NT else K)
        return dict(A=(a_rows + slack) * c['lda'] * t, B=(b_rows + slack) * c['ldb'] * t, C=(M + slack) * c['ldc'] * o,
                    bias=4 * N, residual=(M + slack) * c['ldr'] * o, aux=(M + slack) * c['ldaux'] * o, workspace=c['workspace_bytes'],
                    colsum_out=4 * N, q8_out=(M + slack) * c['ldq8'], q8_scale=4, q8_amax=4, scale_a=4, scale_b=4)
    size = {p: 0 for p in G.POINTERS}
    for _, c in cases:
        for p, n in need(c).items():
            size[p] = max(size[p], n)
    assert sum(size.values()) < (3 << 30), size
    pool = {p: torch.zeros(n + 65536, dtype=torch.uint8, device='cuda') for p, n in size.items()}
    for p in ('q8_scale', 'scale_a', 'scale_b'):
        pool[p][:4].view(torch.float32).fill_(1.0)
    l = lib()
    SENT = 0x5A
    for label, c in cases:
        c = dict(c)
        for p in G.POINTERS:
            if p in c:
                c[p] = pool[p].data_ptr() + (c[p] - G.BASE_ADDR[p])
        n = need(c)
        pool['C'][:n['C']].fill_(SENT)
        pool['colsum_out'][:n['colsum_out']].fill_(SENT)
        d = G.fill(c)
        route = l.ecgvit_gemm_kernel(ctypes.byref(d))
        rc = l.ecgvit_gemm(ctypes.byref(d), stream())
        torch.cuda.synchronize()
        assert (rc == 0) == (route != hip.KERNEL_NONE), (label, rc, route)
        if rc != 0:
            assert bool((pool['C'][:n['C']] == SENT).all()) and bool((pool['colsum_out'][:n['colsum_out']] == SENT).all()), label


def test_gemm_dropout_epilogue_mask_is_reproducible():
    """the epilogue mask is a pure function of (seed, element): forward epilogue == ecgvit_dropout_apply on the same index"""
    g = torch.Generator().manual_seed(13)
    M, N, K = 192, 136, 64
    p, seed = 0.25, 1234
    for dtype in (F32, BF16):
        A, B = _operands(hip.GEMM_NT, M, N, K, dtype, g)
        C0 = torch.zeros(M, N, device='cuda', dtype=dtype)
        C1 = torch.zeros(M, N, device='cuda', dtype=dtype)
        hip.gemm(hip.GEMM_NT, dev(A), dev(B), C0, M, N, K, K, K, N)
        hip.gemm(hip.GEMM_NT, dev(A), dev(B), C1, M, N, K, K, K, N, epilogue=hip.EPI_DROPOUT, dropout_p=p, seed=seed)
        C2 = torch.empty_like(C0)
        check(lib().ecgvit_dropout_apply(ptr(C0), ptr(C2), M * N, p, seed, hip.code(dtype), stream()), 'dropout_apply')
        keep = (C1 != 0).float().mean().item()
        assert abs(keep - (1 - p)) < 0.02
        if dtype == F32:
            assert torch.equal(C1, C2)
        else:  # bf16: the epilogue scales the f32 accumulator, dropout_apply the rounded value
            assert torch.equal(C1 != 0, C2 != 0) and rel_err(C1, C2.float()) < 4e-3


# ------------------------------------------------------------------------------------------------------ row ops
@pytest.mark.parametrize('geom', [(2560, 64), (5000, 20), (40, 10), (1000, 20)])
@pytest.mark.parametrize('dtype', [F32, BF16])
def test_patch_gather_bit_exact(geom, dtype):
    L, P = geom
    B, C = 3, 12
    g = torch.Generator().manual_seed(L)
    x = torch.randn(B, C, L, generator=g)
    ld = C * P
    out = torch.full((B * (L // P), ld), float('nan'), device='cuda', dtype=dtype)
    check(lib().ecgvit_patch_gather(ptr(dev(x)), ptr(out), B, C, L, P, ld, hip.code(dtype), stream()), 'patch_gather')
    ref = torch.from_numpy(O.patch_gather_np(x.numpy(), P)).reshape(-1, ld).to(dtype)
    assert torch.equal(out.cpu(), ref)
    # arange input: pure integer pin, padded leading dimension zero-filled
    xi = torch.arange(B * C * L, dtype=torch.float32).reshape(B, C, L)
    ld2 = ld + 16
    out2 = torch.full((B * (L // P), ld2), float('nan'), device='cuda')
    check(lib().ecgvit_patch_gather(ptr(dev(xi)), ptr(out2), B, C, L, P, ld2, hip.F32, stream()), 'patch_gather')
    assert torch.equal(out2[:, :ld].cpu(), torch.from_numpy(O.patch_gather_np(xi.numpy(), P)).reshape(-1, ld))
    assert (out2[:, ld:] == 0).all()


@pytest.mark.parametrize('dtype', [F32, BF16])
def test_embed_finish_and_bwd(dtype):
    g = torch.Generator().manual_seed(3)
    B, n, d = 5, 13, 64
    N = n + 1
    tok = torch.randn(B * n, d, generator=g).to(dtype)
    cls, pos = torch.randn(d, generator=g), torch.randn(N, d, generator=g)
    X = torch.zeros(B * N, d, device='cuda', dtype=dtype)
    check(lib().ecgvit_embed_finish(ptr(dev(tok)), ptr(dev(cls)), ptr(dev(pos)), ptr(X), B, n, d, 0.0, 0, hip.code(dtype), stream()), 'ef')
    ref = torch.cat([cls.expand(B, 1, d), tok.float().view(B, n, d)], 1) + pos
    assert rel_err(X.view(B, N, d), ref) < (1e-6 if dtype == F32 else 4e-3)
    dX = torch.randn(B * N, d, generator=g).to(dtype)
    dtok = torch.zeros(B * n, d, device='cuda', dtype=dtype)
    dcls, dpos = torch.zeros(d, device='cuda'), torch.zeros(N, d, device='cuda')
    check(lib().ecgvit_embed_bwd(ptr(dev(dX)), ptr(dtok), ptr(dcls), ptr(dpos), B, n, d, 0.0, 0, hip.code(dtype), stream()), 'eb')
    r = dX.float().view(B, N, d)
    assert torch.equal(dtok.cpu().view(B, n, d), dX.view(B, N, d)[:, 1:])
    assert rel_err(dpos, r.sum(0)) < 1e-5 and rel_err(dcls, r[:, 0].sum(0)) < 1e-5


@pytest.mark.parametrize('d', [32, 128, 768, 1024, 2048])
@pytest.mark.parametrize('dtype', [F32, BF16])
def test_layernorm_fwd_bwd(d, dtype):
    g = torch.Generator().manual_seed(d)
    rows = 203
    x = (torch.randn(rows, d, generator=g) * 2 + 0.5).to(dtype)
    gamma, beta = torch.randn(d, generator=g), torch.randn(d, generator=g)
    y = torch.zeros(rows, d, device='cuda', dtype=dtype)
    mean, rstd = torch.zeros(rows, device='cuda'), torch.zeros(rows, device='cuda')
    check(lib().ecgvit_layernorm_fwd(ptr(dev(x)), ptr(dev(gamma)), ptr(dev(beta)), ptr(y), ptr(mean), ptr(rstd), rows, d, 1e-5,
                                     hip.code(dtype), stream()), 'ln')
    xr = x.double().requires_grad_(True)
    gr, br = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    yr = torch.nn.functional.layer_norm(xr, (d,), gr, br, 1e-5)
    tol = 2e-6 if dtype == F32 else 4e-3
    assert rel_err(y, yr) < tol
    assert rel_err(mean, x.double().mean(1)) < 1e-5
    dy = torch.randn(rows, d, generator=g).to(dtype)
    dres = torch.randn(rows, d, generator=g).to(dtype)
    yr.backward(dy.double())
    ws = torch.empty(lib().ecgvit_layernorm_bwd_workspace(rows, d), dtype=torch.uint8, device='cuda')
    for use_res in (False, True):
        dx = torch.zeros(rows, d, device='cuda', dtype=dtype)
        dg, db = torch.zeros(d, device='cuda'), torch.zeros(d, device='cuda')
        check(lib().ecgvit_layernorm_bwd(ptr(dev(dy)), ptr(dev(x)), ptr(dev(gamma)), ptr(mean), ptr(rstd),
                                         ptr(dev(dres)) if use_res else None, ptr(dx), ptr(dg), ptr(db), ptr(ws), rows, d,
                                         hip.code(dtype), stream()), 'lnb')
        ref_dx = xr.grad + (dres.double() if use_res else 0)
        assert rel_err(dx, ref_dx) < (1e-5 if dtype == F32 else 8e-3)
        assert rel_err(dg, gr.grad) < 1e-5 and rel_err(db, br.grad) < 1e-5


@pytest.mark.parametrize('dtype', [F32, BF16])
def test_colsum(dtype):
    g = torch.Generator().manual_seed(8)
    for (M, N) in ((1003, 72), (257, 3072), (5, 8)):
        x = torch.randn(M, N, generator=g).to(dtype)
        out = torch.zeros(N, device='cuda')
        ws = torch.empty(lib().ecgvit_colsum_workspace(M, N), dtype=torch.uint8, device='cuda')
        check(lib().ecgvit_colsum(ptr(dev(x)), N, ptr(out), ptr(ws), M, N, hip.code(dtype), stream()), 'colsum')
        assert rel_err(out, x.double().sum(0)) < 1e-5


def test_softmax_rows_fwd_bwd():
    g = torch.Generator().manual_seed(9)
    rows, N = 77, 251
    S = torch.randn(rows, N, generator=g) * 3
    Sd = dev(S.clone())
    check(lib().ecgvit_softmax_rows(ptr(Sd), rows, N, N, stream()), 'softmax')
    Pr = torch.softmax(S.double(), -1)
    assert rel_err(Sd, Pr) < 2e-6
    dP = torch.randn(rows, N, generator=g)
    dPd = dev(dP.clone())
    check(lib().ecgvit_softmax_bwd_rows(ptr(Sd), ptr(dPd), rows, N, N, 0.125, stream()), 'softmax_bwd')
    ref = Pr * (dP.double() - (Pr * dP.double()).sum(-1, keepdim=True)) * 0.125
    assert rel_err(dPd, ref) < 1e-5


# ------------------------------------------------------------------------------------------------------ head / loss
@pytest.mark.parametrize('dtype', [F32, BF16])
def test_head_bce_fwd_bwd(dtype):
    g = torch.Generator().manual_seed(10)
    B, N, d, K = 6, 7, 96, 71
    X = torch.randn(B * N, d, generator=g).to(dtype)
    gamma, beta = torch.randn(d, generator=g), torch.randn(d, generator=g)
    W, bias = torch.randn(K, d, generator=g) * 0.1, torch.randn(K, generator=g)
    y = (torch.rand(B, K, generator=g) < 0.1).float()
    wgt = torch.tensor([1.0, 3.0])[y.long()]
    Xd = dev(X)
    logits = torch.zeros(B, K, device='cuda')
    xhat, rstd = torch.zeros(B, d, device='cuda'), torch.zeros(B, device='cuda')
    args = [ptr(dev(gamma)), ptr(dev(beta)), ptr(dev(W)), ptr(dev(bias))]
    gd, bd, Wd, biasd = dev(gamma), dev(beta), dev(W), dev(bias)
    check(lib().ecgvit_head_fwd(ptr(Xd), N, ptr(gd), ptr(bd), ptr(Wd), ptr(biasd), ptr(logits), ptr(xhat), ptr(rstd), B, d, K, 1e-5,
                                hip.code(dtype), stream()), 'head_fwd')
    Xr = X.double().requires_grad_(True)
    pr = [t.double().requires_grad_(True) for t in (gamma, beta, W, bias)]
    cls_rows = Xr.view(B, N, d)[:, 0]
    z = torch.nn.functional.layer_norm(cls_rows, (d,), pr[0], pr[1], 1e-5) @ pr[2].T + pr[3]
    assert rel_err(logits, z) < 1e-5
    for weight in (None, wgt):
        le, lm = torch.zeros(B, K, device='cuda'), torch.zeros(1, device='cuda')
        check(lib().ecgvit_bce_fwd(ptr(logits), ptr(dev(y)), ptr(dev(weight)) if weight is not None else None, ptr(le), ptr(lm), B * K,
                                   stream()), 'bce')
        ref_le = torch.nn.functional.binary_cross_entropy_with_logits(z, y.double(), weight=None if weight is None else weight.double(),
                                                                      reduction='none')
        assert rel_err(le, ref_le) < 1e-5 and abs(float(lm) - float(ref_le.mean())) < 1e-6
    # backward through mean loss (weighted)
    for p_ in [Xr] + pr:
        p_.grad = None
    ref_le.mean().backward()
    dl = torch.zeros(B, K, device='cuda')
    one = torch.ones(1, device='cuda')
    check(lib().ecgvit_bce_bwd(ptr(logits), ptr(dev(y)), ptr(dev(wgt)), ptr(one), None, 1.0 / (B * K), ptr(dl), B * K, stream()), 'bce_bwd')
    dW, dbias = torch.zeros(K, d, device='cuda'), torch.zeros(K, device='cuda')
    dg, db = torch.zeros(d, device='cuda'), torch.zeros(d, device='cuda')
    dX = torch.full((B * N, d), 7.0, device='cuda', dtype=dtype)
    check(lib().ecgvit_head_bwd(ptr(dl), ptr(xhat), ptr(rstd), ptr(gd), ptr(bd), ptr(Wd), ptr(dW), ptr(dbias), ptr(dg), ptr(db), ptr(dX),
                                N, B, d, K, hip.code(dtype), stream()), 'head_bwd')
    tol = 1e-5 if dtype == F32 else 1e-2
    assert rel_err(dW, pr[2].grad) < tol and rel_err(dbias, pr[3].grad) < tol
    assert rel_err(dg, pr[0].grad) < tol and rel_err(db, pr[1].grad) < tol
    assert rel_err(dX, Xr.grad) < tol
    assert (dX.view(B, N, d)[:, 1:] == 0).all()


# ------------------------------------------------------------------------------------------------------ attention (bf16, fused)
def _attn_ref(qkv, B, N, h, dh, scale, mask=None):
    d = h * dh
    q, k, v = (qkv[:, i * d:(i + 1) * d].reshape(B, N, h, dh).permute(0, 2, 1, 3) for i in range(3))
    s = q @ k.transpose(-1, -2) * scale
    p = torch.softmax(s, -1)
    lse = torch.logsumexp(s, -1)
    pd = p if mask is None else p * mask
    o = (pd @ v).permute(0, 2, 1, 3).reshape(B * N, d)
    return o, lse, p


@pytest.mark.parametrize('N', [51, 251, 128, 256, 1, 33, 257, 300, 501, 512])
def test_attention_bf16_fwd_bwd(N):
    g = torch.Generator().manual_seed(N)
    B, h, dh = 2, 3, 64
    d = h * dh
    scale = dh ** -0.5
    qkv = (torch.randn(B * N, 3 * d, generator=g) * 1.5).to(BF16)
    qd = dev(qkv)
    out = torch.full((B * N, d), float('nan'), device='cuda', dtype=BF16)
    lse = torch.zeros(B * h * N, device='cuda')
    check(lib().ecgvit_attention_fwd(ptr(qd), ptr(out), ptr(lse), B, N, h, dh, scale, 0.0, 0, hip.BF16, stream()), 'attn_fwd')
    qr = qkv.double().requires_grad_(True)
    o_ref, lse_ref, _ = _attn_ref(qr, B, N, h, dh, scale)
    assert torch.isfinite(out.float()).all()
    assert max_err(out, o_ref) < 2e-2 and rel_err(out, o_ref) < 1e-2
    assert max_err(lse.view(B, h, N), lse_ref) < 2e-3
    do = torch.randn(B * N, d, generator=g).to(BF16)
    o_ref.backward(do.double())
    dqkv = torch.full((B * N, 3 * d), float('nan'), device='cuda', dtype=BF16)
    check(lib().ecgvit_attention_bwd(ptr(qd), ptr(out), ptr(dev(do)), ptr(lse), ptr(dqkv), B, N, h, dh, scale, 0.0, 0, hip.BF16, stream()),
          'attn_bwd')
    assert torch.isfinite(dqkv.float()).all()
    for i, nm in enumerate('qkv'):
        got, ref = dqkv[:, i * d:(i + 1) * d], qr.grad[:, i * d:(i + 1) * d]
        assert rel_err(got, ref) < 2e-2, (nm, rel_err(got, ref))


@pytest.mark.parametrize('B,h,N,p', [(171, 3, 251, 0.1), (100, 6, 251, 0.0), (33, 4, 130, 0.1), (9, 6, 64, 0.1), (5, 3, 1, 0.0), (60, 5, 501, 0.1), (70, 4, 300, 0.0),
                                     (52, 5, 257, 0.1), (64, 4, 512, 0.1), (43, 6, 449, 0.0), (7, 1, 251, 0.3), (3, 1, 501, 0.3), (40, 12, 200, 0.1)])
def test_attention_fwd_streamed_equals_one_item_kernel(B, h, N, p):
    """the STREAMED forward (round 6: one persistent 16-wave workgroup per CU, K / V windows through a two-slot LDS-DMA ring that runs across items, counted
    waits) against the one-(record, head)-per-workgroup forward on the same inputs, seed and dropout rate: output, LSE -- and with them the dropout mask --
    BIT-IDENTICAL (a window boundary changes no arithmetic of the online softmax); repeated launches identical (a ring race would show); odd item
    counts (the second wave group idles in the last pair), one or several items per workgroup, one / two windows per item, a one-key last window (257)"""
    tl = tools_lib()
    g = torch.Generator().manual_seed(B * 1000 + N)
    dh = 64
    d = h * dh
    qkv = dev((torch.randn(B * N, 3 * d, generator=g) * 1.3).to(BF16))
    res, res8 = {}, {}
    q8s = torch.full((1,), 0.004, device='cuda')
    try:
        for variant in (0, 1, 2):     # 0: one item per workgroup; 1: streamed, 16 waves (two items side by side up to 256 tokens); 2: streamed, 8 waves x 2 workgroups per CU (<= 256 tokens)
            tl.ecgvit_tools_attn_fwd_variant(variant)
            for rep in range(4 if variant else 1):
                out = torch.full((B * N, d), float('nan'), device='cuda', dtype=BF16)
                lse = torch.full((B * h * N,), float('nan'), device='cuda')
                check(tl.ecgvit_attention_fwd(ptr(qkv), ptr(out), ptr(lse), B, N, h, dh, dh ** -0.5, p, 4321, hip.BF16, stream()), 'attn_fwd')
                torch.cuda.synchronize()
                if rep == 0:
                    res[variant] = (out, lse)
                else:
                    assert torch.equal(out.view(torch.int16), res[variant][0].view(torch.int16)) and torch.equal(lse, res[variant][1]), rep
            # the 8-bit emitting entry point of the same form: same bf16 results, same e4m3 copy, same amax (the slot starts at zero, as inside a train step)
            out = torch.full((B * N, d), float('nan'), device='cuda', dtype=BF16)
            lse = torch.full((B * h * N,), float('nan'), device='cuda')
            o8 = torch.full((B * N, d), 0x7F, device='cuda', dtype=torch.uint8)
            am = torch.zeros(1, device='cuda')
            check(tl.ecgvit_attention_fwd_q8(ptr(qkv), ptr(out), ptr(lse), B, N, h, dh, dh ** -0.5, p, 4321, ptr(o8), ptr(q8s), ptr(am), stream()), 'attn_fwd_q8')
            torch.cuda.synchronize()
            res8[variant] = (out, lse, o8, am)
    finally:
        tl.ecgvit_tools_attn_fwd_variant(-1)
    assert torch.isfinite(res[1][0].float()).all() and torch.isfinite(res[1][1]).all()
    for variant in (1, 2):
        assert torch.equal(res[0][0].view(torch.int16), res[variant][0].view(torch.int16)), variant
        assert torch.equal(res[0][1], res[variant][1]), variant
    for variant in (0, 1, 2):
        o, l, o8, am = res8[variant]
        assert torch.equal(o.view(torch.int16), res[0][0].view(torch.int16)) and torch.equal(l, res[0][1]), variant
        assert torch.equal(o8, res8[0][2]) and float(am) == float(res[0][0].float().abs().max()), variant


def test_attention_fwd_product_dispatch_takes_the_streamed_kernel_at_full_occupancy():
    """the product library picks the streamed forward for records of more than 256 tokens once there is an item per CU: at 300 x 1 x 501 (and the
    one-item kernel at 600 x 1 x 251) it must agree with the double-precision reference like the small shapes above (maximum error over 10 M bf16
    outputs of magnitude ~1: 4e-2; relative error of the whole tensor as there)"""
    for B, h, N in ((600, 1, 251), (300, 1, 501), (257, 2, 449)):
        g = torch.Generator().manual_seed(N)
        qkv = (torch.randn(B * N, 3 * h * 64, generator=g) * 1.5).to(BF16)
        out = torch.full((B * N, h * 64), float('nan'), device='cuda', dtype=BF16)
        lse = torch.zeros(B * h * N, device='cuda')
        check(lib().ecgvit_attention_fwd(ptr(dev(qkv)), ptr(out), ptr(lse), B, N, h, 64, 0.125, 0.0, 0, hip.BF16, stream()), 'attn_fwd')
        o_ref, lse_ref, _ = _attn_ref(qkv.double(), B, N, h, 64, 0.125)
        assert torch.isfinite(out.float()).all()
        assert max_err(out, o_ref) < 4e-2 and rel_err(out, o_ref) < 1e-2 and max_err(lse.view(B, h, N), lse_ref) < 2e-3


@pytest.mark.parametrize('N', [251, 501])
@pytest.mark.parametrize('shape', ['rising', 'falling', 'spike'])
def test_attention_fwd_lazy_running_maximum(N, shape):
    """the forward keeps a LAZY running maximum: a query's reference moves only when a key tile exceeds it by more than 2^8 in the exponent.  Peaked score
    profiles take every path of that rule -- keys whose scores RISE tile after tile (the reference is moved again and again), FALL (it never moves after the
    first tile and later tiles underflow towards zero), and one SPIKE key deep in the row (one move of hundreds of exponent units) -- against the fp64 softmax;
    the backward, which rebuilds the probabilities from the stored LSE, against autograd"""
    g = torch.Generator().manual_seed(N)
    B, h, dh = 2, 3, 64
    d = h * dh
    scale = dh ** -0.5
    x = torch.randn(B, N, 3, h, dh, generator=g)
    ramp = torch.linspace(0.2, 6.0, N).view(1, N, 1, 1)
    if shape == 'rising':
        x[:, :, 1] *= ramp            # |k| grows with the key index: the row maximum keeps moving up
    elif shape == 'falling':
        x[:, :, 1] *= ramp.flip(1)
    else:
        x[:, N - 40, 1] *= 25.0       # one key with scores in the hundreds, in the last tiles
    qkv = x.reshape(B * N, 3 * d).to(BF16)
    qd = dev(qkv)
    out = torch.full((B * N, d), float('nan'), device='cuda', dtype=BF16)
    lse = torch.zeros(B * h * N, device='cuda')
    check(lib().ecgvit_attention_fwd(ptr(qd), ptr(out), ptr(lse), B, N, h, dh, scale, 0.0, 0, hip.BF16, stream()), 'attn_fwd')
    qr = qkv.double().requires_grad_(True)
    o_ref, lse_ref, _ = _attn_ref(qr, B, N, h, dh, scale)
    assert torch.isfinite(out.float()).all() and torch.isfinite(lse).all()
    assert rel_err(out, o_ref) < 1e-2, rel_err(out, o_ref)
    assert max_err(lse.view(B, h, N), lse_ref) < 2e-3 * max(1.0, float(lse_ref.abs().max()) / 50)     # f32 LSE: absolute error grows with its magnitude
    do = torch.randn(B * N, d, generator=g).to(BF16)
    o_ref.backward(do.double())
    dqkv = torch.full((B * N, 3 * d), float('nan'), device='cuda', dtype=BF16)
    check(lib().ecgvit_attention_bwd(ptr(qd), ptr(out), ptr(dev(do)), ptr(lse), ptr(dqkv), B, N, h, dh, scale, 0.0, 0, hip.BF16, stream()), 'attn_bwd')
    assert torch.isfinite(dqkv.float()).all()
    for i, nm in enumerate('qkv'):
        got, ref = dqkv[:, i * d:(i + 1) * d], qr.grad[:, i * d:(i + 1) * d]
        assert rel_err(got, ref) < 3e-2, (nm, rel_err(got, ref))


@pytest.mark.parametrize('N', [501, 257, 300, 512, 449])
def test_attention_bf16_long_forward_501(N):
    """forward covers N <= 512 (seq = 500 patches + CLS, the 'large' long-record geometry).  Above 256 tokens a workgroup owns one 256-query half
    and the keys pass through the LDS images in two 256-key windows: 257 = a second window of ONE key and seven idle waves in the second query
    half, 300 / 449 = partial last window and partially idle second half, 512 = both full."""
    g = torch.Generator().manual_seed(N)
    B, h, dh = 2, 3, 64
    d = h * dh
    qkv = torch.randn(B * N, 3 * d, generator=g).to(BF16)
    out = torch.full((B * N, d), float('nan'), device='cuda', dtype=BF16)
    lse = torch.zeros(B * h * N, device='cuda')
    check(lib().ecgvit_attention_fwd(ptr(dev(qkv)), ptr(out), ptr(lse), B, N, h, dh, dh ** -0.5, 0.0, 0, hip.BF16, stream()), 'attn_fwd')
    o_ref, lse_ref, _ = _attn_ref(qkv.double(), B, N, h, dh, dh ** -0.5)
    assert torch.isfinite(out.float()).all()
    assert rel_err(out, o_ref) < 1e-2 and max_err(lse.view(B, h, N), lse_ref) < 2e-3


def test_attention_bf16_dropout_mask_consistent_fwd_bwd():
    """V = identity exposes the dropped probabilities as the output; backward must use the same mask"""
    B, h, dh, N = 1, 1, 64, 64
    p, seed = 0.3, 99
    g = torch.Generator().manual_seed(1)
    qkv = torch.zeros(N, 3 * dh)
    qkv[:, :2 * dh] = torch.randn(N, 2 * dh, generator=g) * 0.5
    qkv[:, 2 * dh:] = torch.eye(N)
    qkv = qkv.to(BF16)
    out = torch.zeros(N, dh, device='cuda', dtype=BF16)
    lse = torch.zeros(N, device='cuda')
    check(lib().ecgvit_attention_fwd(ptr(dev(qkv)), ptr(out), ptr(lse), B, N, h, dh, 0.125, p, seed, hip.BF16, stream()), 'attn_fwd')
    o = out.float().cpu()
    mask = (o != 0).double()
    keep = mask.mean().item()
    assert abs(keep - (1 - p)) < 0.03
    qr = qkv.double().requires_grad_(True)
    o_ref, _, P = _attn_ref(qr, B, N, h, dh, 0.125, mask=(mask / (1 - p)).view(1, 1, N, N))
    assert rel_err(out, o_ref) < 1e-2
    do = torch.randn(N, dh, generator=g).to(BF16)
    o_ref.backward(do.double())
    dqkv = torch.zeros(N, 3 * dh, device='cuda', dtype=BF16)
    check(lib().ecgvit_attention_bwd(ptr(dev(qkv)), ptr(out), ptr(dev(do)), ptr(lse), ptr(dqkv), B, N, h, dh, 0.125, p, seed, hip.BF16,
                                     stream()), 'attn_bwd')
    assert rel_err(dqkv, qr.grad) < 3e-2


def test_attention_dropout_mask_statistics():
    """the attention-probability mask (one hash per 4 consecutive keys, 8 bits each): V = identity exposes it.  Keep rate = the
    quantised probability 1 - round(256 p)/256 to sampling error; keys inside one hash word, neighbouring words, neighbouring queries
    and different seeds are uncorrelated (< 5e-3 on 1 M elements); a rerun reproduces it bit for bit"""
    B, h, dh, N = 64, 4, 64, 64
    g = torch.Generator().manual_seed(2)
    qkv = torch.zeros(B * N, 3 * h * dh)
    for hd in range(h):
        qkv[:, 2 * h * dh + hd * dh:2 * h * dh + (hd + 1) * dh] = torch.eye(N).repeat(B, 1)      # V = I per head; Q = K = 0: uniform P
    qd = dev(qkv.to(BF16))
    masks = {}
    for p, seed in ((0.1, 7), (0.1, 8), (0.3, 7)):
        out = torch.zeros(B * N, h * dh, device='cuda', dtype=BF16)
        lse = torch.zeros(B * h * N, device='cuda')
        for rep in range(2):
            check(lib().ecgvit_attention_fwd(ptr(qd), ptr(out), ptr(lse), B, N, h, dh, 0.125, p, seed, hip.BF16, stream()), 'attn_fwd')
            m = (out.float() != 0).view(B, N, h, N).permute(0, 2, 1, 3).contiguous()              # [b, head, query, key]
            if rep == 0:
                masks[(p, seed)] = m
            else:
                assert torch.equal(m, masks[(p, seed)])
        keep = m.double().mean().item()
        want = 1.0 - round(256 * p) / 256.0
        assert abs(keep - want) < 2e-3, (p, keep, want)
        kept = out.float()[out.float() != 0]
        assert abs(kept.mean().item() * N - 1.0 / want) < 2e-2 / want          # kept probabilities are scaled by exactly 1 / keep-rate
    m = masks[(0.1, 7)].double()

    def corr(a, b):
        a, b = a.flatten() - a.mean(), b.flatten() - b.mean()
        return abs(float((a * b).mean() / (a.std() * b.std())))
    assert corr(m[..., 0::2], m[..., 1::2]) < 5e-3            # keys 2j, 2j+1: same hash word
    assert corr(m[..., 0::4], m[..., 3::4]) < 5e-3            # first / last byte of a word
    assert corr(m[..., 3:-4:4], m[..., 4::4][..., :m[..., 3:-4:4].shape[-1]]) < 5e-3   # neighbouring words
    assert corr(m[:, :, :-1], m[:, :, 1:]) < 5e-3             # neighbouring queries
    assert corr(m[:, :-1], m[:, 1:]) < 5e-3                   # neighbouring heads
    assert corr(m, masks[(0.1, 8)].double()) < 5e-3           # another seed


# ------------------------------------------------------------------------------------------------------ optimiser
def test_sumsq_clip_adamw_match_torch():
    g = torch.Generator().manual_seed(21)
    n = 100003
    p0 = torch.randn(n, generator=g)
    pt = torch.nn.Parameter(p0.clone())
    opt = torch.optim.AdamW([pt], lr=1e-2, weight_decay=0.1)
    p, m, v = dev(p0.clone()), torch.zeros(n, device='cuda'), torch.zeros(n, device='cuda')
    plow = torch.zeros(n, device='cuda', dtype=BF16)
    ws = torch.empty(lib().ecgvit_sumsq_workspace(n), dtype=torch.uint8, device='cuda')
    ss, no = torch.zeros(1, device='cuda'), torch.zeros(2, device='cuda')
    for step in range(1, 4):
        gr = torch.randn(n, generator=g) * (0.01 if step == 2 else 1.0)  # step 2: norm < 1, no clipping
        pt.grad = gr.clone()
        tn = torch.nn.utils.clip_grad_norm_([pt], 1.0, error_if_nonfinite=True)
        opt.step()
        gd = dev(gr)
        check(lib().ecgvit_sumsq(ptr(gd), n, ptr(ss), ptr(ws), stream()), 'sumsq')
        assert abs(float(ss) - float(gr.double().pow(2).sum())) / float(gr.double().pow(2).sum()) < 1e-5
        check(lib().ecgvit_adamw_step(ptr(p), ptr(gd), ptr(m), ptr(v), ptr(plow), n, ptr(ss), 1.0, 1.0, 1e-2, 0.9, 0.999, 1e-8, 0.1, step, 1,
                                      ptr(no), stream()), 'adamw')
        assert abs(float(no[0]) - float(tn)) / float(tn) < 1e-5 and float(no[1]) == 1.0
        assert max_err(p, pt.detach()) < 2e-6
        assert torch.equal(plow.cpu(), p.cpu().to(BF16))
    # non-finite gradient: flagged, nothing updated
    gd = dev(torch.full((n,), float('nan')))
    before = p.clone()
    check(lib().ecgvit_sumsq(ptr(gd), n, ptr(ss), ptr(ws), stream()), 'sumsq')
    check(lib().ecgvit_adamw_step(ptr(p), ptr(gd), ptr(m), ptr(v), None, n, ptr(ss), 1.0, 1.0, 1e-2, 0.9, 0.999, 1e-8, 0.1, 4, 1, ptr(no),
                                  stream()), 'adamw')
    assert float(no[1]) == 0.0 and torch.equal(p, before)
    # Adam (coupled weight decay) variant + stand-alone clip
    q0 = torch.randn(1000, generator=g)
    qt = torch.nn.Parameter(q0.clone())
    opt2 = torch.optim.Adam([qt], lr=1e-2, weight_decay=0.1)
    gr = torch.randn(1000, generator=g)
    qt.grad = gr.clone()
    opt2.step()
    q, m2, v2 = dev(q0.clone()), torch.zeros(1000, device='cuda'), torch.zeros(1000, device='cuda')
    gd = dev(gr)
    check(lib().ecgvit_sumsq(ptr(gd), 1000, ptr(ss), ptr(ws), stream()), 'sumsq')
    check(lib().ecgvit_adamw_step(ptr(q), ptr(gd), ptr(m2), ptr(v2), None, 1000, ptr(ss), 1.0, 0.0, 1e-2, 0.9, 0.999, 1e-8, 0.1, 1, 0, ptr(no),
                                  stream()), 'adam')
    assert max_err(q, qt.detach()) < 2e-6
    check(lib().ecgvit_clip_scale(ptr(gd), 1000, ptr(ss), 1.0, ptr(no), stream()), 'clip')
    assert rel_err(gd, gr / (gr.norm() + 1e-6)) < 1e-5


def test_casts_roundtrip():
    x = torch.randn(10007)
    b = torch.zeros(10007, device='cuda', dtype=BF16)
    check(lib().ecgvit_cast_f32_to_bf16(ptr(dev(x)), ptr(b), 10007, stream()), 'cast')
    assert torch.equal(b.cpu(), x.to(BF16))
    f = torch.zeros(10007, device='cuda')
    check(lib().ecgvit_cast_bf16_to_f32(ptr(b), ptr(f), 10007, stream()), 'cast')
    assert torch.equal(f.cpu(), x.to(BF16).float())


# ------------------------------------------------------------------------------------------------------ masked-objective ops
@pytest.mark.parametrize('dtype', [F32, BF16])
def test_masked_objective_ops(dtype):
    g = torch.Generator().manual_seed(31)
    B, n, m, d = 4, 25, 12, 64
    tok = torch.randn(B * n, d, generator=g).to(dtype)
    mt, pos = torch.randn(d, generator=g), torch.randn(n + 1, d, generator=g)
    idx = torch.stack([torch.randperm(n, generator=g)[:m] for _ in range(B)]).int()
    X = torch.zeros(B * n, d, device='cuda', dtype=dtype)
    flag = torch.zeros(B * n, dtype=torch.uint8, device='cuda')
    check(lib().ecgvit_mask_embed_finish(ptr(dev(tok)), ptr(dev(mt)), ptr(dev(pos)), ptr(dev(idx)), ptr(X), ptr(flag), B, n, m, d,
                                         hip.code(dtype), stream()), 'mask_embed')
    t = tok.float().view(B, n, d).clone()
    for b in range(B):
        t[b, idx[b].long()] = mt
    ref = (t + pos[1:]).view(B * n, d)
    assert rel_err(X, ref) < (1e-6 if dtype == F32 else 4e-3)
    # bit-exact integer index handling: which rows were replaced
    is_masked = torch.zeros(B, n, dtype=torch.bool)
    is_masked.scatter_(1, idx.long(), True)
    assert torch.equal(flag.cpu().view(B, n).bool(), is_masked)
    out = torch.zeros(B * m, d, device='cuda', dtype=dtype)
    check(lib().ecgvit_gather_rows(ptr(X), ptr(dev(idx)), ptr(out), B, n, m, d, d, d, hip.code(dtype), stream()), 'gather')
    bi = torch.arange(B).unsqueeze(-1)
    assert torch.equal(out.cpu().view(B, m, d), X.cpu().view(B, n, d)[bi, idx.long()])
    back = torch.zeros(B * n, d, device='cuda', dtype=dtype)
    check(lib().ecgvit_scatter_rows(ptr(out), ptr(dev(idx)), ptr(back), B, n, m, d, d, d, hip.code(dtype), stream()), 'scatter')
    exp = torch.zeros(B, n, d, dtype=dtype)
    exp[bi, idx.long()] = X.cpu().view(B, n, d)[bi, idx.long()]
    assert torch.equal(back.cpu().view(B, n, d), exp)
    pred, tgt = torch.randn(B * m, d, generator=g).to(dtype), torch.randn(B * m, d, generator=g).to(dtype)
    loss, dpred = torch.zeros(1, device='cuda'), torch.zeros(B * m, d, device='cuda', dtype=dtype)
    l1part = torch.empty(1024, device='cuda')
    check(lib().ecgvit_l1_loss_fwd_bwd(ptr(dev(pred)), ptr(dev(tgt)), ptr(loss), ptr(dpred), None, ptr(l1part), B * m, d, d, hip.code(dtype), stream()), 'l1')
    diff = pred.double() - tgt.double()
    assert abs(float(loss) - float(diff.abs().mean())) < 1e-5
    assert rel_err(dpred, torch.sign(diff) / diff.numel()) < (1e-6 if dtype == F32 else 4e-3)


# ------------------------------------------------------------------------------------------------------ large-shape GEMM variant
@pytest.mark.parametrize('layout,shape', [
    (hip.GEMM_NT, (4133, 768, 768)), (hip.GEMM_NT, (2048, 264, 240)), (hip.GEMM_NT, (2500, 3072, 768)),
    (hip.GEMM_NT, (40000, 768, 192)), (hip.GEMM_NT, (33001, 520, 256)), (hip.GEMM_NT, (70000, 1032, 448)),   # > 256 tiles: persistent walk
    (hip.GEMM_NN, (4133, 768, 2304)), (hip.GEMM_NN, (2051, 520, 768)),
    (hip.GEMM_TN, (768, 3072, 9001)), (hip.GEMM_TN, (2304, 768, 4099)), (hip.GEMM_TN, (768, 240, 5000)),
])
def test_gemm_bf16_large_shapes(layout, shape):
    """shapes that dispatch to the 256x256 LDS-DMA kernel (gemm_bf16_v2.hip): ragged M, N and K tails, split-K wgrad"""
    M, N, K = shape
    g = torch.Generator().manual_seed(M + N + K)
    A, B = _operands(layout, M, N, K, BF16, g)
    ref = _gemm_ref(layout, A.float(), B.float())
    if layout == hip.GEMM_TN:
        ws = torch.empty(max(16, hip.gemm_workspace_bytes(layout, BF16, M, N, K)), dtype=torch.uint8, device='cuda')
        C = torch.full((M, N), float('nan'), device='cuda')
        hip.gemm(layout, dev(A), dev(B), C, M, N, K, A.shape[1], B.shape[1], N, workspace=ws)
        assert rel_err(C, ref) < 2e-5
    else:
        C = torch.full((M, N), float('nan'), device='cuda', dtype=BF16)
        bias = torch.randn(N, generator=g)
        res = torch.randn(M, N, generator=g).to(BF16)
        hip.gemm(layout, dev(A), dev(B), C, M, N, K, A.shape[1], B.shape[1], N, epilogue=hip.EPI_BIAS | hip.EPI_RESIDUAL, bias=dev(bias),
                 residual=dev(res), ldr=N)
        assert torch.isfinite(C.float()).all()
        assert rel_err(C, ref + bias.double() + res.double()) < 4e-3


def test_gemm_bf16_chunked_dispatch_equals_persistent():
    """`tiles_per_workgroup` (dispatcher-balanced chunks for launches that share the GPU with collectives) changes only which workgroup
    computes a tile: outputs, saved aux and fused column sums are bit-identical to the persistent launch, ragged M / N included"""
    g = torch.Generator().manual_seed(11)
    M, N, K = 70011, 776, 256
    A = torch.randn(M, K, generator=g).to(BF16).cuda()
    B = (torch.randn(N, K, generator=g) * 0.1).to(BF16).cuda()
    bias = torch.randn(N, generator=g).cuda()
    aux = torch.rand(M, N, generator=g).to(BF16).cuda()
    ws = torch.empty(64 << 20, dtype=torch.uint8, device='cuda')
    outs = []
    for tpw in (0, 1, 2, 5):
        C = torch.full((M, N), float('nan'), device='cuda', dtype=BF16)
        C2 = torch.full((M, N), float('nan'), device='cuda', dtype=BF16)
        cs = torch.zeros(N, device='cuda')
        hip.gemm(hip.GEMM_NT, A, B, C, M, N, K, K, K, N, epilogue=hip.EPI_BIAS | hip.EPI_DROPOUT, bias=bias, dropout_p=0.1, seed=5, tiles_per_workgroup=tpw)
        hip.gemm(hip.GEMM_NT, A, B, C2, M, N, K, K, K, N, epilogue=hip.EPI_MUL_AUX | hip.EPI_COLSUM, aux=aux, ldaux=N, workspace=ws, colsum_out=cs,
                 tiles_per_workgroup=tpw)
        outs.append((C, C2, cs))
    for C, C2, cs in outs[1:]:
        assert torch.equal(C, outs[0][0]) and torch.equal(C2, outs[0][1]) and torch.equal(cs, outs[0][2])
    assert torch.isfinite(outs[0][0].float()).all() and rel_err(outs[0][2], outs[0][1].float().sum(0)) < 1e-5


def test_gemm_bf16_persistent_forward_is_race_free_and_exact():
    """the quadrant-phased persistent forward kernel (continuous operand stream across output tiles, counted waits): small-integer
    operands make every product and sum exact in f32, so the result must EQUAL the integer reference bit for bit, on every one of
    many repeated launches (a DMA/ds_read race shows up as a sporadically wrong tile), f32 and bf16 outputs, ragged M and N"""
    g = torch.Generator().manual_seed(5)
    for (M, N, K) in ((66000, 776, 192), (30011, 2304, 768), (9000, 768, 3072)):
        A = torch.randint(-3, 4, (M, K), generator=g).float()
        B = torch.randint(-3, 4, (N, K), generator=g).float()
        Ad, Bd = A.to(BF16).cuda(), B.to(BF16).cuda()
        ref = (Ad.float() @ Bd.float().t())                     # exact: |sum| <= 9 * 3072 < 2^24
        C = torch.empty(M, N, device='cuda')
        for rep in range(12):
            C.fill_(float('nan'))
            hip.gemm(hip.GEMM_NT, Ad, Bd, C, M, N, K, K, K, N)
            assert torch.equal(C, ref), (M, N, K, rep, int((C != ref).sum()))
        Cb = torch.empty(M, N, device='cuda', dtype=BF16)
        hip.gemm(hip.GEMM_NT, Ad, Bd, Cb, M, N, K, K, K, N)
        assert torch.equal(Cb, ref.to(BF16))


def test_gemm_bf16_four_wave_body_is_race_free_exact_and_equal_to_the_eight_wave_body():
    """plain bf16 products with K >= 1536 (and the residual launches with K >= 768) run on gemm_nt_kernel_4w (one wave per SIMD, 128 x 128 per wave, fixed-order k-steps); outputs of
    more than 256 MB are stored non-temporally (either body).  Small-integer operands make the result exact: it must EQUAL the integer
    reference on every repeated launch (ragged M and N, one to many tiles per workgroup, K-tile counts 12 to 48), persistent and as
    dispatcher-balanced chunks; the f32-output launch of the same product -- which runs on the eight-wave body -- rounds to the same bits."""
    g = torch.Generator().manual_seed(9)
    for (M, N, K) in ((66001, 776, 1536), (9000, 768, 3072), (2259, 2304, 2304), (60011, 2304, 1536), (60011, 2304, 768)):
        A = torch.randint(-3, 4, (M, K), generator=g).float()
        B = torch.randint(-3, 4, (N, K), generator=g).float()
        Ad, Bd = A.to(BF16).cuda(), B.to(BF16).cuda()
        ref = (Ad.float() @ Bd.float().t()).to(BF16)            # exact before the bf16 rounding: |sum| <= 9 * 3072 < 2^24
        assert hip.gemm_kernel(hip.GEMM_NT, Ad, Bd, ref, M, N, K, K, K, N) == hip.KERNEL_GEMM_NT
        C = torch.empty(M, N, device='cuda', dtype=BF16)
        for rep in range(6):
            C.fill_(float('nan'))
            hip.gemm(hip.GEMM_NT, Ad, Bd, C, M, N, K, K, K, N)
            assert torch.equal(C, ref), (M, N, K, rep, int((C != ref).sum()))
        C.fill_(float('nan'))
        hip.gemm(hip.GEMM_NT, Ad, Bd, C, M, N, K, K, K, N, tiles_per_workgroup=2)
        assert torch.equal(C, ref), (M, N, K, 'chunked')
        C32 = torch.full((M, N), float('nan'), device='cuda')
        hip.gemm(hip.GEMM_NT, Ad, Bd, C32, M, N, K, K, K, N)      # f32 output: eight-wave body
        assert torch.equal(C32.to(BF16), ref), (M, N, K, 'eight-wave body, f32 output')
        del C32
    # random operands: the two bodies accumulate in the same order -- the f32 result of the eight-wave body rounds to the four-wave body's bits
    M, N, K = 20000, 1000, 2304
    Ad = torch.randn(M, K, generator=g).to(BF16).cuda()
    Bd = (torch.randn(N, K, generator=g) * 0.05).to(BF16).cuda()
    C4, C8 = torch.empty(M, N, device='cuda', dtype=BF16), torch.empty(M, N, device='cuda', dtype=BF16)
    C8f = torch.empty(M, N, device='cuda')
    hip.gemm(hip.GEMM_NT, Ad, Bd, C4, M, N, K, K, K, N)
    hip.gemm(hip.GEMM_NT, Ad, Bd, C8, M, N, K, K, K, N, tiles_per_workgroup=3)
    hip.gemm(hip.GEMM_NT, Ad, Bd, C8f, M, N, K, K, K, N)
    assert torch.equal(C4, C8) and torch.equal(C4, C8f.to(BF16))
    assert rel_err(C4, Ad.double() @ Bd.double().t()) < 4e-3     # bf16 output rounding
    # the residual launches (bias + residual [+ dropout], K >= 768) take the four-wave body too: persistent and chunked launches agree bit for bit
    for (M, N, K, epi) in ((30011, 776, 768, hip.EPI_BIAS | hip.EPI_RESIDUAL | hip.EPI_DROPOUT), (9000, 768, 3072, hip.EPI_BIAS | hip.EPI_RESIDUAL)):
        Ad = torch.randn(M, K, generator=g).to(BF16).cuda()
        Bd = (torch.randn(N, K, generator=g) * 0.05).to(BF16).cuda()
        bias, res = torch.randn(N, generator=g).cuda(), torch.randn(M, N, generator=g).to(BF16).cuda()
        outs = []
        for tpw in (0, 2):
            C = torch.full((M, N), float('nan'), device='cuda', dtype=BF16)
            hip.gemm(hip.GEMM_NT, Ad, Bd, C, M, N, K, K, K, N, epilogue=epi, bias=bias, residual=res, ldr=N, dropout_p=0.1 if epi & hip.EPI_DROPOUT else 0.0,
                     seed=11, tiles_per_workgroup=tpw)
            outs.append(C)
        assert torch.equal(outs[0], outs[1]) and torch.isfinite(outs[0].float()).all()
        if not epi & hip.EPI_DROPOUT:
            assert rel_err(outs[0], Ad.double() @ Bd.double().t() + bias.double() + res.double()) < 4e-3


# ------------------------------------------------------------------------------------------------------ f1: evaluation metrics
def _metrics_golden():
    import json
    import os
    with open(os.path.join(os.path.dirname(__file__), 'golden', 'metrics.json')) as f:
        return json.load(f)


def test_eval_counts_bit_exact_and_get_accuracy_matches_reference():
    import ecg_representation_learning_amd as E
    from oracle.metrics_oracle import eval_counts_np
    g = _metrics_golden()
    for name, case in g['cases'].items():
        probs, labels = np.asarray(case['probs'], np.float32), np.asarray(case['labels'], np.float32)
        h = E.eval_counts(torch.from_numpy(probs).cuda(), torch.from_numpy(labels).cuda(), id2code=g['id2code'])
        np.testing.assert_array_equal(h.counts.cpu().numpy(), eval_counts_np(probs, labels), err_msg=name)   # integers: bit-exact
        got, want = h.result(), case['expect']
        for k, v in want.items():
            if v is None:
                assert got[k] is None, (name, k)
            elif isinstance(v, dict):
                assert list(got[k]) == list(v)
                assert max(abs(got[k][c] - a) for c, a in v.items()) < 1e-12, name
            else:
                assert abs(got[k] - v) < 1e-12, (name, k)
        no_auc = E.get_accuracy(torch.from_numpy(probs).cuda(), torch.from_numpy(labels).cuda(), return_auc=False)
        assert no_auc['macro_auc'] is None and no_auc['per_class_auc'] is None and no_auc['binary_accuracy'] == got['binary_accuracy']


def test_eval_counts_eval_set_size_rank_identity():
    """whole-eval-set size (PTB-XL test fold ~ 2.2k; here 20k x 71, ragged vs the 256 / 2048 tiles): the pair counts must equal the
    Mann-Whitney statistic from average ranks (O(B log B) on the host), and logits input == probabilities input"""
    import ecg_representation_learning_amd as E
    from scipy.stats import rankdata
    rng = np.random.default_rng(3)
    B, K = 20011, 71
    prior = np.concatenate([np.full(8, 0.3), np.full(23, 0.05), np.full(40, 0.002)])
    lb = (rng.random((B, K)) < prior).astype(np.float32)
    logit = (rng.standard_normal((B, K)) + 1.5 * lb - 2).astype(np.float32)
    logit = np.round(logit * 64) / 64                                  # ties
    prob = torch.sigmoid(torch.from_numpy(logit).cuda())
    h = E.eval_counts(prob, torch.from_numpy(lb).cuda())
    cnt = h.counts.cpu().numpy()
    p = prob.cpu().numpy()
    for c in range(K):
        y = lb[:, c] != 0
        P, N = int(y.sum()), int((~y).sum())
        assert cnt[4 + c] == P
        r = rankdata(p[:, c])                                            # average ranks, halves exact in f64
        u2 = int(round(2 * (r[y].sum() - P * (P + 1) / 2)))
        assert cnt[4 + K + c] == u2, c
    pred, yy = p >= 0.5, lb != 0
    assert cnt[0] == (pred & yy).sum() and cnt[1] == (~pred & ~yy).sum() and cnt[2] == (pred & ~yy).sum() and cnt[3] == (~pred & yy).sum()
    h2 = E.eval_counts(torch.from_numpy(logit).cuda(), torch.from_numpy(lb).cuda(), from_logits=True)
    c2 = h2.counts.cpu().numpy()
    np.testing.assert_array_equal(c2[:4 + K], cnt[:4 + K])
    # in-kernel f32 sigmoid vs torch's: tie structure of saturated values may differ by a few pairs at most
    assert np.max(np.abs(c2[4 + K:] - cnt[4 + K:]) / np.maximum(cnt[4 + K:], 1)) < 1e-5


def test_transpose_bf16_batched():
    """transposed shadow weights: several matrices at their offsets in one flat buffer, interior and ragged tiles, untouched gaps"""
    g = torch.Generator().manual_seed(4)
    shapes = [(768, 2304), (64, 64), (200, 72), (3072, 768), (8, 8)]
    offs, table, t, total = [], [], 0, 16
    for r, c in shapes:
        offs.append(total)
        table.append([total, r, c, t])
        t += ((r + 63) // 64) * ((c + 63) // 64)
        total += r * c + 24                                           # gaps (other parameters) must stay untouched
    src = torch.randn(total, generator=g).to(BF16).cuda()
    dst = torch.full((total,), 7.0, dtype=BF16, device='cuda')
    tb = torch.tensor(table, dtype=torch.int64, device='cuda')
    check(lib().ecgvit_transpose_bf16_batched(ptr(src), ptr(dst), ptr(tb), len(shapes), t, stream()), 'transpose')
    expect = torch.full((total,), 7.0, dtype=BF16)
    for (r, c), o in zip(shapes, offs):
        expect[o:o + r * c] = src[o:o + r * c].cpu().view(r, c).t().contiguous().view(-1)
    assert torch.equal(dst.cpu(), expect)


@pytest.mark.parametrize('shape', [(260, 136, 128), (4100, 520, 256)])    # 128^2 kernel / persistent 256^2 kernel
def test_gemm_bf16_saved_gelu_grad_and_mul_aux(shape):
    """EPI_GELU_GRAD_AUX: C = [dropout](gelu(pre)), aux = gelu'(pre) * dropout multiplier; EPI_MUL_AUX: C = acc * aux.
    Together they are forward and backward of `dropout(gelu(Linear))` with the mask hashed once."""
    M, N, K = shape
    g = torch.Generator().manual_seed(M)
    A, B = _operands(hip.GEMM_NT, M, N, K, BF16, g)
    bias = torch.randn(N, generator=g)
    pre = _gemm_ref(hip.GEMM_NT, A.float(), B.float()) + bias.double()
    C = torch.zeros(M, N, device='cuda', dtype=BF16)
    aux = torch.zeros(M, N, device='cuda', dtype=BF16)
    Ad, Bd, bd = dev(A), dev(B), dev(bias)
    hip.gemm(hip.GEMM_NT, Ad, Bd, C, M, N, K, K, K, N, epilogue=hip.EPI_BIAS | hip.EPI_GELU | hip.EPI_GELU_GRAD_AUX, bias=bd, aux=aux, ldaux=N)
    assert rel_err(C, gelu(pre)) < 4e-3 and rel_err(aux, gelu_grad(pre)) < 4e-3
    # with dropout: the kept set of C and aux is the same, both scaled by 1/(1-p); identical to the plain-dropout epilogue's mask
    p = 0.25
    C2, aux2, C3 = torch.zeros_like(C), torch.zeros_like(aux), torch.zeros_like(C)
    kw = dict(bias=bd, dropout_p=p, seed=99)
    hip.gemm(hip.GEMM_NT, Ad, Bd, C2, M, N, K, K, K, N, epilogue=hip.EPI_BIAS | hip.EPI_GELU | hip.EPI_GELU_GRAD_AUX | hip.EPI_DROPOUT, aux=aux2, ldaux=N, **kw)
    hip.gemm(hip.GEMM_NT, Ad, Bd, C3, M, N, K, K, K, N, epilogue=hip.EPI_BIAS | hip.EPI_DROPOUT, **kw)
    keep = (C3 != 0).cpu()
    assert abs(float(keep.float().mean()) - (1 - p)) < 0.01
    assert rel_err(C2, gelu(pre) * keep / (1 - p)) < 4e-3
    assert rel_err(aux2, gelu_grad(pre) * keep / (1 - p)) < 4e-3
    # backward multiply
    dY, W = _operands(hip.GEMM_NT, M, N, K, BF16, g)
    D = torch.zeros(M, N, device='cuda', dtype=BF16)
    hip.gemm(hip.GEMM_NT, dev(dY), dev(W), D, M, N, K, K, K, N, epilogue=hip.EPI_MUL_AUX, aux=aux2, ldaux=N)
    assert rel_err(D, _gemm_ref(hip.GEMM_NT, dY.float(), W.float()) * aux2.float().double().cpu()) < 4e-3


def test_dropout_mask_statistics():
    """the f32 parity path's counter-based mask (one Weyl step + one xorshift-multiply round per pair of elements, exact p): keep rate, independence of neighbours
    along a row, across rows and across seeds -- on 4M elements the standard error of a correlation is 5e-4"""
    rows, d = 4096, 1024
    ones = torch.ones(rows * d, device='cuda')
    masks = []
    for p, seed in ((0.1, 1), (0.1, 2), (0.5, 123456789012345), (0.25, 7)):
        out = torch.empty_like(ones)
        check(lib().ecgvit_dropout_apply(ptr(ones), ptr(out), rows * d, p, seed, hip.F32, stream()), 'dropout_apply')
        keep = (out != 0).float().view(rows, d)
        assert abs(float(keep.mean()) - (1 - p)) < 2e-3, (p, float(keep.mean()))
        assert torch.allclose(out[out != 0], torch.tensor(1.0 / (1 - p), device='cuda'))
        z = keep - keep.mean()
        var = float((z * z).mean())

        def corr(a, b):
            return float((a * b).mean()) / var
        assert abs(corr(z[:, :-1], z[:, 1:])) < 4e-3            # neighbours (half of them share a hash: the two 16-bit halves)
        assert abs(corr(z[:, :-2], z[:, 2:])) < 4e-3            # next pair (one Weyl step apart)
        assert abs(corr(z[:-1, :], z[1:, :])) < 4e-3            # next row (d/2 Weyl steps apart)
        assert abs(corr(z[:, :-64], z[:, 64:])) < 4e-3
        colmean, rowmean = keep.mean(0), keep.mean(1)             # no column or row is systematically kept / dropped
        assert float((colmean - (1 - p)).abs().max()) < 5 * (p * (1 - p) / rows) ** 0.5 + 1e-3
        assert float((rowmean - (1 - p)).abs().max()) < 5 * (p * (1 - p) / d) ** 0.5 + 1e-3
        masks.append(keep)
    z0, z1 = masks[0] - masks[0].mean(), masks[1] - masks[1].mean()
    assert abs(float((z0 * z1).mean()) / float((z0 * z0).mean())) < 4e-3   # seeds 1 and 2: unrelated masks


def test_dropout_mask_statistics_bf16_quad_form():
    """the 16-bit sites' mask (round 5): one hash per FOUR consecutive elements, 8 bits each, keep iff byte >= round(256 p), exact rescale of the rate
    actually applied.  Keep rate, value of the kept elements, independence inside a quad (bytes of one hash), across quads, rows and seeds;
    thresholds on both sides of 128 (the bit-parallel compare has two forms) and the smallest one; 0 < p < 1/512 is an error, not "no dropout"."""
    rows, d = 4096, 1024
    ones = torch.ones(rows * d, device='cuda', dtype=BF16)
    masks = []
    for p, seed in ((0.1, 1), (0.1, 2), (0.5, 123456789012345), (0.75, 7), (1.0 / 256, 3), (0.3, 11)):
        t8 = min(255, int(p * 256 + 0.5))
        pa = t8 / 256.0
        out = torch.empty_like(ones)
        check(lib().ecgvit_dropout_apply(ptr(ones), ptr(out), rows * d, p, seed, hip.BF16, stream()), 'dropout_apply')
        keep = (out != 0).float().view(rows, d)
        assert abs(float(keep.mean()) - (1 - pa)) < 1.5e-3, (p, float(keep.mean()))
        kept = out[out != 0].float()
        assert float((kept - 1.0 / (1 - pa)).abs().max()) <= 2.0 ** -8 / (1 - pa)      # 256 / (256 - t), rounded to bf16 once
        z = keep - keep.mean()
        var = float((z * z).mean())

        def corr(a, b):
            return float((a * b).mean()) / var
        for lag in (1, 2, 3, 4, 8, 64):                                # lags 1-3: mostly the same hash word; 4: the next Weyl step
            assert abs(corr(z[:, :-lag], z[:, lag:])) < 5e-3, (p, lag)
        assert abs(corr(z[:-1, :], z[1:, :])) < 5e-3
        colmean, rowmean = keep.mean(0), keep.mean(1)
        assert float((colmean - (1 - pa)).abs().max()) < 5 * (pa * (1 - pa) / rows) ** 0.5 + 1e-3
        assert float((rowmean - (1 - pa)).abs().max()) < 5 * (pa * (1 - pa) / d) ** 0.5 + 1e-3
        masks.append(keep)
    z0, z1 = masks[0] - masks[0].mean(), masks[1] - masks[1].mean()
    assert abs(float((z0 * z1).mean()) / float((z0 * z0).mean())) < 5e-3   # seeds 1 and 2: unrelated masks
    out = torch.empty_like(ones)
    assert lib().ecgvit_dropout_apply(ptr(ones), ptr(out), rows * d, 1.0 / 1024, 5, hip.BF16, stream()) != 0
    A, B = torch.zeros(256, 64, device='cuda', dtype=BF16), torch.zeros(256, 64, device='cuda', dtype=BF16)
    with pytest.raises(RuntimeError):
        hip.gemm(hip.GEMM_NT, A, B, torch.zeros(256, 256, device='cuda', dtype=BF16), 256, 256, 64, 64, 64, 256, epilogue=hip.EPI_DROPOUT, dropout_p=1e-3, seed=1)


@pytest.mark.parametrize('epi_extra', [0, 'lin'])
def test_large_gemm_dropout_mask_equals_dropout_apply(epi_extra):
    """the persistent A . B^T kernels' dropout (eight-wave body: plain + dropout; four-wave body: bias + residual + dropout, K >= 768) keeps
    exactly the elements ecgvit_dropout_apply keeps for the same (seed, element index): one mask function for every 16-bit site"""
    g = torch.Generator().manual_seed(21)
    M, N, K = 2304, 768, 768
    A, B = _operands(hip.GEMM_NT, M, N, K, BF16, g)
    p, seed = 0.1, 77
    C0 = torch.zeros(M, N, device='cuda', dtype=BF16)
    C1 = torch.zeros(M, N, device='cuda', dtype=BF16)
    bias = torch.randn(N, generator=g).cuda() if epi_extra else None
    res = torch.zeros(M, N, device='cuda', dtype=BF16) if epi_extra else None
    base = hip.EPI_BIAS | hip.EPI_RESIDUAL if epi_extra else 0
    hip.gemm(hip.GEMM_NT, dev(A), dev(B), C0, M, N, K, K, K, N, epilogue=base, bias=bias, residual=res, ldr=N)
    hip.gemm(hip.GEMM_NT, dev(A), dev(B), C1, M, N, K, K, K, N, epilogue=base | hip.EPI_DROPOUT, bias=bias, residual=res, ldr=N, dropout_p=p, seed=seed)
    C2 = torch.empty_like(C0)
    check(lib().ecgvit_dropout_apply(ptr(C0), ptr(C2), M * N, p, seed, hip.BF16, stream()), 'dropout_apply')
    nz = C0 != 0
    assert torch.equal((C1 != 0) & nz, (C2 != 0) & nz)
    assert abs(float((C1 != 0).float().mean()) - (1 - 26 / 256)) < 4e-3
    assert rel_err(C1, C2.float()) < 4e-3


@pytest.mark.parametrize('p,M,N', [(0.0, 2304, 1024), (0.25, 2304, 1024), (0.25, 2101, 1000), (0.25, 10277, 2048)])   # third: ragged tiles in both directions (N % 8 == 0); last: 328 tiles, i.e. workgroups that walk SEVERAL tiles (the x-aux launch requests a tile's saved-tensor rows with its first K-tile: counted waits across the tile boundary)
def test_ffn_saved_tensor_as_e4m3_bytes(p, M, N):
    """ECGVIT_EPI_AUX8: the saved tensor gelu'(pre) x dropout multiplier stored by the FFN-up epilogue as e4m3 bytes and read back by the x-aux epilogue
    of the FFN-down input gradient.  The forward OUTPUT is bit-identical with and without the flag; the bytes are the e4m3 rounding (torch's
    float8_e4m3fn cast) of the values the bf16 form rounds to bf16 -- compared through the bf16 tensor: within 2^-4 relative + the bf16 ulp, zeros
    (dropped elements) exactly where the bf16 form has them; the backward product with it equals the backward with the decoded bytes bit for bit
    and stays within the format's noise of the bf16 form.  Small shapes (not on the large kernel) reject the flag."""
    g = torch.Generator().manual_seed(9)
    K = 256
    A, B = _operands(hip.GEMM_NT, M, N, K, BF16, g)
    B = (B * 0.08).to(BF16)
    bias = torch.randn(N, generator=g) * 0.3
    Ad, Bd, bd = dev(A), dev(B), dev(bias)
    epi = hip.EPI_BIAS | hip.EPI_GELU | hip.EPI_GELU_GRAD_AUX | (hip.EPI_DROPOUT if p > 0 else 0)
    C1, X1 = torch.zeros(M, N, device='cuda', dtype=BF16), torch.zeros(M, N, device='cuda', dtype=BF16)
    C2, X2 = torch.zeros(M, N, device='cuda', dtype=BF16), torch.full((M, N), 0x7F, device='cuda', dtype=torch.uint8)
    kw = dict(bias=bd, dropout_p=p, seed=17)
    hip.gemm(hip.GEMM_NT, Ad, Bd, C1, M, N, K, K, K, N, epilogue=epi, aux=X1, ldaux=N, **kw)
    hip.gemm(hip.GEMM_NT, Ad, Bd, C2, M, N, K, K, K, N, epilogue=epi | hip.EPI_AUX8, aux=X2, ldaux=N, **kw)
    assert torch.equal(C1, C2)
    x8 = X2.view(torch.float8_e4m3fn).float()
    x16 = X1.float()
    assert bool((x8[x16 == 0] == 0).all()) and bool((x16[x8 == 0].abs() <= 2.0 ** -10).all())   # dropped stays dropped; only |v| below half of e4m3's smallest subnormal (2^-9) flushes
    assert bool(((x8 - x16).abs() <= 2.0 ** -4 * x16.abs() + 2.0 ** -9).all())
    # backward: dh = (dY . W) x aux (+ column sums)
    dY, W = _operands(hip.GEMM_NT, M, N, K, BF16, g)
    ws = torch.empty(8 * ((M + 255) // 256) * N, device='cuda', dtype=torch.uint8)
    outs = []
    for aux, extra in ((X1, 0), (X2, hip.EPI_AUX8), (x8.to(BF16), 0)):
        D, cs = torch.zeros(M, N, device='cuda', dtype=BF16), torch.zeros(N, device='cuda')
        hip.gemm(hip.GEMM_NT, dev(dY), dev(W), D, M, N, K, K, K, N, epilogue=hip.EPI_MUL_AUX | hip.EPI_COLSUM | extra, aux=aux, ldaux=N, workspace=ws, colsum_out=cs)
        outs.append((D, cs))
    assert torch.equal(outs[1][0], outs[2][0]) and torch.equal(outs[1][1], outs[2][1])      # e4m3 values are exact in bf16: same products
    d16, d8 = outs[0][0].double().cpu().flatten(), outs[1][0].double().cpu().flatten()
    assert float((d16 @ d8) / (d16.norm() * d8.norm())) > 0.9995
    # column sums (the FFN-up bias gradient): each is a sum of 2304 INCOHERENT terms here (random-sign products), so the e4m3 rounding -- zero-mean, rms
    # 2.6 % per element -- shows at its full relative size in the sum: what every gradient built from this tensor carries (cosine 0.9997 to the bf16 form)
    c16, c8 = outs[0][1].double().cpu(), outs[1][1].double().cpu()
    assert rel_err(c8, c16) < (4e-2 if M < 4096 else 6e-2) and float((c16 @ c8) / (c16.norm() * c8.norm())) > 0.999
    small = torch.zeros(64, 64, device='cuda', dtype=BF16)
    with pytest.raises(RuntimeError):
        hip.gemm(hip.GEMM_NT, small, small, torch.zeros(64, 64, device='cuda', dtype=BF16), 64, 64, 64, 64, 64, 64, epilogue=hip.EPI_MUL_AUX | hip.EPI_AUX8,
                 aux=torch.zeros(64, 64, device='cuda', dtype=torch.uint8), ldaux=64)


def test_stored_gelu_within_one_bf16_ulp_of_erf():
    """the bf16 path's GELU / GELU' (three-term erf, common.h) as STORED by the FFN-up epilogue against the f64 erf formulation evaluated on the
    epilogue's own f32 pre-activation: within one bf16 ulp of the exact value (+ 1e-4 absolute, the approximation's floor in the negative
    tail) over x in [-8, 8] -- the change of erf formulation (round 5) is invisible at the resolution of the stored tensors"""
    M, N, K = 4096, 256, 64
    A, Bm = torch.zeros(M, K), torch.zeros(N, K)
    A[:, 0] = torch.linspace(-8, 8, M)           # rank-1 product: pre[m, n] = a[m] * 1 + bias[n], exact in f32
    Bm[:, 0] = 1.0
    bias = torch.linspace(-0.03, 0.03, N)
    Ab, Bb = A.to(BF16), Bm.to(BF16)
    pre = Ab.double()[:, :1] * Bb.double()[:, 0].unsqueeze(0) + bias.double()
    C = torch.zeros(M, N, device='cuda', dtype=BF16)
    aux = torch.zeros(M, N, device='cuda', dtype=BF16)
    hip.gemm(hip.GEMM_NT, dev(Ab), dev(Bb), C, M, N, K, K, K, N, epilogue=hip.EPI_BIAS | hip.EPI_GELU | hip.EPI_GELU_GRAD_AUX, bias=dev(bias), aux=aux, ldaux=N)
    pre = pre.float().double()                   # the epilogue adds the bias in f32
    y, dy = gelu(pre), gelu_grad(pre)
    ey = (C.double().cpu() - y).abs()
    ed = (aux.double().cpu() - dy).abs()
    assert bool((ey <= 2.0 ** -8 * y.abs() + 1e-4).all()), float((ey - 2.0 ** -8 * y.abs()).max())
    assert bool((ed <= 2.0 ** -8 * dy.abs() + 1e-4).all()), float((ed - 2.0 ** -8 * dy.abs()).max())


@pytest.mark.parametrize('B,h,N,p', [(24, 12, 251, 0.0), (45, 6, 200, 0.0), (64, 5, 130, 0.0), (40, 12, 251, 0.2), (90, 3, 256, 0.1),
                                     (30, 10, 501, 0.0), (70, 4, 384, 0.0)])
def test_attention_bwd_persistent_stream(B, h, N, p):
    """the persistent backward (slab stream continuous across (record, head) items, counted waits, 1-3 items per workgroup) against
    the double-precision reference (p = 0) and against the one-item-per-workgroup kernel on the same dropout mask (p > 0);
    ragged N (a whole wave of keys out of range at N = 200 / 130), repeated launches bit-identical (a stream race would show)"""
    g = torch.Generator().manual_seed(B * 1000 + N)
    dh = 64
    d = h * dh
    scale = dh ** -0.5
    qkv = (torch.randn(B * N, 3 * d, generator=g) * 1.2).to(BF16)
    do = torch.randn(B * N, d, generator=g).to(BF16)
    qd, dod = dev(qkv), dev(do)
    out = torch.empty(B * N, d, device='cuda', dtype=BF16)
    lse = torch.zeros(B * h * N, device='cuda')
    check(lib().ecgvit_attention_fwd(ptr(qd), ptr(out), ptr(lse), B, N, h, dh, scale, p, 1234, hip.BF16, stream()), 'attn_fwd')

    def bwd(persist):
        fn = lib().ecgvit_attention_bwd if persist else tools_lib().ecgvit_attention_bwd_oneitem
        r = torch.full((B * N, 3 * d), float('nan'), device='cuda', dtype=BF16)
        check(fn(ptr(qd), ptr(out), ptr(dod), ptr(lse), ptr(r), B, N, h, dh, scale, p, 1234, hip.BF16, stream()), 'attn_bwd')
        torch.cuda.synchronize()
        return r
    new = bwd(True)
    assert torch.isfinite(new.float()).all()
    for _ in range(5):
        assert torch.equal(bwd(True), new)
    if N <= 256:                                             # the one-item kernel holds at most 256 keys
        old = bwd(False)
        assert rel_err(new, old.float().double().cpu()) < 2e-3
    if p == 0.0:
        qr = qkv.double().requires_grad_(True)
        o_ref, _, _ = _attn_ref(qr, B, N, h, dh, scale)
        o_ref.backward(do.double())
        for i, nm in enumerate('qkv'):
            assert rel_err(new[:, i * d:(i + 1) * d], qr.grad[:, i * d:(i + 1) * d]) < 2e-2, nm


def test_gemm_bf16_weight_gradient_stream_is_race_free_and_exact():
    """the streaming weight-gradient kernel (k-major operands, 3+2 tile rings, counted waits, split-K slabs): small-integer operands
    make every product and partial sum exact in f32, so dW must EQUAL the integer reference on every repeated launch"""
    g = torch.Generator().manual_seed(9)
    for (M, N, K) in ((768, 2304, 40000), (3072, 768, 33333 // 64 * 64 + 17), (256, 256, 130000)):
        A = torch.randint(-3, 4, (K, M), generator=g).to(BF16).cuda()     # dY: tokens x outputs
        B = torch.randint(-3, 4, (K, N), generator=g).to(BF16).cuda()     # X:  tokens x inputs
        ref = A.float().t() @ B.float()                                   # |sum| <= 9 * 130000 < 2^24: exact
        ws = torch.empty(max(16, hip.gemm_workspace_bytes(hip.GEMM_TN, BF16, M, N, K)), dtype=torch.uint8, device='cuda')
        C = torch.empty(M, N, device='cuda')
        for rep in range(10):
            C.fill_(float('nan'))
            hip.gemm(hip.GEMM_TN, A, B, C, M, N, K, M, N, N, workspace=ws)
            assert torch.equal(C, ref), (M, N, K, rep, int((C != ref).sum()))
