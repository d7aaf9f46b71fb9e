"""
The embedding and masked-objective kernels (csrc/rowops.hip: ecgvit_embed_finish / _bwd and their ragged pair; csrc/masked.hip: ecgvit_mask_embed_finish / _bwd,
ecgvit_gather_rows, ecgvit_scatter_rows, ecgvit_l1_loss_fwd_bwd) through the C ABI, element by element, against tests/embed_ref.py, whose case
lists and bounds tests/test_embed_ref.py calibrates on the CPU.  Every output is a slice of a larger buffer whose 64-element sentinel bands must
come back bit-identical, and is pre-filled with NaN; no element the contract owns may still be NaN; every call runs twice into fresh buffers and
the two results must have equal bits.  What is a copy, a single rounding or an exact zero is compared by bits; the batch sums (dpos, dcls) and
the loss are held to the derived bounds of embed_ref (`dpos_bound`, `l1_chain`), and each figure is printed (`RATIO case name value`, the error
divided by its bound) before it is asserted.

Worst RATIO per kernel, measured on the MI355X over every case of this file (a ratio above 1 is a failure):

    kernel, figure                    f32                               bf16
    ecgvit_embed_bwd       dpos       0.031   (33, 5, 72), p = 0        0.0039  (65, 3, 264), p = 0.5
    ecgvit_embed_bwd_ragged dpos      0.059   65 records of 2..6 tokens 0.0012  the same
    ecgvit_mask_embed_bwd  dpos       0.082   (33, 5, 72), any m        0.0014  (65, 3, 264), any m
    (varlen at full length dpos       0.082   (33, 5, 72), m = 2        0)
    ecgvit_l1_loss_fwd_bwd loss       0.092   (3, 5, 7), h = 21         0.026   (1, 2049, 2056), h = 25

(up to 33 bf16 terms of eight significant bits add exactly in f32, so most bf16 dpos figures are 0: there the bound is the one-ulp floor and
the test is one of exactness.)  Everything else in this file is a comparison of bits.
"""
import pytest
import torch

import embed_ref as R
from embed_ref import F32
from hiputil import ptr, check, stream, lib, hip, bits, Guarded, PAD, SENTINEL

pytestmark = pytest.mark.gpu

FLAG_BAND, FLAG_FILL = 0xA5, 7


class GuardedFlag:
    """n bytes of 7 inside a band of 0xA5: the mask workspace of ecgvit_mask_embed_finish"""

    def __init__(self, n):
        self.n = n
        self.buf = torch.full((n + 2 * PAD,), FLAG_BAND, dtype=torch.uint8, device='cuda')
        self.t = self.buf[PAD:PAD + n]
        self.t.fill_(FLAG_FILL)
        self.before = self.buf.clone()

    def bands_ok(self):
        return torch.equal(self.buf[:PAD], self.before[:PAD]) and torch.equal(self.buf[PAD + self.n:], self.before[PAD + self.n:])


def raw(t):
    return t if t.dtype == torch.uint8 else bits(t)


def twice(run):
    """run() -> {name: guarded buffer}, called twice: bands intact, equal bits; the first call's buffers"""
    a, b = run(), run()
    torch.cuda.synchronize()
    for k in a:
        assert a[k].bands_ok() and b[k].bands_ok(), f'{k}: a guard band was written'
        assert torch.equal(raw(a[k].buf), raw(b[k].buf)), f'{k}: two launches, different bits'
    return a


def written(name, t):
    assert not bool(torch.isnan(t.float()).any()), f'{name}: an element was never written'


def same_bits(name, got, want):
    assert got.shape == want.shape and got.dtype == want.dtype, name
    assert torch.equal(bits(got.contiguous()), bits(want.contiguous())), f'{name}: bits differ from the restatement'


def hold(cid, name, got, ref, bound):
    r = R.worst_ratio(got, ref, bound)
    print(f'RATIO {cid} {name} {r:.4g}')
    return [] if r <= 1.0 else [(name, r)]


def cases(shapes_of):
    return [pytest.param(dt, s, id=f'{R.dtype_id(dt)}-{R.shape_id(s[:3])}') for dt in R.DTYPES for s in shapes_of(dt)]


def dropout_apply(x, p, seed):
    """ecgvit_dropout_apply over the flat elements of x"""
    out = Guarded(x.numel(), x.dtype)
    check(lib().ecgvit_dropout_apply(ptr(x), ptr(out.t), x.numel(), float(p), int(seed), hip.code(x.dtype), stream()), 'dropout_apply')
    torch.cuda.synchronize()
    assert out.bands_ok()
    written('dropout_apply', out.t)
    return out.t.view(x.shape)


# ------------------------------------------------------------------------------------------------------------------ embed_finish / embed_bwd
class Embed:
    def __init__(self, B, n, d, dtype):
        self.B, self.n, self.N, self.d, self.dtype = B, n, n + 1, d, dtype
        self.tok, self.cls, self.pos, self.dX = (t.cuda() for t in R.embed_inputs(B, n, d, dtype))
        self.cid = f'{R.dtype_id(dtype)}-{R.shape_id((B, n, d))}'

    def fwd(self, p=0.0, seed=0):
        B, n, N, d = self.B, self.n, self.N, self.d

        def run():
            X = Guarded(B * N * d, self.dtype)
            check(lib().ecgvit_embed_finish(ptr(self.tok), ptr(self.cls), ptr(self.pos), ptr(X.t), B, n, d, float(p), int(seed), hip.code(self.dtype),
                                            stream()), 'embed_finish')
            return dict(X=X)
        X = twice(run)['X'].t.view(B, N, d)
        written('X', X)
        return X

    def bwd(self, p=0.0, seed=0):
        B, n, N, d = self.B, self.n, self.N, self.d

        def run():
            o = dict(dtok=Guarded(B * n * d, self.dtype), dcls=Guarded(d, F32), dpos=Guarded(N * d, F32))
            check(lib().ecgvit_embed_bwd(ptr(self.dX), ptr(o['dtok'].t), ptr(o['dcls'].t), ptr(o['dpos'].t), B, n, d, float(p), int(seed),
                                         hip.code(self.dtype), stream()), 'embed_bwd')
            return o
        o = twice(run)
        for k, g in o.items():
            written(k, g.t)
        return o['dtok'].t.view(B, n, d), o['dcls'].t, o['dpos'].t.view(N, d)

    def hold_bwd(self, got, dX, tag):
        """dX [B, N, d]: the gradient the sums are taken of (the dropped one under dropout)"""
        dtok, dcls, dpos = got
        same_bits('dtok', dtok, dX[:, 1:])
        same_bits('dcls == dpos[0]', dcls, dpos[0])
        _, _, ref = R.embed_bwd(dX)
        bad = hold(self.cid + tag, 'embed_bwd.dpos', dpos, ref, R.dpos_bound(dX, ref))
        assert not bad, (self.cid, bad)


@pytest.mark.parametrize('dtype,shape', cases(R.embed_shapes))
def test_embed_finish_and_bwd_by_element(dtype, shape):
    """p = 0: X is the restatement rounded once, bit for bit; dtok is rows 1..n of dX, dcls is row 0 of dpos, dpos within its bound of fp64"""
    B, n, d, forward_only = shape
    e = Embed(B, n, d, dtype)
    same_bits('X', e.fwd(), R.embed_rounded(e.tok, e.cls, e.pos, B, n, d, dtype))
    if not forward_only:
        e.hold_bwd(e.bwd(), e.dX.view(B, n + 1, d), '')


@pytest.mark.parametrize('dtype,shape,p', [pytest.param(dt, s, p, id=f'{R.dtype_id(dt)}-{R.shape_id(s)}-p{p}')
                                           for dt in R.DTYPES for s in R.DROPOUT_SHAPES for p in R.DROPOUT_P[dt]])
def test_embed_dropout_is_dropout_apply(dtype, shape, p):
    """one mask for the forward, the backward and ecgvit_dropout_apply: the per-site counter row * d + c0 is the flat element index"""
    B, n, d = shape
    e = Embed(B, n, d, dtype)
    seed = R.DROPOUT_SEED
    X0 = e.fwd()
    want = dropout_apply(X0, p, seed)
    dropped = int((want == 0).sum()) - int((X0 == 0).sum())
    assert 0 < dropped < X0.numel(), 'the mask drops nothing or everything: the comparison below would be empty'
    same_bits('X(p)', e.fwd(p, seed), want)
    dXd = dropout_apply(e.dX.view(B, n + 1, d), p, seed)
    e.hold_bwd(e.bwd(p, seed), dXd, f'-p{p}')


# ------------------------------------------------------------------------------------------------------------------ embed_finish_ragged / _bwd_ragged
def embed_ragged(e, tok, dX, n_tok, p=0.0, seed=0):
    """ecgvit_embed_finish_ragged / ecgvit_embed_bwd_ragged on packed rows (record b: n_tok[b] tokens from row tok_off[b] = the exclusive prefix
    sum), cls / pos / dtype of the Embed `e` -> X [M, d], dtok [M - B, d], dcls [d], dpos [N + 4, d] (N = the widest record)"""
    B, d = e.B, e.d
    n_tok = torch.as_tensor(n_tok, dtype=torch.int32)
    M, N = int(n_tok.sum()), int(n_tok.max())
    ntd, offd = n_tok.cuda(), (torch.cumsum(n_tok, 0, dtype=torch.int32) - n_tok).cuda()

    def run():
        o = dict(X=Guarded(M * d, e.dtype), dtok=Guarded((M - B) * d, e.dtype), dcls=Guarded(d, F32), dpos=Guarded((N + 4) * d, F32))
        check(lib().ecgvit_embed_finish_ragged(ptr(tok), ptr(e.cls), ptr(e.pos), ptr(o['X'].t), ptr(ntd), ptr(offd), B, N, d, float(p), int(seed),
                                               hip.code(e.dtype), stream()), 'embed_finish_ragged')
        check(lib().ecgvit_embed_bwd_ragged(ptr(dX), ptr(o['dtok'].t), ptr(o['dcls'].t), ptr(o['dpos'].t), ptr(ntd), ptr(offd), B, N, d, float(p),
                                            int(seed), hip.code(e.dtype), stream()), 'embed_bwd_ragged')
        return o
    o = twice(run)
    X, dtok, dcls, dpos = o['X'].t.view(M, d), o['dtok'].t.view(M - B, d), o['dcls'].t, o['dpos'].t.view(N + 4, d)
    written('X', X), written('dtok', dtok), written('dcls', dcls), written('dpos', dpos[:N])
    assert bool(torch.isnan(dpos[N:]).all()), 'a dpos row past the widest record was written'
    return X, dtok, dcls, dpos


@pytest.mark.parametrize('dtype,shape,p', [pytest.param(dt, s, p, id=f'{R.dtype_id(dt)}-{R.shape_id(s)}-p{p}')
                                           for dt in R.DTYPES for s in R.DROPOUT_SHAPES for p in (0.0, 0.1)])
def test_embed_ragged_equals_uniform_at_equal_lengths(dtype, shape, p):
    """n_tok[b] = n + 1, tok_off[b] = b (n + 1): the ragged pair returns the bits of the uniform pair -- the same element index for the dropout
    counter, the same lane walk, the same fold.  (33, 5, 72): lane 0 takes a second trip, the last column group is partly live; (65, 3, 264): a
    third trip"""
    B, n, d = shape
    e = Embed(B, n, d, dtype)
    seed = R.DROPOUT_SEED
    X, dtok, dcls, dpos = embed_ragged(e, e.tok, e.dX, [n + 1] * B, p, seed)
    same_bits('X', X.view(B, n + 1, d), e.fwd(p, seed))
    utok, ucls, upos = e.bwd(p, seed)
    same_bits('dtok', dtok.view(B, n, d), utok)
    same_bits('dpos', dpos[:n + 1], upos)
    same_bits('dcls', dcls, ucls)


@pytest.mark.parametrize('dtype', R.DTYPES, ids=R.dtype_id)
def test_embed_ragged_mixed_lengths_by_element(dtype):
    """B = 65 records of 2 + (7 b mod 5) tokens (N = 6; token 1 has 65 contributors, token 5 has 13: the lanes' trip counts differ across
    positions): X is each record's own restatement rounded once, bit for bit; dtok the copied rows; dpos[t] within the bound of the f64 sum over
    the records that hold t; dcls is row 0 of dpos"""
    B, d = 65, 72
    n_tok = [2 + 7 * b % 5 for b in range(B)]
    N, M = max(n_tok), sum(n_tok)
    e = Embed(B, N - 1, d, dtype)
    tok, dX = e.tok[:M - B], e.dX[:M]
    X, dtok, dcls, dpos = embed_ragged(e, tok, dX, n_tok)
    r0 = 0
    for b, nb in enumerate(n_tok):
        same_bits(f'X of record {b}', X[r0:r0 + nb], R.embed_rounded(tok[r0 - b:r0 - b + nb - 1], e.cls, e.pos[:nb], 1, nb - 1, d, dtype)[0])
        same_bits(f'dtok of record {b}', dtok[r0 - b:r0 - b + nb - 1], dX[r0 + 1:r0 + nb])
        r0 += nb
    same_bits('dcls == dpos[0]', dcls, dpos[0])
    off = torch.cumsum(torch.tensor([0] + n_tok[:-1]), 0)
    ref, bound = [], []
    for t in range(N):
        terms = dX[[int(off[b]) + t for b in range(B) if n_tok[b] > t]].to(R.F64)[:, None]     # [the records that hold t, 1, d]
        assert terms.shape[0] == {0: 65, 1: 65, 5: 13}.get(t, terms.shape[0])
        ref.append(terms.sum(0))
        bound.append(R.dpos_bound(terms, ref[-1]))
    cid = f'{R.dtype_id(dtype)}-ragged-{B}x{d}'
    bad = hold(cid, 'embed_bwd_ragged.dpos', dpos[:N], torch.cat(ref), torch.cat(bound))
    assert not bad, (cid, bad)


# ------------------------------------------------------------------------------------------------------------------ mask_embed_finish / _bwd
class MaskEmbed:
    def __init__(self, B, n, d, dtype, m):
        self.B, self.n, self.d, self.dtype, self.m = B, n, d, dtype, m
        self.tok, self.mt, self.pos, self.dX = (t.cuda() for t in R.embed_inputs(B, n, d, dtype, cls_row=False))
        idx = R.mask_index(B, n, m)
        self.idx = None if idx is None else idx.cuda()
        self.mask = R.mask_of(self.idx, B, n, 'cuda')
        self.cid = f'{R.dtype_id(dtype)}-{R.shape_id((B, n, d))}-m{m}'

    def fwd(self):
        B, n, d, m = self.B, self.n, self.d, self.m

        def run():
            o = dict(X=Guarded(B * n * d, self.dtype), flag=GuardedFlag(B * n))
            check(lib().ecgvit_mask_embed_finish(ptr(self.tok), ptr(self.mt), ptr(self.pos), ptr(self.idx), ptr(o['X'].t), ptr(o['flag'].t), B, n, m, d,
                                                 hip.code(self.dtype), stream()), 'mask_embed_finish')
            return o
        o = twice(run)
        written('X', o['X'].t)
        return o['X'].t.view(B, n, d), o['flag'].t

    def bwd(self, flag):
        B, n, d = self.B, self.n, self.d

        def run():
            o = dict(dtok=Guarded(B * n * d, self.dtype), dmasked=Guarded(B * n * d, self.dtype), dpos=Guarded((n + 4) * d, F32))
            check(lib().ecgvit_mask_embed_bwd(ptr(self.dX), ptr(flag), ptr(o['dtok'].t), ptr(o['dmasked'].t), ptr(o['dpos'].t), B, n, d,
                                              hip.code(self.dtype), stream()), 'mask_embed_bwd')
            return o
        o = twice(run)
        return o['dtok'].t.view(B, n, d), o['dmasked'].t.view(B, n, d), o['dpos'].t.view(n + 4, d)

    def hold_fwd(self, X, flag):
        B, n, d = self.B, self.n, self.d
        same_bits('X', X, R.mask_embed_rounded(self.tok, self.mt, self.pos, self.mask, B, n, d, self.dtype))
        assert torch.equal(flag.view(B, n), self.mask.to(torch.uint8)), 'flag_ws is not the 0 / 1 mask'

    def hold_bwd(self, got, tag=''):
        n = self.n
        dtok, dmasked, dpos = got
        dX = self.dX.view(self.B, n, self.d)
        zero = torch.zeros_like(dX)
        written('dtok', dtok), written('dmasked', dmasked), written('dpos', dpos[:n + 1])
        same_bits('dtok', dtok, torch.where(self.mask[..., None], zero, dX))
        same_bits('dmasked', dmasked, torch.where(self.mask[..., None], dX, zero))
        assert bool((bits(dpos[0]) == 0).all()), 'dpos row 0 is not exactly +0'
        assert bool(torch.isnan(dpos[n + 1:]).all()), 'a dpos row past n was written'
        ref = R.mask_embed_bwd(dX, self.mask)[2]
        bad = hold(self.cid + tag, 'mask_embed_bwd.dpos', dpos[1:n + 1], ref[1:], R.dpos_bound(dX, ref[1:]))
        assert not bad, (self.cid, bad)


@pytest.mark.parametrize('dtype,shape', cases(R.mask_shapes))
def test_mask_embed_finish_and_bwd_by_element(dtype, shape):
    """m in {0, 1, n // 2, n} rows by randperm (m = 0: a null idx): X bit for bit, flag_ws the 0 / 1 mask inside its own bands; on that flag dtok
    and dmasked are dX split by the mask with exact zeros, dpos rows 1..n within the bound, row 0 exactly 0, the rows past n untouched"""
    B, n, d, forward_only = shape
    for m in R.mask_counts(n):
        k = MaskEmbed(B, n, d, dtype, m)
        X, flag = k.fwd()
        k.hold_fwd(X, flag)
        if not forward_only:
            k.hold_bwd(k.bwd(flag))


@pytest.mark.parametrize('dtype', R.DTYPES, ids=R.dtype_id)
def test_mask_embed_uniform_equals_varlen_at_full_length(dtype):
    """ecgvit_mask_embed_varlen_fwd / _bwd with every n_tok = n, n_pad = n and order = 0..B-1: X, dtok and dmasked bit-equal to the uniform pair,
    both dpos inside the bound"""
    B, n, d = R.VARLEN_CROSS_SHAPE
    m = n // 2
    k = MaskEmbed(B, n, d, dtype, m)
    X, flag = k.fwd()
    k.hold_fwd(X, flag)
    uni = k.bwd(flag)
    k.hold_bwd(uni)
    ar = torch.arange(B, dtype=torch.int32, device='cuda')
    n_tok, tok_off, order = torch.full_like(ar, n), ar * n, ar.clone()
    rows = (tok_off[:, None] + k.idx).reshape(-1).contiguous()

    def run_fwd():
        o = dict(X=Guarded(B * n * d, dtype), flag=GuardedFlag(B * n))
        check(lib().ecgvit_mask_embed_varlen_fwd(ptr(k.tok), ptr(k.mt), ptr(k.pos), ptr(rows), ptr(o['X'].t), ptr(o['flag'].t), ptr(n_tok), ptr(tok_off),
                                                 B, n, n, B * n, B * m, d, hip.code(dtype), stream()), 'mask_embed_varlen_fwd')
        return o
    f = twice(run_fwd)
    same_bits('varlen X', f['X'].t.view(B, n, d), X)
    assert torch.equal(f['flag'].t, flag)

    def run_bwd():
        o = dict(dtok=Guarded(B * n * d, dtype), dmasked=Guarded(B * n * d, dtype), dpos=Guarded((n + 4) * d, F32))
        check(lib().ecgvit_mask_embed_varlen_bwd(ptr(k.dX), ptr(f['flag'].t), ptr(o['dtok'].t), ptr(o['dmasked'].t), ptr(o['dpos'].t), ptr(n_tok),
                                                 ptr(tok_off), ptr(order), B, n, n, d, hip.code(dtype), stream()), 'mask_embed_varlen_bwd')
        return o
    o = twice(run_bwd)
    var = (o['dtok'].t.view(B, n, d), o['dmasked'].t.view(B, n, d), o['dpos'].t.view(n + 4, d))
    same_bits('varlen dtok', var[0], uni[0])
    same_bits('varlen dmasked', var[1], uni[1])
    k.hold_bwd(var, '-varlen')


# ------------------------------------------------------------------------------------------------------------------ gather_rows / scatter_rows
@pytest.mark.parametrize('f,dtype', [pytest.param(f, dt, id=f'{R.dtype_id(dt)}-{R.shape_id(f["form"])}') for f in R.ROW_FORMS for dt in f['dtypes']])
def test_gather_and_scatter_rows_forms(f, dtype):
    """bit-exact against torch indexing in every form the engine calls; pitch gaps of `in` hold NaN that must not travel, pitch gaps of `out` and,
    in a scatter, the rows no index names keep their sentinel bits"""
    B, n, m, width, ld_in, ld_out = f['form']
    idx = R.row_index(f['form'], f['idx']).cuda()
    li, bi = idx.long(), torch.arange(B, device='cuda')[:, None]
    g = torch.Generator(device='cuda').manual_seed(B * 1000 + n)

    def source(rows):
        t = torch.randn(rows, ld_in, device='cuda', generator=g).to(dtype)
        t[:, width:] = float('nan')
        return t

    # gather: out[b m + k] = in[b n + idx[b, k]]
    src = source(B * n)

    def run_gather():
        out = Guarded(B * m * ld_out, dtype)
        out.t.view(B * m, ld_out)[:, width:] = SENTINEL
        check(lib().ecgvit_gather_rows(ptr(src), ptr(idx), ptr(out.t), B, n, m, width, ld_in, ld_out, hip.code(dtype), stream()), 'gather_rows')
        return dict(out=out)
    got = twice(run_gather)['out'].t.view(B, m, ld_out)
    want = torch.full((B, m, ld_out), SENTINEL, dtype=dtype, device='cuda')
    want[:, :, :width] = src.view(B, n, ld_in)[bi, li][:, :, :width]
    written('gather', got)
    same_bits('gather', got, want)
    del src, got, want

    # scatter: out[b n + idx[b, k]] = in[b m + k], into a buffer that holds the sentinel everywhere
    src = source(B * m)

    def run_scatter():
        out = Guarded(B * n * ld_out, dtype)
        out.t.fill_(SENTINEL)
        check(lib().ecgvit_scatter_rows(ptr(src), ptr(idx), ptr(out.t), B, n, m, width, ld_in, ld_out, hip.code(dtype), stream()), 'scatter_rows')
        return dict(out=out)
    got = twice(run_scatter)['out'].t.view(B, n, ld_out)
    want = torch.full((B, n, ld_out), SENTINEL, dtype=dtype, device='cuda')
    head = want[:, :, :width]
    head[bi, li] = src.view(B, m, ld_in)[:, :, :width]
    written('scatter', got)
    same_bits('scatter', got, want)
    assert int((got[:, :, 0] != SENTINEL).sum()) == B * m       # exactly the named rows changed


# ------------------------------------------------------------------------------------------------------------------ l1_loss_fwd_bwd
@pytest.mark.parametrize('c,dtype', [pytest.param(c, dt, id=f'{R.dtype_id(dt)}-{R.shape_id(c["case"])}') for c in R.L1_CASES for dt in R.DTYPES])
def test_l1_loss_by_element(c, dtype):
    """three ways (gscalar null, gscalar = 2.5, dpred null): one loss bit pattern, within h 2^-24 relative of the fp64 mean; dpred one constant
    rounded once with the exact sign, exactly 0 at ties, the pitch gap untouched"""
    rows, width, ld = c['case']
    cid = f'{R.dtype_id(dtype)}-{R.shape_id(c["case"])}'
    pred, target = (t.cuda() for t in R.l1_inputs(rows, width, ld, dtype))
    gs = torch.tensor([R.L1_GSCALAR], device='cuda')
    nb, _ = R.l1_blocks(rows * width)
    h = R.l1_chain(rows * width)
    ref, _ = R.l1(pred, target, rows, width, ld)
    bound = h * R.U32 * ref

    def way(gscalar, with_dpred):
        def run():
            o = dict(loss=Guarded(1, F32), partial=Guarded(R.L1_BLOCKS, F32))
            if with_dpred:
                o['dpred'] = Guarded(rows * ld, dtype)
                o['dpred'].t.view(rows, ld)[:, width:] = SENTINEL
            check(lib().ecgvit_l1_loss_fwd_bwd(ptr(pred), ptr(target), ptr(o['loss'].t), ptr(o['dpred'].t) if with_dpred else None,
                                               ptr(gs) if gscalar is not None else None, ptr(o['partial'].t), rows, width, ld, hip.code(dtype), stream()),
                  'l1_loss_fwd_bwd')
            return o
        o = twice(run)
        written('loss', o['loss'].t), written('partial', o['partial'].t[:nb])
        if with_dpred:
            got = o['dpred'].t.view(rows, ld)
            want = torch.full((rows, ld), SENTINEL, dtype=dtype, device='cuda')
            want[:, :width] = R.l1_dpred_rounded(pred, target, rows, width, ld, gscalar, dtype)
            written('dpred', got)
            same_bits(f'dpred (gscalar {gscalar})', got, want)
        return o['loss'].t

    losses = {'plain': way(None, True), 'gscalar': way(R.L1_GSCALAR, True), 'loss_only': way(None, False)}
    bad = []
    for name, loss in losses.items():
        bad += hold(cid, f'l1.loss.{name}', loss[0], ref, bound)
    print(f'l1 {cid}: nb {nb}, h {h}, loss {float(losses["plain"][0]):.9g}, fp64 {float(ref):.17g}')
    same_bits('loss with and without dpred', losses['loss_only'], losses['plain'])
    same_bits('loss with and without gscalar', losses['gscalar'], losses['plain'])
    assert not bad, (cid, bad)
