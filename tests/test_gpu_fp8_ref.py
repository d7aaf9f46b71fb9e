"""-m gpu: every producer of 8-bit operand copies outside LayerNorm and attention (which tests/test_gpu_fp8.py, tests/test_gpu_layernorm.py and
tests/test_gpu_long_attention.py hold to the same criterion) against the exact encoder of tests/fp8_ref.py, byte by byte: no share of bytes may
differ anywhere.  Coverage, case by case:

    ecgvit_fp8_quantize, all 65 536 bf16 patterns (NaN -> 0, +-inf kept), both formats      test_quantize_every_bf16_pattern
        scales 1, 2^-6, 2^5: one accepted byte; 0.0137, 3.1e-5 (over half of e4m3 saturates), 6e37 (the 8-bit subnormals); 0 and -0.37: zero codes
        amax_next from 0, pre-filled below and above the maximum, NULL
    the count % 16 == 8 branch of fp8_quantize_kernel (the 8-byte tail store)                  test_quantize_and_amax_length_edges
        counts 8, 24, 4088, 4104 (lane 0's second trip), 4096 x 4096 + 24 (the capped grid's second trip ends in the tail); 16: no tail
    segment tables: unequal, gaps, a segment of 8, tails in three, one past the nseg > 1 cap  test_quantize_and_amax_segment_table
        x between the segments is 1e30 (a read outside shows in the amax), y and the amax slots around them carry sentinels
    ecgvit_fp8_amax: the maximum a negative value, -0.0, a bf16 subnormal, a tail's last       test_amax_sign_zero_subnormal_and_last_of_tail
    the per-site `formats` path of ecgvit_fp8_scale_update, n = 257, mixed formats             test_scale_update_per_site_formats
        amax 0 keeps a positive scale, amax 0 with scale 0 (or below) gives 1.0, every amax reset, scale = f32(amax) / f32(max)
    every Q-bearing epilogue set of the 8-bit A . B^T kernel (csrc/gemm_plan.h)                test_epi_quant_out
        UP|Q, UP|D|Q, UP|Q|A8, UP|D|Q|A8 (e4m3 x e4m3 -> e4m3 copy), DH|Q, DH|Q|A8 (e5m2 x e4m3 -> e5m2 copy), each with its |NO form: 12 sets
        (2051, 136, 384) a 3-row last tile; (2304, 264, 512) an 8-column last tile; (8200, 2056, 384) 297 tiles on 256 workgroups
        the several-tiles-per-workgroup amax carry: the last shape, *q8_amax pre-filled below (the carry must raise it) and above
        a power-of-two q8_scale (one accepted byte) and a saturating one that is none; ldq8 = N + 24 and 3 slack rows of sentinels
    small-integer operands, q8_scale = 1, three launches                                       test_epi_quant_out_small_integers
        the DH sets only: the UP sets pass through GELU, which no operands make exact
"""
import math

import pytest
import torch

import fp8_ref as R
from fp8_ref import E4M3, E5M2, F32, BF16, FMAX, FMT_CODE
from ecg_representation_learning_amd import hip
from ecg_representation_learning_amd.hip import lib, check, ptr, stream

pytestmark = pytest.mark.gpu
SENT = 0x7F        # NaN in both formats: no emitter produces it
POISON = 1e30      # x outside what a call may read


def _data(n, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(n, generator=g) * torch.exp(torch.randn(n, generator=g))).to(BF16).cuda()


def _assert_accepted(got, stored, scale, fmt, what):
    ok = R.accepts(got, stored, scale, fmt)
    assert bool(ok.all()), (what, R.describe_refused(got, stored, scale, fmt))


def _f32(v):
    return torch.tensor([v], dtype=F32, device='cuda')


# ------------------------------------------------------------------------------------------------------------------ 1. exhaustive quantise
@pytest.mark.parametrize('fmt', R.FORMATS)
def test_quantize_every_bf16_pattern(fmt):
    x = R.all_bf16('cuda')
    xfin = torch.where(torch.isinf(x), torch.zeros_like(x), x)
    n = x.numel()
    top = R.code_values(fmt).numel() - 1
    for scale in R.POW2_SCALES + R.QUANT_NP2_SCALES:
        assert len(R.reciprocals(scale)) == (1 if scale in R.POW2_SCALES else 3)
        sc = _f32(scale)
        y = torch.full((n,), SENT, dtype=torch.uint8, device='cuda')
        nxt = torch.zeros(1, device='cuda')
        check(lib().ecgvit_fp8_quantize(ptr(x), ptr(y), None, 1, n, FMT_CODE[fmt], ptr(sc), ptr(nxt), stream()), 'quantize')
        _assert_accepted(y, x, sc, fmt, (fmt, scale))
        assert float(nxt) == math.inf                                                   # max |x| over +-inf
        code = y & 0x7F
        if scale == R.SATURATING_SCALE:
            assert float((code == top).float().mean()) > (0.5 if fmt == E4M3 else 0.4)
        if scale == R.SUBNORMAL_SCALE:
            assert float((code < 2 ** R._DEF[fmt][1]).float().mean()) > 0.9
        # amax_next: the maximum semantics on finite input, and NULL
        true_max = float(xfin.float().abs().max())
        for pre, want in ((1.0, true_max), (float(torch.finfo(F32).max), float(torch.finfo(F32).max))):
            assert (pre < true_max) == (want == true_max)
            nxt = _f32(pre)
            y2 = torch.full((n,), SENT, dtype=torch.uint8, device='cuda')
            check(lib().ecgvit_fp8_quantize(ptr(xfin), ptr(y2), None, 1, n, FMT_CODE[fmt], ptr(sc), ptr(nxt), stream()), 'quantize')
            assert float(nxt) == want
            _assert_accepted(y2, xfin, sc, fmt, (fmt, scale, 'finite'))
        y3 = torch.full((n,), SENT, dtype=torch.uint8, device='cuda')
        check(lib().ecgvit_fp8_quantize(ptr(x), ptr(y3), None, 1, n, FMT_CODE[fmt], ptr(sc), None, stream()), 'quantize')
        assert torch.equal(y3, y)
    for scale in R.ZERO_CODE_SCALES:
        sc = _f32(scale)
        y = torch.full((n,), SENT, dtype=torch.uint8, device='cuda')
        nxt = torch.zeros(1, device='cuda')
        check(lib().ecgvit_fp8_quantize(ptr(xfin), ptr(y), None, 1, n, FMT_CODE[fmt], ptr(sc), ptr(nxt), stream()), 'quantize')
        assert bool(((y & 0x7F) == 0).all()), (fmt, scale)
        _assert_accepted(y, xfin, sc, fmt, (fmt, scale))
        assert float(nxt) == float(xfin.float().abs().max())


# ------------------------------------------------------------------------------------------------------------------ 2. lengths and segments
@pytest.mark.parametrize('fmt', R.FORMATS)
@pytest.mark.parametrize('count', R.COUNTS)
def test_quantize_and_amax_length_edges(count, fmt):
    pad = 64
    xb = torch.full((count + 2 * pad,), POISON, dtype=BF16, device='cuda')
    xb[pad:pad + count] = _data(count, count)
    x = xb[pad:pad + count]
    true_max = float(x.float().abs().max())
    am = torch.tensor([-5.0, 0.0, -5.0], device='cuda')
    check(lib().ecgvit_fp8_amax(ptr(x), None, 1, count, ptr(am[1:]), stream()), 'amax')
    assert am.tolist() == [-5.0, true_max, -5.0]
    for scale in (0.25, 0.0137):
        sc = _f32(scale)
        yb = torch.full((count + 2 * pad,), SENT, dtype=torch.uint8, device='cuda')
        nxt = torch.tensor([-5.0, 0.0, -5.0], device='cuda')
        check(lib().ecgvit_fp8_quantize(ptr(x), ptr(yb[pad:]), None, 1, count, FMT_CODE[fmt], ptr(sc), ptr(nxt[1:]), stream()), 'quantize')
        _assert_accepted(yb[pad:pad + count], x, sc, fmt, (count, fmt, scale))
        assert bool((yb[:pad] == SENT).all()) and bool((yb[pad + count:] == SENT).all())
        assert nxt.tolist() == [-5.0, true_max, -5.0]


@pytest.mark.parametrize('fmt', R.FORMATS)
def test_quantize_and_amax_segment_table(fmt):
    nseg = len(R.SEGMENTS)
    xb = torch.full((R.SEG_TOTAL,), POISON, dtype=BF16, device='cuda')
    inside = torch.zeros(R.SEG_TOTAL, dtype=torch.bool, device='cuda')
    for s, (off, cnt) in enumerate(R.SEGMENTS):
        xb[off:off + cnt] = _data(cnt, 100 + s) * (3.0 ** s)
        inside[off:off + cnt] = True
    table = torch.tensor(R.SEGMENTS, dtype=torch.int64, device='cuda')
    nmax = max(c for _, c in R.SEGMENTS)
    want_max = [float(xb[o:o + c].float().abs().max()) for o, c in R.SEGMENTS]
    am = torch.tensor([-5.0] + [0.0] * nseg + [-5.0], device='cuda')
    check(lib().ecgvit_fp8_amax(ptr(xb), ptr(table), nseg, nmax, ptr(am[1:]), stream()), 'amax')
    assert am.tolist() == [-5.0] + want_max + [-5.0]
    scales = torch.tensor(R.SEG_SCALES, dtype=F32, device='cuda')
    yb = torch.full((R.SEG_TOTAL,), SENT, dtype=torch.uint8, device='cuda')
    nxt = torch.tensor([-5.0] + [0.0] * nseg + [-5.0], device='cuda')
    check(lib().ecgvit_fp8_quantize(ptr(xb), ptr(yb), ptr(table), nseg, nmax, FMT_CODE[fmt], ptr(scales), ptr(nxt[1:]), stream()), 'quantize')
    for s, (off, cnt) in enumerate(R.SEGMENTS):
        _assert_accepted(yb[off:off + cnt], xb[off:off + cnt], scales[s], fmt, (fmt, 'segment', s))
    assert bool((yb[~inside] == SENT).all())
    assert nxt.tolist() == [-5.0] + want_max + [-5.0]


@pytest.mark.parametrize('case', ['negative', 'minus_zero', 'subnormal', 'last_of_tail'])
def test_amax_sign_zero_subnormal_and_last_of_tail(case):
    count = 4096 + 24
    x = (_data(count, 7).float().abs().clamp(max=1.0) * 0.5).to(BF16)
    if case == 'negative':
        x[count // 2] = -7.0
        want = 7.0
    elif case == 'minus_zero':
        x = torch.full((count,), -0.0, dtype=BF16, device='cuda')
        want = 0.0
    elif case == 'subnormal':
        x = torch.zeros(count, dtype=BF16, device='cuda')
        x[5] = -(2.0 ** -130)
        assert float(x[5]) == -(2.0 ** -130)
        want = 2.0 ** -130
    else:
        x[count - 1] = 3.0
        want = 3.0
    am = torch.zeros(1, device='cuda')
    check(lib().ecgvit_fp8_amax(ptr(x), None, 1, count, ptr(am), stream()), 'amax')
    assert float(am) == want and int(am.view(torch.int32)) == int(torch.tensor(want, dtype=F32).view(torch.int32))
    nxt = torch.zeros(1, device='cuda')
    y = torch.full((count,), SENT, dtype=torch.uint8, device='cuda')
    sc = _f32(0.0137)
    check(lib().ecgvit_fp8_quantize(ptr(x), ptr(y), None, 1, count, FMT_CODE[E4M3], ptr(sc), ptr(nxt), stream()), 'quantize')
    assert float(nxt) == want and int(nxt.view(torch.int32)) == int(torch.tensor(want, dtype=F32).view(torch.int32))
    _assert_accepted(y, x, sc, E4M3, case)


# ------------------------------------------------------------------------------------------------------------------ 3. scale update
def test_scale_update_per_site_formats():
    n = R.SCALE_UPDATE_N
    g = torch.Generator().manual_seed(11)
    fm = torch.randint(2, 4, (n,), generator=g, dtype=torch.int32)
    fm[256] = hip.BF8_E5M2                                  # the one live lane of the second block
    amax = (torch.rand(n, generator=g) * torch.exp(4 * torch.randn(n, generator=g))).to(F32)
    scale = torch.rand(n, generator=g).to(F32) + 0.1
    keep, never, below = torch.arange(n) % 5 == 1, torch.arange(n) % 5 == 2, torch.arange(n) % 10 == 7
    amax[keep | never] = 0.0
    scale[never] = 0.0
    scale[never & below] = -2.0
    amax[256], scale[0] = 3.25, 0.0                         # a first amax on a scale never set
    amax[0] = 1.5
    assert bool((amax[~(keep | never)] > 0).all()) and int(keep.sum()) > 40 and int(never.sum()) > 40 and int((never & below).sum()) > 0
    fmax = torch.where(fm == hip.BF8_E5M2, torch.tensor(FMAX[E5M2], dtype=F32), torch.tensor(FMAX[E4M3], dtype=F32))
    want = torch.where(amax > 0, amax / fmax, torch.where(scale > 0, scale, torch.ones_like(scale)))   # the f32 quotient (host division: correctly rounded)
    assert len(set(fm.tolist())) == 2
    sd, ad, fd = scale.cuda(), amax.cuda(), fm.cuda()
    check(lib().ecgvit_fp8_scale_update(ptr(sd), ptr(ad), n, ptr(fd), hip.FP8_E4M3, stream()), 'scale_update')   # format_all is ignored
    assert torch.equal(sd.cpu(), want), int((sd.cpu() != want).sum())
    assert bool((ad == 0).all()) and not bool(torch.signbit(ad).any())
    # one format for all: the other branch, same sites
    sd, ad = scale.cuda(), amax.cuda()
    check(lib().ecgvit_fp8_scale_update(ptr(sd), ptr(ad), n, None, hip.BF8_E5M2, stream()), 'scale_update')
    want_all = torch.where(amax > 0, amax / torch.tensor(FMAX[E5M2], dtype=F32), torch.where(scale > 0, scale, torch.ones_like(scale)))
    assert torch.equal(sd.cpu(), want_all) and bool((ad == 0).all())


# ------------------------------------------------------------------------------------------------------------------ 4. EPI_QUANT_OUT
SA, SB = 0.37, 0.19
_REF = {}


@pytest.fixture(scope='module', autouse=True)
def _drop_references():
    yield
    _REF.clear()
    torch.cuda.empty_cache()


def _operands(shape, afmt):
    """operands and the float64 product of their dequantised values, once per (shape, format of A)"""
    key = (shape, afmt)
    if key not in _REF:
        M, N, K = shape
        g = torch.Generator().manual_seed(M + N + K + (afmt == E5M2))
        A = (torch.randn(M, K, generator=g) * 2.0).to(R.TORCH8[afmt]).cuda()
        B = (torch.randn(N, K, generator=g) * 0.5).to(R.TORCH8[E4M3]).cuda()
        sa, sb = _f32(SA), _f32(SB)
        s = float(sa) * float(sb)
        Ad, Bd = A.float().double(), B.float().double()
        acc = (Ad @ Bd.t()) * s
        absp = (Ad.abs() @ Bd.abs().t()) * abs(s)
        bias = (torch.randn(N, generator=g) * 0.3).cuda()
        auxv = (torch.rand(M, N, generator=g) * 1.2).to(R.TORCH8[E4M3])          # exact in bf16 too: one saved tensor for both forms
        aux16, aux8 = auxv.float().to(BF16).cuda(), auxv.view(torch.uint8).cuda()
        ones = torch.ones(M * N, dtype=BF16, device='cuda')
        keep = torch.empty_like(ones)
        check(lib().ecgvit_dropout_apply(ptr(ones), ptr(keep), M * N, R.GEMM_P, R.GEMM_SEED, hip.BF16, stream()), 'dropout_apply')
        keep = (keep != 0).view(M, N)
        _REF[key] = dict(A=A.view(torch.uint8), B=B.view(torch.uint8), sa=sa, sb=sb, acc=acc, absp=absp, bias=bias, aux16=aux16, aux8=aux8, keep=keep)
    return _REF[key]


def _reference(o, flags, K):
    """(ref, bound, must_be_zero) of C, float64"""
    if flags & R.EPI_GELU:
        pre = o['acc'] + o['bias'].double()
        y = 0.5 * pre * (1 + torch.erf(pre / 2 ** 0.5))
        if flags & R.EPI_DROPOUT:
            inv = 256.0 / (256.0 - round(256 * R.GEMM_P))
            assert abs(inv - 1 / (1 - R.GEMM_P)) < 1e-12
            ref, zero = y * inv, ~o['keep']
        else:
            inv, ref, zero = 1.0, y, None
        bound = 2.0 ** -8 * ref.abs() + 1e-4 * inv + R.GELU_LIP * inv * (K * 2.0 ** -23) * o['absp']
        return ref, bound, zero
    aux = o['aux16'].double()
    ref = o['acc'] * aux
    return ref, R.c_bound(ref, o['absp'], K, aux.abs(), False), None


def _launch(o, shape, flags, afmt, q8_scale, amax_pre, no_out, check_kernel=True):
    M, N, K = shape
    ldq = N + R.LDQ_PAD
    fl = flags | (R.EPI_NO if no_out else 0)
    C = torch.full((M + R.SLACK_ROWS, N), float('nan'), dtype=BF16, device='cuda')
    q8 = torch.full((M + R.SLACK_ROWS, ldq), SENT, dtype=torch.uint8, device='cuda')
    am = _f32(amax_pre)
    kw = dict(fp8_format=FMT_CODE[afmt], scale_a=o['sa'], scale_b=o['sb'], epilogue=fl, q8_out=q8, ldq8=ldq, q8_scale=q8_scale, q8_amax=am,
              q8_format=FMT_CODE[afmt])
    out = dict(q8=q8, am=am, C=C)
    if flags & R.EPI_GELU:
        aux = torch.full((M, N), SENT, dtype=torch.uint8, device='cuda') if flags & R.EPI_A8 else torch.full((M, N), float('nan'), dtype=BF16, device='cuda')
        kw.update(bias=o['bias'], aux=aux, ldaux=N, dropout_p=R.GEMM_P if flags & R.EPI_DROPOUT else 0.0, seed=R.GEMM_SEED)
        out['aux'] = aux
    else:
        ws = torch.empty(max(lib().ecgvit_colsum_workspace(M, N), 8 * ((M + 255) // 256) * N), dtype=torch.uint8, device='cuda')
        cs = torch.full((N,), float('nan'), device='cuda')
        kw.update(aux=o['aux8'] if flags & R.EPI_A8 else o['aux16'], ldaux=N, workspace=ws, colsum_out=cs)
        out['cs'] = cs
    args = (hip.GEMM_NT, o['A'], o['B'], None if no_out else C, M, N, K, K, K, N)
    assert hip.gemm_kernel(*args, **kw) == hip.KERNEL_GEMM_NT, (shape, fl)
    hip.gemm(*args, **kw)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize('shape', R.GEMM_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
@pytest.mark.parametrize('name', list(R.Q_SETS))
def test_epi_quant_out(name, shape):
    flags, fmt = R.Q_SETS[name]
    M, N, K = shape
    o = _operands(shape, fmt)
    ref, bound, zero = _reference(o, flags, K)
    top = R.code_values(fmt).numel() - 1
    # run 1: a power-of-two scale near max |ref| / max (one accepted byte), the amax slot pre-filled below the maximum
    s1 = 2.0 ** math.ceil(math.log2(float(ref.abs().max()) / FMAX[fmt]))
    runs = [(_f32(s1), 2.0 ** -20)]
    for i in range(2):
        q8_scale, pre = runs[i]
        w = _launch(o, shape, flags, fmt, q8_scale, pre, False)
        C = w['C'][:M]
        stored = C.float()
        cmax = float(stored.abs().max())
        assert bool(torch.isfinite(stored).all()) and bool(torch.isnan(w['C'][M:]).all())
        # C against the float64 product through the same epilogue
        err = (C.double() - ref).abs()
        if zero is not None:
            assert bool((C[zero] == 0).all()), (name, shape, 'a dropped element is not zero')
            err = torch.where(zero, torch.zeros_like(err), err)
        ratio = float(torch.where(err == 0, torch.zeros_like(err), err / bound).max())   # (a zero saved-tensor element: ref = bound = 0, C must be 0)
        print(f'fp8_ref C accuracy: {name} {shape} run {i}: worst |C - ref| / bound = {ratio:.4f}')
        assert ratio <= 1.0, (name, shape, ratio)
        # the bytes against C as stored by this call; the pitch and the slack rows keep their sentinels
        got = w['q8'][:M, :N]
        _assert_accepted(got, stored, q8_scale, fmt, (name, shape, i))
        assert bool((w['q8'][:M, N:] == SENT).all()) and bool((w['q8'][M:] == SENT).all())
        sat = float(((got & 0x7F) == top).float().mean())
        if i == 0:
            assert len(R.reciprocals(q8_scale)) == 1 and pre < cmax
            assert float(w['am']) == cmax, (name, shape, float(w['am']), cmax)
            # run 2: a scale that is no power of two and saturates about 3 % of the bytes; the amax slot pre-filled above the maximum
            q97 = float(torch.kthvalue(stored.abs().flatten(), int(0.97 * M * N)).values)
            runs.append((_f32(q97 / FMAX[fmt]), 2.0 * cmax))
        else:
            assert len(R.reciprocals(q8_scale)) == 3 and 0.01 < sat < 0.1, (name, shape, sat)
            assert float(w['am']) == pre
        # the no-output form: the same bytes (sentinels included), amax, saved tensor and column sums
        v = _launch(o, shape, flags, fmt, q8_scale, pre, True)
        assert torch.equal(v['q8'], w['q8']) and torch.equal(v['am'], w['am']), (name, shape, i, 'NO_OUT')
        assert bool(torch.isnan(v['C']).all())
        for k in ('aux', 'cs'):
            if k in w:
                assert torch.equal(v[k].view(torch.uint8), w[k].view(torch.uint8)), (name, shape, i, 'NO_OUT', k)
        if 'cs' in w:
            assert bool(torch.isfinite(w['cs']).all())


# ------------------------------------------------------------------------------------------------------------------ 5. small integers
@pytest.mark.parametrize('shape', [R.GEMM_SHAPES[0], R.GEMM_SHAPES[2]], ids=lambda s: 'x'.join(map(str, s)))
@pytest.mark.parametrize('name', ['DH|Q', 'DH|Q|A8'])
def test_epi_quant_out_small_integers(name, shape):
    """operands in {-2 .. 2}, saved tensor in {0, 1, 2}, unit scales: every product and partial sum is exact, C is the bf16 rounding of the exact
    integer and the bytes are `encode` of it, on three launches of the writing and of the no-output form"""
    flags, fmt = R.Q_SETS[name]
    M, N, K = shape
    g = torch.Generator().manual_seed(M + K)
    Ai, Bi = torch.randint(-2, 3, (M, K), generator=g).float(), torch.randint(-2, 3, (N, K), generator=g).float()
    auxi = torch.randint(0, 3, (M, N), generator=g).float()
    one = _f32(1.0)
    o = dict(A=Ai.to(R.TORCH8[E5M2]).view(torch.uint8).cuda(), B=Bi.to(R.TORCH8[E4M3]).view(torch.uint8).cuda(), sa=one, sb=one,
             aux16=auxi.to(BF16).cuda(), aux8=auxi.to(R.TORCH8[E4M3]).view(torch.uint8).cuda())
    exact = (Ai.cuda().double() @ Bi.cuda().double().t()) * auxi.cuda().double()
    assert float(exact.abs().max()) < 2 ** 24
    want_c = exact.to(BF16)
    want_q = R.encode(want_c.float(), fmt)
    assert bool(((want_q & 0x7F) <= R.code_values(fmt).numel() - 1).all())
    want_cs = want_c.double().sum(0)
    assert float(want_c.double().abs().sum(0).max()) < 2 ** 24
    for i in range(3):
        for no_out in (False, True):
            w = _launch(o, shape, flags, fmt, one, 0.0, no_out)
            assert torch.equal(R.canon(w['q8'][:M, :N]), R.canon(want_q)), (name, shape, i, no_out)
            assert bool((w['q8'][:M, N:] == SENT).all()) and bool((w['q8'][M:] == SENT).all())
            assert float(w['am']) == float(want_c.float().abs().max())
            if not no_out:
                assert torch.equal(w['C'][:M], want_c)
            assert torch.equal(w['cs'].double(), want_cs), (name, shape, i, no_out)      # integers below 2^24: exact in f32 in any order
