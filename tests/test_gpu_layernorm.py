"""
The LayerNorm kernels of csrc/rowops.hip (the generic kernel at MAXV = 1, 2, 4, 8, the exact-lane-mapping bf16 kernel at E = 4 .. 32, their EXTRA,
row-pitch and Q8 forms, and reduce_partials_kernel behind every backward) through the C ABI, element by element, against tests/layernorm_ref.py,
whose case lists and bounds tests/test_layernorm_ref.py calibrates on the CPU.  Every output is a NaN-filled slice inside sentinel bands that must
come back intact (the 8-bit copies: 0x7F, the NaN code of both formats, inside bands of 0xA5); no element the contract owns may still hold its
fill; with dropout off dxm must keep its fill; every call runs twice into fresh buffers with equal bits.  mean, rstd, y, dx, dgamma, dbeta and
dcolsum are held to the derived bounds of layernorm_ref and each figure is printed (`RATIO case name value`, the error divided by its bound) before
it is asserted; dxm, the 8-bit copies and the amax are compared by bits (`Q8DIFF case name count` prints the bytes that are the adjacent code).

Worst RATIO per entry point and output, measured on the MI355X over every case of this file (a ratio above 1 is a failure; the bounds were fixed
on the CPU before the first run; cases as `rows x d`):

    entry point, output                        f32                                  bf16
    ecgvit_layernorm_fwd             mean      0.21    65 x 8                       0.016   193 x 72
                                     rstd      0.20    8195 x 264                   0.20    8195 x 264
                                     y         0.50    8195 x 264                   0.50    8195 x 264
    ecgvit_layernorm_fwd_q8          mean                                           0.0075  8195 x 256
                                     rstd                                           0.20    8195 x 2048
                                     y                                              0.50    8195 x 768
    ecgvit_layernorm_bwd             dx        0.51    257 x 72, dres               0.50    4099 x 264, dres
                                     dgamma    0.54    1 x 768                      0.57    1 x 768
                                     dbeta     0.45    3 x 768                      0.0054  61 x 768
    ecgvit_layernorm_bwd_fused       dx        0.51    257 x 72, dres, p 0.1        0.50    65 x 72, p 0.5
                                     dgamma    0.54    1 x 768                      0.57    1 x 768
                                     dbeta     0.45    3 x 768                      0.0054  61 x 768
                                     dcolsum   0.52    5 x 768, p 0.1               0.38    5 x 2040, p 0
    ecgvit_layernorm_bwd_fused_rowpitch dx     0.50    65 x 64, p 0.1               0.50    65 x 2040, p 0.5
                                     dgamma    0.32    5 x 2040, p 0.1              0.38    5 x 2040, p 0.5
                                     dbeta     0.40    5 x 2040, p 0.1              0.0050  65 x 2040, p 0.5
                                     dcolsum   0.46    5 x 2040, p 0.1              0.19    5 x 768, p 0.1
    ecgvit_layernorm_bwd_fused_q8    dx                                             0.50    65 x 2048, p 0.5
                                     dgamma                                         0.36    5 x 768, p 0.5
                                     dbeta                                          0.0047  65 x 2048, p 0.5
                                     dcolsum                                        0.19    5 x 768, p 0.1

(y and dx sit at 0.5 because their bound is floored at one ulp of the element type and a correctly rounded result is half an ulp off; the one-row
dgamma figures are the single f32 rounding of one term against the one-ulp floor.)  dxm had the restatement's bits in every case; of 203 120 640
e4m3 bytes and 5 160 960 e5m2 bytes, none differed from torch's cast, so the adjacent-code allowance was not used; every amax was exact.

One thing the header did not say: ecgvit_layernorm_fwd_q8 returns mean with the bits of ecgvit_layernorm_fwd but rstd may differ in the last place
(the two instantiations fuse their multiply-adds differently), and with it at most a few y per million (2199 of 12 587 520 at 8195 x 1536, where the
constant rows hold y = beta + a rounding residue).  Both stay inside the bounds; include/ecgvit_hip.h now says so, and `test_fwd_q8` prints the count.

Wall time on the MI355X: the 159 items of this file take 5.4 s together; the slowest, test_fwd_by_width[f32-8], takes 0.94 s (it pays the first
launch of the process), the next, test_fwd_q8[bf16-2048-8195], 0.34 s.
"""
import pytest
import torch

import layernorm_ref as R
from layernorm_ref import F32, BF16
from hiputil import ptr, check, stream, lib, hip, bits, Guarded, PAD
from test_gpu_embed_masked_ops import twice, written, same_bits, hold, dropout_apply, raw

pytestmark = pytest.mark.gpu

EINVAL = 1
BYTE_BAND, BYTE_FILL = 0xA5, 0x7F


class GuardedBytes:
    """n bytes of 0x7F (NaN in e4m3fn and in e5m2: no saturating cast produces it) inside a band of 0xA5"""

    def __init__(self, n):
        self.n = n
        self.buf = torch.full((n + 2 * PAD,), BYTE_BAND, dtype=torch.uint8, device='cuda')
        self.t = self.buf[PAD:PAD + n]
        self.t.fill_(BYTE_FILL)
        self.before = self.buf.clone()

    def bands_ok(self):
        return torch.equal(self.buf[:PAD], self.before[:PAD]) and torch.equal(self.buf[PAD + self.n:], self.before[PAD + self.n:])


def untouched(g):
    return torch.equal(raw(g.buf), raw(g.before))


def ids(dtype, *parts):
    return '-'.join([R.dtype_id(dtype)] + [str(p) for p in parts])


class LN:
    """one (rows, d, dtype) problem on the device; `launch` is the raw call of an entry point into the guarded buffers of `outs`"""

    def __init__(self, rows, d, dtype, family='mixed'):
        self.rows, self.d, self.dtype = rows, d, dtype
        c = R.ln_inputs(rows, d, dtype, family)
        self.x, self.gamma, self.beta, self.dy, self.dres = (c[k].cuda() for k in ('x', 'gamma', 'beta', 'dy', 'dres'))
        self.mean32, self.rstd32 = R.stats32(self.x)
        self.cid = ids(dtype, R.shape_id(rows, d))
        self.n = max(rows, 1)

    def outs(self, entry, with_y=True, with_dxm=True, prev=0.0):
        n, d, T = self.n, self.d, self.dtype
        if entry in ('fwd', 'fwd_q8'):
            o = dict(mean=Guarded(n, F32), rstd=Guarded(n, F32))
            if with_y:
                o['y'] = Guarded(n * d, T)
        else:
            floats = max(lib().ecgvit_layernorm_bwd_workspace(n, min(d, R.ROW_MAX_D)) // 4, 3 * d)
            o = dict(dx=Guarded(n * d, T), dgamma=Guarded(d, F32), dbeta=Guarded(d, F32), partial=Guarded(floats, F32))
            if entry != 'bwd':
                o['dcolsum'] = Guarded(d, F32)
                if with_dxm:
                    o['dxm'] = Guarded(n * d, T)
        if entry in ('fwd_q8', 'q8'):
            o['q8'], o['amax'] = GuardedBytes(n * d), Guarded(1, F32)
            o['amax'].t[0] = prev
            o['amax'].before = o['amax'].buf.clone()
        return o

    def launch(self, entry, o, dres=False, p=0.0, pitch=1, scale=None, rows=None, d=None):
        rows, d = self.rows if rows is None else rows, self.d if d is None else d
        l, T, st = lib(), hip.code(self.dtype), stream()
        t = lambda k: ptr(o[k].t) if k in o else None
        if entry == 'fwd':
            return l.ecgvit_layernorm_fwd(ptr(self.x), ptr(self.gamma), ptr(self.beta), t('y'), t('mean'), t('rstd'), rows, d, R.EPS, T, st)
        if entry == 'fwd_q8':
            return l.ecgvit_layernorm_fwd_q8(ptr(self.x), ptr(self.gamma), ptr(self.beta), t('y'), t('mean'), t('rstd'), rows, d, R.EPS, t('q8'), ptr(scale),
                                             t('amax'), st)
        common = (ptr(self.dy), ptr(self.x), ptr(self.gamma), ptr(self.mean32), ptr(self.rstd32), ptr(self.dres) if dres else None, t('dx'), t('dgamma'),
                  t('dbeta'), t('partial'), rows, d)
        if entry == 'bwd':
            return l.ecgvit_layernorm_bwd(*common, T, st)
        if entry == 'fused':
            return l.ecgvit_layernorm_bwd_fused(*common, t('dxm'), t('dcolsum'), float(p), R.SEED, T, st)
        if entry == 'rowpitch':
            return l.ecgvit_layernorm_bwd_fused_rowpitch(*common, t('dxm'), t('dcolsum'), float(p), R.SEED, pitch, T, st)
        assert entry == 'q8'
        return l.ecgvit_layernorm_bwd_fused_q8(*common, t('dxm'), t('dcolsum'), float(p), R.SEED, t('q8'), ptr(scale), t('amax'), st)

    def run(self, entry, skip=('partial',), **kw):
        """the entry point twice into fresh buffers: equal bits, bands intact, everything owned written (dxm is the caller's to judge)"""
        okw = {k: kw.pop(k) for k in ('with_y', 'with_dxm', 'prev') if k in kw}

        def once():
            o = self.outs(entry, **okw)
            check(self.launch(entry, o, **kw), entry)
            return o
        o = twice(once)
        for k, g in o.items():
            if k == 'q8':
                assert not bool((g.t == BYTE_FILL).any()), f'{entry}.{k}: a byte was never written'
            elif k not in skip and k != 'dxm':
                written(f'{entry}.{k}', g.t)
        return o

    # ---- what is held
    def hold_fwd(self, o, entry='layernorm_fwd', tag=''):
        held = R.fwd_held(self.x, self.gamma, self.beta, self.dtype)
        bad = []
        for k in ('mean', 'rstd', 'y'):
            if k in o:
                bad += hold(self.cid + tag, f'{entry}.{k}', o[k].t.view(held[k][0].shape), *held[k])
        assert not bad, (self.cid, bad)

    def hold_bwd(self, o, dres, entry='layernorm_bwd', tag=''):
        held = R.bwd_held(self.dy, self.x, self.gamma, self.mean32, self.rstd32, self.dres if dres else None, self.dtype)
        bad = []
        for k in ('dx', 'dgamma', 'dbeta'):
            bad += hold(self.cid + tag, f'{entry}.{k}', o[k].t.view(held[k][0].shape), *held[k])
        assert not bad, (self.cid, bad)

    def keep(self, p, pitch=1):
        """the mask bits of rows r * pitch, observed through ecgvit_dropout_apply on ones with the same seed"""
        m = dropout_apply(torch.ones(self.rows * pitch, self.d, dtype=self.dtype, device='cuda'), p, R.SEED)
        keep = (m != 0)[::pitch]
        assert keep.shape == (self.rows, self.d) and 0 < int((~keep).sum()) < keep.numel(), 'the mask drops nothing or everything'
        return keep

    def hold_extra(self, o, p, entry, tag='', pitch=1, dxm=None):
        """dxm by bits (or untouched without dropout), dcolsum within its bound of the f64 sum of the values as stored -> those values"""
        dx = o['dx'].t.view(self.rows, self.d)
        if p > 0:
            want = R.dxm_rounded(dx, self.keep(p, pitch), p)
            if 'dxm' in o:
                written(f'{entry}.dxm', o['dxm'].t)
                same_bits(f'{entry}.dxm', o['dxm'].t.view(self.rows, self.d), want)
            stored = want
        else:
            assert 'dxm' not in o or untouched(o['dxm']), f'{entry}: dxm was written with dropout off'
            stored = dx
        bad = hold(self.cid + tag, f'{entry}.dcolsum', o['dcolsum'].t, *R.colsum_held(stored))
        assert not bad, (self.cid, bad)
        return stored


def hold_q8(cid, name, got, stored, scale, fmt):
    want = R.q8_bytes(stored.reshape(-1), scale, fmt)
    n, far = R.q8_differences(got, want)
    print(f'Q8DIFF {cid} {name} {n} of {got.numel()}')
    assert far == 0, f'{name}: {far} bytes are not the wanted code nor the one next to it'
    assert n <= R.Q8_DIFFER_CAP * got.numel(), f'{name}: {n} of {got.numel()} bytes differ'


def delayed_scale(stored, fmt):
    return (stored.float().abs().max() / R.FP8[fmt][1] * R.Q8_DELAY).reshape(1)


def amax_cases(stored):
    top = float(stored.float().abs().max())
    return top, ((0.0, top), (2.0 * top, 2.0 * top))        # (previous, wanted): from 0, and a previous value above the tensor's, which survives


# ------------------------------------------------------------------------------------------------------------------ forward
@pytest.mark.parametrize('dtype,d', [pytest.param(dt, d, id=ids(dt, d)) for dt in R.DTYPES for d in R.WIDTHS])
def test_fwd_by_width(dtype, d):
    """every kernel form and partly live vector, at 5 rows (the second block holds one live wave) and 65"""
    for rows in R.WIDTH_ROWS:
        k = LN(rows, d, dtype)
        k.hold_fwd(k.run('fwd'))


@pytest.mark.parametrize('dtype,d,rows', [pytest.param(dt, d, r, id=ids(dt, d, r)) for dt in R.DTYPES for d in R.ROW_WIDTHS for r in R.ROW_COUNTS])
def test_fwd_by_rows(dtype, d, rows):
    k = LN(rows, d, dtype)
    k.hold_fwd(k.run('fwd'))


@pytest.mark.parametrize('dtype,d', [pytest.param(dt, d, id=ids(dt, d)) for dt in R.DTYPES for d in R.CAPPED_WIDTHS])
def test_fwd_capped_grid(dtype, d):
    """8195 rows on 2048 blocks: three waves take a second row"""
    k = LN(R.CAPPED_FWD_ROWS, d, dtype)
    k.hold_fwd(k.run('fwd'))


# ------------------------------------------------------------------------------------------------------------------ backward
@pytest.mark.parametrize('dtype,d', [pytest.param(dt, d, id=ids(dt, d)) for dt in R.DTYPES for d in R.WIDTHS])
def test_bwd_by_width(dtype, d):
    for rows in R.WIDTH_ROWS:
        k = LN(rows, d, dtype)
        for dres in (False, True):
            k.hold_bwd(k.run('bwd', dres=dres), dres, tag='+dres' if dres else '')


@pytest.mark.parametrize('dtype,d,rows', [pytest.param(dt, d, r, id=ids(dt, d, r)) for dt in R.DTYPES for d in R.ROW_WIDTHS for r in R.ROW_COUNTS])
def test_bwd_by_rows(dtype, d, rows):
    """nparts = 1, 1, 16, 17, 49, 65: both sides of each loop boundary of the reducer, with two outputs (plain) and with three (fused, p = 0.1)"""
    k = LN(rows, d, dtype)
    k.hold_bwd(k.run('bwd', dres=True), True, tag='+dres')
    o = k.run('fused', dres=True, p=0.1)
    k.hold_bwd(o, True, 'layernorm_bwd_fused', '+dres-p0.1')
    k.hold_extra(o, 0.1, 'layernorm_bwd_fused', '+dres-p0.1')


@pytest.mark.parametrize('dtype,d', [pytest.param(dt, d, id=ids(dt, d)) for dt in R.DTYPES for d in R.CAPPED_WIDTHS])
def test_bwd_capped_grid(dtype, d):
    """4099 rows on 1024 blocks: three waves take a second row, the reducer walks 1024 partial rows"""
    k = LN(R.CAPPED_BWD_ROWS, d, dtype)
    k.hold_bwd(k.run('bwd', dres=True), True, tag='+dres')
    o = k.run('fused', dres=True, p=0.1)
    k.hold_bwd(o, True, 'layernorm_bwd_fused', '+dres-p0.1')
    k.hold_extra(o, 0.1, 'layernorm_bwd_fused', '+dres-p0.1')


@pytest.mark.parametrize('dtype,d', [pytest.param(dt, d, id=ids(dt, d)) for dt in R.DTYPES for d in R.FUSED_WIDTHS[dt]])
def test_bwd_fused(dtype, d):
    """the EXTRA form against an independent reference: dx, dgamma, dbeta as the plain backward's; dxm = T(f32(dx as stored) m) by bits with the mask
    ecgvit_dropout_apply draws, untouched at p = 0; dcolsum the sum of what was stored"""
    for rows in R.FUSED_ROWS:
        k = LN(rows, d, dtype)
        for p in R.FUSED_P[dtype]:
            for dres in (False, True):
                tag = f'{"+dres" if dres else ""}-p{p}'
                o = k.run('fused', dres=dres, p=p)
                k.hold_bwd(o, dres, 'layernorm_bwd_fused', tag)
                k.hold_extra(o, p, 'layernorm_bwd_fused', tag)


@pytest.mark.parametrize('dtype,d', [pytest.param(dt, d, id=ids(dt, d)) for dt in R.DTYPES for d in R.FUSED_WIDTHS[dt]])
def test_bwd_fused_rowpitch(dtype, d):
    """row r draws the mask bits of row 7 r of a [7 rows, d] tensor"""
    for rows in R.FUSED_ROWS:
        k = LN(rows, d, dtype)
        for p in R.FUSED_P[dtype]:
            tag = f'+dres-p{p}-pitch{R.PITCH}'
            o = k.run('rowpitch', dres=True, p=p, pitch=R.PITCH)
            k.hold_bwd(o, True, 'layernorm_bwd_fused_rowpitch', tag)
            k.hold_extra(o, p, 'layernorm_bwd_fused_rowpitch', tag, pitch=R.PITCH)


@pytest.mark.parametrize('d', R.Q8_WIDTHS)
def test_bwd_fused_q8(d):
    """the emitting form at every exact-mapping width: everything the fused form returns, by the same bounds and bits, plus g8 = the e5m2 byte of the
    gradient the next stage consumes (dxm under dropout, dx without; as stored) over a delayed scale, and the running amax; dxm given and NULL"""
    entry = 'layernorm_bwd_fused_q8'
    for rows in R.Q8_BWD_ROWS:
        k = LN(rows, d, BF16)
        for p in R.FUSED_P[BF16]:
            tag = f'+dres-p{p}'
            stored = k.hold_extra(k.run('fused', dres=True, p=p), p, 'layernorm_bwd_fused', tag)
            scale = delayed_scale(stored, 'e5m2')
            top, amaxes = amax_cases(stored)
            for with_dxm in (True, False):
                for prev, want in amaxes:
                    t = f'{tag}{"" if with_dxm else "-nodxm"}-prev{prev:.3g}'
                    o = k.run('q8', dres=True, p=p, scale=scale, with_dxm=with_dxm, prev=prev)
                    k.hold_bwd(o, True, entry, t)
                    same_bits(f'{entry}.stored', k.hold_extra(o, p, entry, t), stored)
                    hold_q8(k.cid + t, f'{entry}.g8', o['q8'].t, stored, scale, 'e5m2')
                    assert float(o['amax'].t[0]) == want, (k.cid, t, float(o['amax'].t[0]), want)


# ------------------------------------------------------------------------------------------------------------------ forward, emitting
@pytest.mark.parametrize('d,rows', [pytest.param(d, r, id=f'bf16-{d}-{r}') for d in R.Q8_WIDTHS for r in R.Q8_FWD_ROWS])
def test_fwd_q8(d, rows):
    """mean, rstd and y within the plain forward's bounds, y8 = the e4m3 byte of y as stored over a delayed scale, the running amax; with y NULL, y8
    is the cast of the y the run with y wrote, and mean, rstd, y8 and the amax have the bits of that run"""
    entry = 'layernorm_fwd_q8'
    k = LN(rows, d, BF16)
    plain = k.run('fwd')
    scale = delayed_scale(plain['y'].t, 'e4m3')
    first = k.run('fwd_q8', scale=scale, prev=0.0)
    y = first['y'].t
    differ = bits(y) != bits(plain['y'].t)
    print(f'YBITS {k.cid} y of the emitting forward differs from the plain forward\'s in {int(differ.sum())} of {y.numel()} elements, by at most '
          f'{int((bits(y).int() - bits(plain["y"].t).int()).abs().max())} codes; mean equal {torch.equal(first["mean"].t, plain["mean"].t)}, '
          f'rstd equal {torch.equal(first["rstd"].t, plain["rstd"].t)}')
    top, amaxes = amax_cases(y)
    for with_y in (True, False):
        for prev, want in amaxes:
            t = f'{"" if with_y else "-noy"}-prev{prev:.3g}'
            o = first if (with_y and prev == 0.0) else k.run('fwd_q8', scale=scale, with_y=with_y, prev=prev)
            k.hold_fwd(o, entry, t)
            for name in ('y', 'mean', 'rstd', 'q8'):
                if name in o:
                    assert torch.equal(raw(o[name].t), raw(first[name].t)), f'{entry}.{name}{t}: not the bits of the first run'
            hold_q8(k.cid + t, f'{entry}.y8', o['q8'].t, y, scale, 'e4m3')
            assert float(o['amax'].t[0]) == want, (k.cid, t, float(o['amax'].t[0]), want)


# ------------------------------------------------------------------------------------------------------------------ refusals
def refused(k, entry, **kw):
    okw = {n: kw.pop(n) for n in ('with_y', 'with_dxm') if n in kw}
    o = k.outs(entry, **okw)
    rc = k.launch(entry, o, **kw)
    torch.cuda.synchronize()
    assert rc == EINVAL, (entry, kw, rc)
    for name, g in o.items():
        assert untouched(g), f'{entry} {kw}: refused, yet {name} was written'


@pytest.mark.parametrize('dtype', R.DTYPES, ids=R.dtype_id)
@pytest.mark.parametrize('shape', R.REFUSED_SHAPES, ids=lambda s: R.shape_id(*s))
def test_refused_shapes(dtype, shape):
    """d = 12 (no multiple of 8), d = 2056 (past ECGVIT_ROW_MAX_D), rows = 0: ECGVIT_EINVAL from every entry point, nothing written"""
    rows, d = shape
    k = LN(rows, d, dtype)
    one = torch.ones(1, device='cuda')
    refused(k, 'fwd')
    refused(k, 'bwd', dres=True)
    refused(k, 'fused', dres=True, p=0.1)
    refused(k, 'rowpitch', dres=True, p=0.1, pitch=R.PITCH)
    if dtype == BF16:
        refused(k, 'fwd_q8', scale=one)
        refused(k, 'q8', dres=True, p=0.1, scale=one)


def test_refused_forms():
    """the emitting forms off the exact-mapping widths; a bf16 probability that rounds to no dropout; dropout without a dxm to write"""
    one = torch.ones(1, device='cuda')
    k = LN(5, R.REFUSED_Q8_D, BF16)
    refused(k, 'fwd_q8', scale=one)
    refused(k, 'q8', dres=True, p=0.1, scale=one)
    for d in (72, 256):
        k = LN(5, d, BF16)
        refused(k, 'fused', dres=True, p=R.REFUSED_BF16_P)
        refused(k, 'rowpitch', dres=True, p=R.REFUSED_BF16_P, pitch=R.PITCH)
        for dtype in R.DTYPES:
            k = LN(5, d, dtype)
            refused(k, 'fused', dres=True, p=0.1, with_dxm=False)
            refused(k, 'rowpitch', dres=True, p=0.1, pitch=R.PITCH, with_dxm=False)
    refused(LN(5, 256, BF16), 'q8', dres=True, p=R.REFUSED_BF16_P, scale=one)
