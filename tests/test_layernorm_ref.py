"""
Calibrates tests/layernorm_ref.py on the CPU; no kernel runs here.  The float64 restatement equals torch autograd of F.layer_norm in float64 and two
rows computed by hand; every bound is loose enough for an honest f32 evaluation of the same formulas in torch's own order (ratio <= 1 on every
shared case) and tight enough that the planted errors of the issue exceed it on the smallest and on one wide case; every shared case reaches the
edge it is listed for, by integer arithmetic from the launch constants layernorm_ref restates.

One planted error cannot be seen by a derived bound in f32: two f32 ulps of one element.  The mean alone may be off by (d - 1) roundings in any
order, which is 7 u sum|x| / d at the smallest width, and that passes into every y of the row: `test_two_ulps_of_one_element` holds it for bf16
(where the element's own rounding dominates) and, for f32, on the outputs that are compared by bits (dxm), and prints how many f32 ulps the f32
bound of y leaves room for.
"""
import pytest
import torch
import torch.nn.functional as Fn

import layernorm_ref as R
from layernorm_ref import F64, F32, BF16, EPS

TOL = 1e-12
SMALL, WIDE = (5, 8), (65, 768)


# ------------------------------------------------------------------------------------------------------------------ restatement == autograd, == by hand
@pytest.mark.parametrize('family', R.FAMILIES + ('mixed',))
@pytest.mark.parametrize('shape', [SMALL, (65, 72), WIDE], ids=lambda s: R.shape_id(*s))
def test_restatement_is_autograd_of_layer_norm(family, shape):
    rows, d = shape
    for dtype in R.DTYPES:
        c = R.ln_inputs(rows, d, dtype, family)
        x = c['x'].to(F64).requires_grad_()
        gamma, beta = c['gamma'].to(F64).requires_grad_(), c['beta'].to(F64).requires_grad_()
        y = Fn.layer_norm(x, (d,), gamma, beta, EPS)
        gx, gg, gb = torch.autograd.grad((y * c['dy'].to(F64)).sum(), (x, gamma, beta))
        mean, rstd, yr = R.fwd(c['x'], c['gamma'], c['beta'])
        dx, dgamma, dbeta = R.bwd(c['dy'], c['x'], c['gamma'], mean, rstd)      # (the unrounded statistics: this is a statement about the formulas)
        for got, want in ((yr, y.detach()), (dx, gx), (dgamma, gg), (dbeta, gb)):
            assert float(((got - want).abs() / (1 + want.abs())).max()) <= TOL
        with_res = R.bwd(c['dy'], c['x'], c['gamma'], mean, rstd, c['dres'])[0]
        assert float((with_res - dx - c['dres'].to(F64)).abs().max()) <= TOL
        assert float((mean - c['x'].to(F64).mean(1)).abs().max()) <= TOL
        assert float((rstd ** -2 - EPS - c['x'].to(F64).var(1, unbiased=False)).abs().max()) <= 1e-9 * float(rstd.max() ** -2 + 1)


def test_two_rows_by_hand():
    # x = (1, 3): mean 2, variance 1; eps = 0: rstd 1, xh = (-1, 1)
    mean, rstd, y = R.fwd(torch.tensor([[1.0, 3.0]]), torch.tensor([2.0, -1.0]), torch.tensor([0.5, 0.25]), eps=0.0)
    assert (mean.tolist(), rstd.tolist(), y.tolist()) == ([2.0], [1.0], [[-1.5, -0.75]])
    # x = (2, 4, 4, 4, 5, 5, 7, 9): mean 5, biased variance 32 / 8 = 4 (unbiased: 32 / 7), rstd 1 / 2
    x = torch.tensor([[2.0, 4.0, 4.0, 4.0, 5.0, 5.0, 7.0, 9.0]])
    one, zero = torch.ones(8), torch.zeros(8)
    mean, rstd, y = R.fwd(x, one, zero, eps=0.0)
    assert (mean.tolist(), rstd.tolist()) == ([5.0], [0.5]) and y.tolist() == [[-1.5, -0.5, -0.5, -0.5, 0.0, 0.0, 1.0, 2.0]]
    # dy = e0, gamma = 1: c1 = 1 / 8, c2 = -1.5 / 8, dx = (g - c1 - xh c2) / 2
    dy = torch.zeros(1, 8)
    dy[0, 0] = 1.0
    dx, dgamma, dbeta = R.bwd(dy, x, one, mean.float(), rstd.float())
    assert dx.tolist() == [[0.296875, -0.109375, -0.109375, -0.109375, -0.0625, -0.0625, 0.03125, 0.125]]
    assert dgamma.tolist() == [-1.5] + [0.0] * 7 and dbeta.tolist() == [1.0] + [0.0] * 7
    dres = torch.full((1, 8), 0.5)
    assert R.bwd(dy, x, one, mean.float(), rstd.float(), dres)[0].tolist() == [[v + 0.5 for v in dx[0].tolist()]]
    m32, r32 = R.stats32(x, eps=0.0)
    assert m32.dtype == F32 and r32.dtype == F32 and (m32.tolist(), r32.tolist()) == ([5.0], [0.5])


def test_inputs_are_as_stated():
    for dtype in R.DTYPES:
        for rows, d in (SMALL, WIDE, (65, 2048)):
            c = R.ln_inputs(rows, d, dtype)
            x = c['x'].to(F64)
            assert c['x'].dtype == dtype and c['gamma'].dtype == F32 and c['gamma'][R.ZERO_COL] == 0 and c['gamma'][0] > 0 > c['gamma'][1]
            off, const, spike = x[1], x[2], x[3]
            assert abs(float(off.mean())) / float(off.std()) >= 30 and len(set(off.tolist())) >= min(d, 8) // 2      # still varied after rounding
            assert bool((const == R.CONST).all())
            assert int((spike == R.SPIKE).sum()) == 1
            mean, rstd, _ = R.fwd(c['x'], c['gamma'], c['beta'])
            assert float(rstd[2]) == pytest.approx(EPS ** -0.5, rel=1e-12)
            one = R.ln_inputs(rows, d, dtype, 'constant')['x']
            assert bool((one == R.CONST).all())


def test_inv_keep_and_thresholds():
    assert [R.threshold8(p) for p in (0.0, 0.001, 0.1, 0.5)] == [0, 0, 26, 128]      # 0.001 rounds to no dropout: refused
    assert float(R.inv_keep(0.1, BF16)) == float(torch.tensor(256.0 / 230.0, dtype=F32)) and float(R.inv_keep(0.5, BF16)) == 2.0
    assert float(R.inv_keep(0.1, F32)) == float(torch.tensor(1.0, dtype=F32) / (torch.tensor(1.0, dtype=F32) - torch.tensor(0.1, dtype=F32)))
    assert R.REFUSED_BF16_P * 256 + 0.5 < 1


def test_q8_helpers():
    for fmt, (dt, mx) in R.FP8.items():
        v = torch.tensor([0.0, -0.0, 1.0, -1.0, 3.0 * mx, -3.0 * mx, 1e-9], dtype=BF16)
        b = R.q8_bytes(v, torch.tensor([1.0]), fmt)
        back = b.view(dt).float()
        assert back.tolist()[:6] == [0.0, -0.0, 1.0, -1.0, mx, -mx]                   # saturated, never the NaN code
        assert R.q8_differences(b, b) == (0, 0)
        assert R.q8_differences(torch.tensor([0x00], dtype=torch.uint8), torch.tensor([0x80], dtype=torch.uint8)) == (0, 0)
        assert R.q8_differences(torch.tensor([0x81, 0x31, 0x31], dtype=torch.uint8), torch.tensor([0x00, 0x32, 0x33], dtype=torch.uint8)) == (3, 1)
        assert R.q8_differences(torch.tensor([0x31], dtype=torch.uint8), torch.tensor([0xB1], dtype=torch.uint8)) == (1, 1)     # the wrong sign
        half = R.q8_bytes(torch.tensor([1.0], dtype=BF16), torch.tensor([2.0]), fmt).view(dt).float()
        assert half.tolist() == [0.5]


def test_ulp_of():
    x = torch.tensor([0.0, 1.0, -1.0, 1.5, 2.0, 0.75, 3e-5], dtype=F64)
    inf = torch.tensor(float('inf'))
    for dtype in R.DTYPES:
        want = [0.0] + [float(torch.nextafter(v.abs().to(dtype), inf.to(dtype)).to(F64) - v.abs().to(dtype).to(F64)) for v in x[1:]]
        assert R.ulp_of(x.to(dtype).to(F64), dtype).tolist() == want


# ------------------------------------------------------------------------------------------------------------------ an honest f32 evaluation
def f32_fwd(c, dtype, unbiased=False, ones_col=None, mean_from=None):
    x, gamma = c['x'].float(), c['gamma'].clone()
    d = x.shape[1]
    if ones_col is not None:
        gamma[ones_col] = 1.0
    mean = x.mean(1)
    t = x - mean[:, None]
    rstd = 1.0 / torch.sqrt((t * t).sum(1) / (d - 1 if unbiased else d) + EPS)
    if mean_from is not None:
        t = t.clone()
        t[mean_from[0]] = x[mean_from[0]] - mean[mean_from[1]]
    return mean, rstd, (t * rstd[:, None] * gamma + c['beta']).to(dtype)


def f32_bwd(c, dtype, dres, ones_col=None, skip_rows=None):
    mean32, rstd32 = R.stats32(c['x'])
    gamma = c['gamma'].clone()
    if ones_col is not None:
        gamma[ones_col] = 1.0
    dy = c['dy'].float()
    xh = (c['x'].float() - mean32[:, None]) * rstd32[:, None]
    g = dy * gamma
    v = rstd32[:, None] * (g - g.mean(1, keepdim=True) - xh * (g * xh).mean(1, keepdim=True))
    if dres:
        v = v + c['dres'].float()
    term = dy * xh
    if skip_rows is not None:
        term = term.clone()
        term[skip_rows] = 0
    return v.to(dtype), term.sum(0), dy.sum(0)


def ratios(held, got):
    return {k: R.worst_ratio(got[k], *held[k]) for k in held}


def all_cases():
    s = [(r, d) for d in R.WIDTHS for r in R.WIDTH_ROWS] + [(r, d) for d in R.ROW_WIDTHS for r in R.ROW_COUNTS]
    return s + [(R.CAPPED_BWD_ROWS, d) for d in R.CAPPED_WIDTHS] + [(R.CAPPED_FWD_ROWS, d) for d in R.CAPPED_WIDTHS] + [(65, d) for d in R.Q8_WIDTHS]


@pytest.mark.parametrize('dtype', R.DTYPES, ids=R.dtype_id)
def test_bounds_hold_an_honest_f32_evaluation_on_every_case(dtype):
    worst = {}
    for rows, d in sorted(set(all_cases())):
        c = R.ln_inputs(rows, d, dtype)
        mean, rstd, y = f32_fwd(c, dtype)
        r = ratios(R.fwd_held(c['x'], c['gamma'], c['beta'], dtype), dict(mean=mean, rstd=rstd, y=y))
        m32, r32 = R.stats32(c['x'])
        for dres in (False, True):
            dx, dgamma, dbeta = f32_bwd(c, dtype, dres)
            r.update({k + ('+dres' if dres else ''): v for k, v in ratios(
                R.bwd_held(c['dy'], c['x'], c['gamma'], m32, r32, c['dres'] if dres else None, dtype), dict(dx=dx, dgamma=dgamma, dbeta=dbeta)).items()})
        ref, bound = R.colsum_held(dx)
        r['dcolsum'] = R.worst_ratio(dx.float().sum(0), ref, bound)
        for k, v in r.items():
            assert v <= 1.0, (rows, d, k, v)
            worst[k] = max(worst.get(k, 0.0), v)
    print('honest f32, worst ratio', R.dtype_id(dtype), {k: round(v, 4) for k, v in worst.items()})


@pytest.mark.parametrize('family', R.FAMILIES)
@pytest.mark.parametrize('dtype', R.DTYPES, ids=R.dtype_id)
def test_bounds_hold_an_honest_f32_evaluation_on_every_family(dtype, family):
    for rows, d in (SMALL, WIDE, (65, 2040)):
        c = R.ln_inputs(rows, d, dtype, family)
        mean, rstd, y = f32_fwd(c, dtype)
        r = ratios(R.fwd_held(c['x'], c['gamma'], c['beta'], dtype), dict(mean=mean, rstd=rstd, y=y))
        m32, r32 = R.stats32(c['x'])
        dx, dgamma, dbeta = f32_bwd(c, dtype, True)
        r.update(ratios(R.bwd_held(c['dy'], c['x'], c['gamma'], m32, r32, c['dres'], dtype), dict(dx=dx, dgamma=dgamma, dbeta=dbeta)))
        assert all(v <= 1.0 for v in r.values()), (rows, d, family, r)


# ------------------------------------------------------------------------------------------------------------------ planted errors
PLANT = [pytest.param(dt, s, id=f'{R.dtype_id(dt)}-{R.shape_id(*s)}') for dt in R.DTYPES for s in (SMALL, WIDE)]


def _held(c, dtype, dres=True):
    m32, r32 = R.stats32(c['x'])
    return R.fwd_held(c['x'], c['gamma'], c['beta'], dtype), R.bwd_held(c['dy'], c['x'], c['gamma'], m32, r32, c['dres'] if dres else None, dtype)


def _keep(rows, d, p=0.1, seed=5):
    return torch.rand(rows, d, generator=torch.Generator().manual_seed(seed)) >= p


@pytest.mark.parametrize('dtype,shape', PLANT)
def test_two_ulps_of_one_element(dtype, shape):
    rows, d = shape
    c = R.ln_inputs(rows, d, dtype)
    fh, bh = _held(c, dtype)
    y = f32_fwd(c, dtype)[2]
    dx = f32_bwd(c, dtype, True)[0]
    r, col = rows - 1, d - 1                     # (an ordinary row: rows - 1 = 4 or 64 is of the randn family)
    if dtype == BF16:
        for got, held in ((y, fh['y']), (dx, bh['dx'])):
            off = got.clone()
            off[r, col] = (off[r, col].to(F64) + 2 * R.ulp_of(off[r, col].to(F64), dtype)).to(dtype)
            assert R.worst_ratio(got, *held) <= 1.0 < R.worst_ratio(off, *held)
    else:
        room = (fh['y'][1] / R.ulp_of(fh['y'][0], dtype))[r, col]
        print(f'f32 {rows}x{d}: the bound of y leaves room for {float(room):.1f} ulps at one element of a randn row')
        assert float(room) > 2                   # the reason this error is held by bits, below, and not by the bound
    # the outputs compared by bits see it in either type
    keep = _keep(rows, d)
    dxm = R.dxm_rounded(dx, keep, 0.1)
    k = int(keep[r].nonzero()[0])
    off = dxm.clone()
    off[r, k] = (off[r, k].to(F64) + 2 * R.ulp_of(off[r, k].to(F64), dtype)).to(dtype)
    assert not torch.equal(off, dxm)
    want = (dx.float() * keep * R.inv_keep(0.1, dtype)).to(dtype)
    assert torch.equal(dxm, want) and bool((dxm[~keep] == 0).all())


@pytest.mark.parametrize('dtype,shape', PLANT)
def test_one_column_with_gamma_taken_as_one(dtype, shape):
    rows, d = shape
    c = R.ln_inputs(rows, d, dtype)
    fh, bh = _held(c, dtype)
    for col in (R.ZERO_COL, d - 1):
        assert abs(float(c['gamma'][col]) - 1) > 0.05
        assert R.worst_ratio(f32_fwd(c, dtype, ones_col=col)[2], *fh['y']) > 1.0
        assert R.worst_ratio(f32_bwd(c, dtype, True, ones_col=col)[0], *bh['dx']) > 1.0


@pytest.mark.parametrize('dtype,shape', PLANT)
def test_one_row_normalised_with_its_neighbours_mean(dtype, shape):
    rows, d = shape
    for family in ('mixed', 'randn'):            # (randn: two rows of one family, whose means differ by about 2 / sqrt(d) only)
        c = R.ln_inputs(rows, d, dtype, family)
        fh, _ = _held(c, dtype)
        assert R.worst_ratio(f32_fwd(c, dtype, mean_from=(rows - 1, rows - 2))[2], *fh['y']) > 1.0


@pytest.mark.parametrize('dtype', R.DTYPES, ids=R.dtype_id)
def test_the_last_chunk_of_768_left_at_its_fill(dtype):
    rows, d = WIDE
    assert d == 768
    c = R.ln_inputs(rows, d, dtype)
    fh, bh = _held(c, dtype)
    for got, held in ((f32_fwd(c, dtype)[2], fh['y']), (f32_bwd(c, dtype, True)[0], bh['dx'])):
        for fill in (float('nan'), -777.25):
            off = got.clone()
            off[rows - 1, d - 4:] = fill
            assert not R.worst_ratio(off, *held) <= 1.0          # (NaN: every comparison with it is false)
    nan = f32_fwd(c, dtype)[2].clone()
    nan[0, d - 4:] = float('nan')
    assert bool(torch.isnan(nan.float()).any())


@pytest.mark.parametrize('dtype,shape', PLANT)
def test_dcolsum_over_dx_and_a_mask_of_the_wrong_row(dtype, shape):
    rows, d = shape
    c = R.ln_inputs(rows, d, dtype)
    dx = f32_bwd(c, dtype, True)[0]
    full = _keep(rows * R.PITCH, d)
    keep, wrong = full[::R.PITCH], full[:rows]
    assert keep.shape == (rows, d) and torch.equal(keep[0], wrong[0]) and not torch.equal(keep[1:], wrong[1:])
    dxm = R.dxm_rounded(dx, keep, 0.1)
    ref, bound = R.colsum_held(dxm)
    assert R.worst_ratio(dxm.float().sum(0), ref, bound) <= 1.0
    assert R.worst_ratio(dx.float().sum(0), ref, bound) > 1.0                                    # summed over dx instead of dxm
    assert R.worst_ratio(R.dxm_rounded(dx, wrong, 0.1).float().sum(0), ref, bound) > 1.0
    assert not torch.equal(R.dxm_rounded(dx, wrong, 0.1), dxm)                                    # masked with row r instead of row 7 r
    assert torch.equal(R.dxm_rounded(dx, torch.ones_like(keep), 0.0), dx)                          # p = 0: the multiplier is 1.0f


@pytest.mark.parametrize('dtype,shape', PLANT)
def test_unbiased_variance(dtype, shape):
    rows, d = shape
    c = R.ln_inputs(rows, d, dtype, 'randn')
    fh, _ = _held(c, dtype)
    mean, rstd, y = f32_fwd(c, dtype, unbiased=True)
    assert R.worst_ratio(rstd, *fh['rstd']) > 1.0 and R.worst_ratio(y, *fh['y']) > 1.0
    assert R.worst_ratio(mean, *fh['mean']) <= 1.0


@pytest.mark.parametrize('dtype,shape', PLANT)
def test_dgamma_missing_the_rows_of_one_block(dtype, shape):
    rows, d = shape
    c = R.ln_inputs(rows, d, dtype)
    _, bh = _held(c, dtype)
    assert R.worst_ratio(f32_bwd(c, dtype, True, skip_rows=slice(4, 8))[1], *bh['dgamma']) > 1.0
    assert R.worst_ratio(f32_bwd(c, dtype, True, skip_rows=slice(0, 4))[1], *bh['dgamma']) > 1.0


# ------------------------------------------------------------------------------------------------------------------ every case reaches its edge
def test_widths_reach_their_kernel_forms():
    assert R.WIDTHS == [8, 64, 72, 256, 264, 512, 520, 768, 1024, 1032, 1536, 2040, 2048]
    assert (R.WV[F32], R.WV[BF16]) == (64 * 4, 64 * 8) == (256, 512)
    maxv32 = {8: 1, 64: 1, 72: 1, 256: 1, 264: 2, 512: 2, 520: 4, 768: 4, 1024: 4, 1032: 8, 1536: 8, 2040: 8, 2048: 8}
    for d in R.WIDTHS:
        assert d % 8 == 0 and d <= R.ROW_MAX_D and R.kernel_form(d, F32) == ('generic', maxv32[d])
        assert (maxv32[d] // 2) * R.WV[F32] < d or maxv32[d] == 1                 # the smaller power of two would not hold the row ...
    assert {d for d in R.WIDTHS if -(-d // R.WV[F32]) < maxv32[d]} == {520, 768, 1032, 1536}   # ... and these run with wholly dead vector indices (3 of 4, 3 of 4, 5 of 8, 6 of 8 live)
    partly32 = {8: 2, 72: 18, 264: 2, 520: 2, 1032: 2, 2040: 62}
    for d, lanes in partly32.items():
        assert R.last_vector_lanes(d, F32) == lanes < 64
    for d in (256, 512, 768, 1024, 1536, 2048):
        assert R.last_vector_lanes(d, F32) == 64
    fit = {256: 4, 512: 8, 768: 12, 1024: 16, 1536: 24, 2048: 32}
    generic16 = {8: 1, 64: 1, 72: 1, 264: 1, 520: 2, 1032: 4, 2040: 4}
    assert sorted(list(fit) + list(generic16)) == R.WIDTHS
    assert tuple(fit.values()) == R.FIT_E and tuple(fit) == R.Q8_WIDTHS
    for d, e in fit.items():
        assert R.kernel_form(d, BF16) == ('fit', e) and d == 64 * e
    assert [(e // 8, e % 8 // 4) for e in R.FIT_E] == [(0, 1), (1, 0), (1, 1), (2, 0), (3, 0), (4, 0)]   # (16-byte chunks, the 8-byte tail): 4 is tail only
    for d, mv in generic16.items():
        assert R.kernel_form(d, BF16) == ('generic', mv)
    assert {d: R.last_vector_lanes(d, BF16) for d in generic16} == {8: 1, 64: 8, 72: 9, 264: 33, 520: 1, 1032: 1, 2040: 63}
    assert R.kernel_form(1280, BF16)[0] == 'generic'                              # a multiple of 256 outside the E list is not exact-mapped
    for rows in R.WIDTH_ROWS:
        assert R.second_trip_waves(rows, R.FWD_CAP) == 0 == R.second_trip_waves(rows, R.BWD_CAP)
    assert R.WIDTH_ROWS == (5, 65) and R.grid(5, R.BWD_CAP) == 2 and 2 * R.WAVES - 5 == 3 and 5 - R.WAVES == 1      # the second block: one live wave
    assert R.nparts(65) == 17


def test_row_counts_reach_the_reducer_edges():
    assert R.ROW_COUNTS == [1, 3, 61, 65, 193, 257] and R.ROW_WIDTHS == (72, 768)
    assert [R.nparts(r) for r in R.ROW_COUNTS] == [1, 1, 16, 17, 49, 65]
    assert (R.RED_SLICES, R.RED_STRIDE) == (16, 64)
    T = R.reducer_trips
    assert T(1, 0) == (0, 1) and all(T(1, s) == (0, 0) for s in range(1, 16))            # one partial row: fifteen idle slices
    assert all(T(16, s) == (0, 1) for s in range(16))                                    # exactly one row per slice
    assert T(17, 0) == (0, 2) and all(T(17, s) == (0, 1) for s in range(1, 16))          # slice 0 takes a second single trip
    assert all(T(48, s) == (0, 3) for s in range(16))                                    # (48: still no unrolled trip)
    assert T(49, 0) == (1, 0) and all(T(49, s) == (0, 3) for s in range(1, 16))          # 49: the first unrolled trip, in slice 0 only
    assert all(T(64, s) == (1, 0) for s in range(16))
    assert T(65, 0) == (1, 1) and all(T(65, s) == (1, 0) for s in range(1, 16))          # 65: an unrolled trip and then a single one
    assert all(T(1024, s) == (16, 0) for s in range(16))
    for n in (1, 16, 17, 48, 49, 64, 65, 1024):                                          # every partial row is read exactly once
        assert sum(4 * a + b for a, b in (T(n, s) for s in range(16))) == n
    assert R.kernel_form(72, BF16)[0] == 'generic' and R.kernel_form(768, BF16) == ('fit', 12)


def test_capped_grids_take_a_second_row():
    assert (R.FWD_CAP, R.BWD_CAP, R.WAVES) == (2048, 1024, 4)
    assert R.CAPPED_BWD_ROWS == 4099 and R.nparts(4099) == 1024 and R.nparts(4096) == 1024 and R.nparts(4092) == 1023
    assert R.second_trip_waves(4099, R.BWD_CAP) == 3 and R.second_trip_waves(4096, R.BWD_CAP) == 0
    assert R.CAPPED_FWD_ROWS == 8195 and R.grid(8195, R.FWD_CAP) == 2048 and R.grid(8188, R.FWD_CAP) == 2047
    assert R.second_trip_waves(8195, R.FWD_CAP) == 3 and R.second_trip_waves(8192, R.FWD_CAP) == 0
    assert R.CAPPED_WIDTHS == (256, 264)
    assert R.kernel_form(256, BF16) == ('fit', 4) and R.kernel_form(256, F32) == ('generic', 1)
    assert R.kernel_form(264, BF16) == ('generic', 1) and R.kernel_form(264, F32) == ('generic', 2)
    assert max(R.CAPPED_FWD_ROWS * d * 4 for d in R.CAPPED_WIDTHS) < 9e6                  # the largest tensor of these cases
    assert R.Q8_FWD_ROWS == (5, 65, 8195) and R.CAPPED_FWD_ROWS * max(R.Q8_WIDTHS) * 2 < 34e6


def test_fused_cases_hold_one_width_of_each_form():
    assert [R.kernel_form(d, BF16) for d in R.FUSED_WIDTHS[BF16]] == [('generic', 1), ('fit', 4), ('generic', 2), ('fit', 12), ('fit', 24), ('generic', 4)]
    assert [R.kernel_form(d, F32)[1] for d in R.FUSED_WIDTHS[F32]] == [1, 2, 4, 8]
    assert all(d in R.WIDTHS for dt in R.DTYPES for d in R.FUSED_WIDTHS[dt])
    assert R.FUSED_P == {F32: (0.0, 0.1), BF16: (0.0, 0.1, 0.5)}
    assert [R.threshold8(p) for p in R.FUSED_P[BF16]] == [0, 26, 128] and R.threshold8(0.1) < 128 <= R.threshold8(0.5)   # both branches of quad_keepbits
    assert R.PITCH == 7 and R.FUSED_ROWS == (5, 65)
    for dt in R.DTYPES:                                                                    # the row-pitch counter stays below 2^32
        assert max(R.FUSED_ROWS) * R.PITCH * max(R.FUSED_WIDTHS[dt]) < 2 ** 32
    assert R.REFUSED_SHAPES == [(5, 12), (5, 2056), (0, 64)] and 12 % 8 and 2056 % 8 == 0 and 2056 > R.ROW_MAX_D
    assert R.kernel_form(R.REFUSED_Q8_D, BF16)[0] == 'generic' and R.threshold8(R.REFUSED_BF16_P) == 0
