"""CPU: the table encoder of tests/fp8_ref.py against torch's float8 casts and against the format definitions, the per-element criterion
against planted wrong encoders, and the case lists against the launch geometry they are listed for."""
import math

import pytest
import torch

import fp8_ref as R
from fp8_ref import E4M3, E5M2, F32, F64, FMAX, FORMATS


def _recips3(scale):
    """r and its two f32 neighbours, also at a power of two: the encoder is held under all three whatever the criterion admits"""
    r = torch.ones((), dtype=F32) / torch.tensor(scale, dtype=F32)
    return [float(r), float(torch.nextafter(r, torch.zeros((), dtype=F32))), float(torch.nextafter(r, torch.full((), math.inf, dtype=F32)))]


@pytest.mark.parametrize('fmt', FORMATS)
def test_code_tables_follow_the_format_definitions(fmt):
    t = R.code_values(fmt)
    assert t.numel() == {E4M3: 127, E5M2: 124}[fmt] and float(t[0]) == 0.0 and float(t[-1]) == FMAX[fmt]
    dec = torch.arange(t.numel(), dtype=torch.uint8).view(R.TORCH8[fmt]).to(F64)      # torch's decoder of the same bytes
    assert torch.equal(dec, t)
    assert float(t[1]) == {E4M3: 2.0 ** -9, E5M2: 2.0 ** -16}[fmt]                     # the smallest subnormal


@pytest.mark.parametrize('fmt', FORMATS)
@pytest.mark.parametrize('scale', R.SWEEP_SCALES)
def test_encode_matches_torch_cpu_cast_on_every_bf16_pattern(fmt, scale):
    x = R.all_bf16()
    for r in _recips3(scale):
        p = R.scaled(x, r, fmt)
        got, want = R.encode(p, fmt), p.to(R.TORCH8[fmt]).view(torch.uint8)
        assert torch.equal(got, want), (fmt, scale, r, int((got != want).sum()))
    rs = R.reciprocals(scale)
    pow2 = math.frexp(scale)[0] == 0.5
    assert len(rs) == (1 if pow2 else 3)
    w = R.want_bytes(x, scale, fmt)
    if pow2:      # exact ties exist and have exactly one accepted byte
        p = R.scaled(x, rs[0], fmt).to(F64).abs()
        t = R.code_values(fmt)
        mids = (t[1:] + t[:-1]) / 2
        assert int(torch.isin(p, mids).sum()) > 100
    else:         # the three reciprocals disagree on a handful of patterns at most
        assert int((w != w[0]).any(0).sum()) <= 2


def _sweep(fmt):
    """(f32 values, expected bytes) by the format's definition, not by `encode`: for every pair of adjacent codes the two codes, their midpoint and
    one f32 ulp to either side of it; the subnormal range on a fine grid; max, one ulp beyond, inf; all of it with both signs"""
    t = R.code_values(fmt)
    vals, want = [], []
    for b in range(t.numel() - 1):
        lo, hi = float(t[b]), float(t[b + 1])
        mid = torch.tensor((lo + hi) / 2, dtype=F32)
        assert float(mid) == (lo + hi) / 2
        below, above = torch.nextafter(mid, torch.zeros((), dtype=F32)), torch.nextafter(mid, torch.full((), math.inf, dtype=F32))
        vals += [lo, hi, float(mid), float(below), float(above)]
        want += [b, b + 1, b if b % 2 == 0 else b + 1, b, b + 1]
    # the subnormal range: step s, values k s / 16 for k = 0 .. 16 (2^mbits + 1): nearest multiple of s, ties (k = 8 mod 16) to the even multiple
    s = float(t[1])
    nsub = 2 ** R._DEF[fmt][1]
    for k in range(16 * (nsub + 1) + 1):
        q, rem = divmod(k, 16)
        vals.append(k * s / 16)
        want.append(q + (1 if rem > 8 or (rem == 8 and q % 2 == 1) else 0))
    top = t.numel() - 1
    mx = torch.tensor(FMAX[fmt], dtype=F32)
    vals += [float(mx), float(torch.nextafter(mx, torch.full((), math.inf, dtype=F32))), math.inf, float(torch.finfo(F32).max), float(torch.finfo(F32).tiny) / 4, 0.0]
    want += [top, top, top, top, 0, 0]
    v = torch.tensor(vals, dtype=F64).to(F32)
    assert torch.equal(v.to(F64), torch.tensor(vals, dtype=F64))                        # every value of the sweep is an f32 value
    w = torch.tensor(want, dtype=torch.uint8)
    return torch.cat([v, -v]), torch.cat([w, w + 128])


@pytest.mark.parametrize('fmt', FORMATS)
def test_encode_on_midpoints_neighbours_subnormals_and_saturation(fmt):
    v, want = _sweep(fmt)
    got = R.encode(v, fmt)
    bad = (got != want).nonzero().flatten()
    assert bad.numel() == 0, [(float(v[i]), int(got[i]), int(want[i])) for i in bad[:5]]
    assert int(R.encode(torch.tensor([-0.0]), fmt)) == 0x80 and int(R.canon(R.encode(torch.tensor([-0.0]), fmt))) == 0
    assert bool(R.accepts(torch.tensor([0x00, 0x80], dtype=torch.uint8), torch.tensor([-0.0, 0.0]), 1.0, fmt).all())


# ------------------------------------------------------------------------------------------------------------------ planted wrong encoders
def _neighbours(p, fmt):
    t = R.code_values(fmt)
    a = p.to(F64).abs().clamp(max=FMAX[fmt])
    hi = torch.searchsorted(t, a.contiguous()).clamp(max=t.numel() - 1)
    lo = (hi - 1).clamp(min=0)
    lo = torch.where(t[hi] == a, hi, lo)                 # an exact code is its own neighbour on both sides
    return t, a, lo, hi


def _signed(b, p):
    return (b + 128 * torch.signbit(p).to(b.dtype)).to(torch.uint8)


def wrong_encoder(name, x, scale, fmt):
    """bytes a subtly wrong emitter would give for the bf16 values x under `scale`"""
    r = R.reciprocals(scale)[0]
    p = R.scaled(x, r, fmt)
    right = R.encode(p, fmt)
    t, a, lo, hi = _neighbours(p, fmt)
    mid = (t[lo] + t[hi]) / 2
    tie = (a == mid) & (lo != hi)
    if name == 'truncation':
        return _signed(lo, p)
    if name == 'round_half_up':                          # ties towards +inf
        return torch.where(tie, _signed(torch.where(torch.signbit(p), lo, hi), p), right)
    if name == 'round_half_away':                        # ties away from zero
        return torch.where(tie, _signed(hi, p), right)
    if name == 'flush_subnormals':
        sub = (right & 0x7F) < 2 ** R._DEF[fmt][1]
        return torch.where(sub, right & 0x80, right)
    if name == 'no_saturation':                          # the conversion of the unclamped product
        raw = (x.to(F32).to(F64) * r).to(F32)
        t_last, t_prev = float(t[-1]), float(t[-2])
        over = raw.abs().to(F64) >= t_last + (t_last - t_prev) / 2
        return torch.where(over, _signed(torch.full_like(lo, R.OVERFLOW_BYTE[fmt]), raw), right)
    if name == 'coarse_reciprocal':                      # a reciprocal held to bf16's half ulp: the finest error 65 282 bf16 patterns resolve at
        return R.encode(R.scaled(x, float(torch.tensor(r * (1 + 2.0 ** -8), dtype=F32)), fmt), fmt)   # every scale (two ulps: the test below)
    if name == 'neighbouring_element':
        return torch.roll(right, 1)
    raise KeyError(name)


WRONG = ('truncation', 'round_half_up', 'round_half_away', 'flush_subnormals', 'no_saturation', 'coarse_reciprocal', 'neighbouring_element')


@pytest.mark.parametrize('fmt', FORMATS)
@pytest.mark.parametrize('name', WRONG)
def test_criterion_refuses_wrong_encoders(name, fmt):
    """on the exhaustive input every planted encoder has refused bytes, at a power-of-two scale (ties: zero slack) and at one that is none; a
    coarse reciprocal is asked for at the scales that are no power of two (at a power of two no kernel's division can miss)"""
    x = R.all_bf16()
    for scale in (1.0, 0.25, 0.0137, 17.3):
        assert bool(R.accepts(R.encode(R.scaled(x, R.reciprocals(scale)[0], fmt), fmt), x, scale, fmt).all())     # the right encoder passes
        if name in ('round_half_up', 'round_half_away') and math.frexp(scale)[0] != 0.5:
            continue                                     # ties need an exact product
        if name == 'coarse_reciprocal' and math.frexp(scale)[0] == 0.5:
            continue
        ok = R.accepts(wrong_encoder(name, x, scale, fmt), x, scale, fmt)
        assert not bool(ok.all()), (name, fmt, scale)
        refused = int((~ok).sum())
        floor = {'truncation': 1000, 'flush_subnormals': 100, 'no_saturation': 1000, 'neighbouring_element': 100}.get(name, 1)
        assert refused >= floor, (name, fmt, scale, refused)


@pytest.mark.parametrize('fmt', FORMATS)
@pytest.mark.parametrize('scale', [0.0137, 0.7, 17.3])
def test_criterion_refuses_a_reciprocal_two_ulps_off(fmt, scale):
    """f32 input laid around every rounding boundary -- f32(midpoint x scale) and its 8 f32 neighbours to either side, both signs: the correctly
    rounded reciprocal and its two neighbours are accepted everywhere, the next one out (two ulps, either way) is refused"""
    t = R.code_values(fmt)
    base = ((t[1:] + t[:-1]) / 2 * scale).to(F32)
    vs, up, dn = [base], base, base
    for _ in range(8):
        up, dn = torch.nextafter(up, torch.full_like(up, math.inf)), torch.nextafter(dn, torch.zeros_like(dn))
        vs += [up, dn]
    v = torch.cat(vs)
    v = torch.cat([v, -v])
    r, lo, hi = (torch.tensor(q, dtype=F32) for q in R.reciprocals(scale))
    for q in (r, lo, hi):
        assert bool(R.accepts(R.encode(R.scaled(v, float(q), fmt), fmt), v, scale, fmt).all())
    for q in (torch.nextafter(lo, torch.zeros((), dtype=F32)), torch.nextafter(hi, torch.full((), math.inf, dtype=F32))):
        refused = int((~R.accepts(R.encode(R.scaled(v, float(q), fmt), fmt), v, scale, fmt)).sum())
        assert refused >= 50, (fmt, scale, refused)


@pytest.mark.parametrize('fmt', FORMATS)
def test_zero_and_negative_scales_accept_zero_codes_only(fmt):
    x = R.all_bf16()
    x = torch.where(torch.isinf(x), torch.zeros_like(x), x)
    for scale in R.ZERO_CODE_SCALES:
        assert R.reciprocals(scale) == [0.0]
        w = R.want_bytes(x, scale, fmt)
        assert w.shape[0] == 1 and bool((R.canon(w) == 0).all())
        assert not bool(R.accepts(torch.full((x.numel(),), 1, dtype=torch.uint8), x, scale, fmt).any())


# ------------------------------------------------------------------------------------------------------------------ the case lists reach their edges
def test_counts_reach_the_tail_branch_and_the_second_trip():
    assert all(c % 8 == 0 for c in R.COUNTS)
    assert {c for c in R.COUNTS if R.takes_tail(c)} == {8, 24, 4088, 4104, R.GRID_CAP_ONE * R.BLOCK_ELEMS + 24}
    assert not R.takes_tail(16)
    assert [R.grid_blocks(c, 1) for c in R.COUNTS] == [1, 1, 1, 1, 1, R.GRID_CAP_ONE]
    assert [R.second_trip(c, 1) for c in R.COUNTS] == [0, 0, 0, 0, 8, 24]              # 8: lane 0's second trip is the tail; 24: a whole step for lane 0, the tail for lane 1


def test_segment_table_has_gaps_tails_and_a_capped_grid():
    end = 0
    for off, cnt in R.SEGMENTS:
        assert off % 16 == 0 and cnt % 8 == 0 and off >= end + 16                       # a gap of sentinels in front of every segment
        end = off + cnt
    assert R.SEG_TOTAL >= end + 16
    cnts = [c for _, c in R.SEGMENTS]
    assert 8 in cnts and sum(R.takes_tail(c) for c in cnts) >= 3 and len(set(cnts)) == len(cnts)
    nmax = max(cnts)
    assert nmax == R.SEG_LONG and R.grid_blocks(nmax, len(cnts)) == R.GRID_CAP_SEG
    assert R.second_trip(nmax, len(cnts)) == 3 * R.BLOCK_ELEMS + 40 and R.takes_tail(nmax)
    assert len(R.SEG_SCALES) == len(R.SEGMENTS)


def test_gemm_cases_reach_their_tile_edges():
    (m0, n0, k0), (m1, n1, k1), (m2, n2, k2) = R.GEMM_SHAPES
    for M, N, K in R.GEMM_SHAPES:
        assert M >= 2048 and N >= 128 and N % 8 == 0 and K >= 384 and K % 128 == 0
    assert m0 % R.GEMM_TILE == 3 and n0 < R.GEMM_TILE
    assert m1 % R.GEMM_TILE == 0 and n1 % R.GEMM_TILE == 8
    assert R.n_tiles(m2, n2) == 297 > 256 and m2 % R.GEMM_TILE and n2 % R.GEMM_TILE
    assert len(R.Q_SETS) == 6 and all(fl & R.EPI_Q and not fl & R.EPI_NO for fl, _ in R.Q_SETS.values())
    assert round(256 * R.GEMM_P) == 64
    x = torch.linspace(-6, 6, 200001, dtype=F64)
    g = 0.5 * (1 + torch.erf(x / 2 ** 0.5)) + x * torch.exp(-0.5 * x * x) / (2 * math.pi) ** 0.5
    assert float(g.abs().max()) < R.GELU_LIP
