"""
Calibrates tests/embed_ref.py on the CPU; no kernel runs here.  The float64 backward functions equal torch.autograd.grad of the forward ones, the
L1 gradient equals autograd's off the ties and is exactly 0 on them, the rounded-once restatements lie within one rounding of the float64 ones,
every shared case fits its stated memory, and every shared case reaches the edge it is listed for (trip counts, group counts, nb / per: plain
integer arithmetic, so a case that stops reaching its edge fails here and not silently on the device).
"""
import pytest
import torch

import embed_ref as R
from embed_ref import F64, F32, BF16, VN, ESIZE

TOL = 1e-12


def _f64(*shape, seed):
    return torch.randn(*shape, dtype=F64, generator=torch.Generator().manual_seed(seed))


# ------------------------------------------------------------------------------------------------------------------ backward == autograd
@pytest.mark.parametrize('s', R.SHAPES, ids=R.shape_id)
def test_embed_bwd_is_autograd(s):
    B, n, d = s
    tok, cls, pos = (_f64(B * n, d, seed=1).requires_grad_(), _f64(d, seed=2).requires_grad_(), _f64(n + 1, d, seed=3).requires_grad_())
    dX = _f64(B, n + 1, d, seed=4)
    X = R.embed(tok, cls, pos, B, n, d)
    assert X.shape == (B, n + 1, d)
    want = torch.autograd.grad((X * dX).sum(), (tok, cls, pos))
    dtok, dcls, dpos = R.embed_bwd(dX)
    assert dpos.shape == (n + 1, d)
    for got, w in zip((dtok.reshape(B * n, d), dcls, dpos), want):
        assert float((got - w).abs().max()) <= TOL
    assert torch.equal(dpos[0], dcls)


@pytest.mark.parametrize('s', R.SHAPES, ids=R.shape_id)
def test_mask_embed_bwd_is_autograd(s):
    B, n, d = s
    for m in R.mask_counts(n):
        idx = R.mask_index(B, n, m)
        tok, mt, pos = (_f64(B * n, d, seed=5).requires_grad_(), _f64(d, seed=6).requires_grad_(), _f64(n + 1, d, seed=7).requires_grad_())
        dX = _f64(B, n, d, seed=8)
        X, mask = R.mask_embed(tok, mt, pos, idx, B, n, m, d)
        assert X.shape == (B, n, d) and mask.shape == (B, n) and bool((mask.sum(1) == m).all())
        g_tok, g_mt, g_pos = torch.autograd.grad((X * dX).sum(), (tok, mt, pos), allow_unused=True)
        g_mt = torch.zeros(d, dtype=F64) if g_mt is None else g_mt
        dtok, dmasked, dpos = R.mask_embed_bwd(dX, mask)
        assert dpos.shape == (n + 1, d) and float(dpos[0].abs().max()) == 0.0
        assert float((dtok.reshape(B * n, d) - g_tok).abs().max()) <= TOL
        assert float((dmasked.sum((0, 1)) - g_mt).abs().max()) <= TOL
        assert float((dpos - g_pos).abs().max()) <= TOL
        assert torch.equal(dtok + dmasked, dX) and bool((dtok[mask] == 0).all()) and bool((dmasked[~mask] == 0).all())


@pytest.mark.parametrize('c', R.L1_CASES, ids=lambda c: R.shape_id(c['case']))
@pytest.mark.parametrize('gscalar', [None, R.L1_GSCALAR])
def test_l1_is_autograd_off_the_ties(c, gscalar):
    rows, width, ld = c['case']
    for dtype in R.DTYPES:
        pred, target = R.l1_inputs(rows, width, ld, dtype)
        p = pred.to(F64).requires_grad_()
        loss, dpred = R.l1(p, target, rows, width, ld, gscalar)
        (g,) = torch.autograd.grad(loss * (1.0 if gscalar is None else gscalar), p)
        tie = (pred[:, :width].float() == target[:, :width].float())
        assert not bool((~tie).any()) or float((dpred.detach() - g[:, :width])[~tie].abs().max()) <= TOL
        assert bool((dpred[tie] == 0).all())
        assert bool((g[:, width:] == 0).all())                   # only the first `width` columns of a row are read
        assert not bool(torch.isnan(loss)) and float(loss.detach()) >= 0
        # the bit-level statement of dpred is the float64 one rounded once
        r = R.l1_dpred_rounded(pred, target, rows, width, ld, gscalar, dtype)
        u = 2.0 ** -24 + (2.0 ** -8 if dtype == BF16 else 0.0)      # the f32 quotient, then the element type (bf16: 8 significant bits)
        assert bool(((r.to(F64) - dpred).abs() <= u * dpred.abs()).all()) and bool((r[tie] == 0).all())


def test_l1_inputs_are_as_stated():
    for c in R.L1_CASES:
        rows, width, ld = c['case']
        for dtype in R.DTYPES:
            pred, target = R.l1_inputs(rows, width, ld, dtype)
            assert bool(torch.isnan(pred[:, width:]).all()) and bool(torch.isnan(target[:, width:]).all())
            p, t = pred[:, :width].float(), target[:, :width].float()
            assert not bool(torch.isnan(p).any() | torch.isnan(t).any())
            diff = (p - t)[p != t]
            assert bool((diff.abs() >= 2.0 ** -126).all())          # no subnormal difference: its sign is exact
            if rows * width >= 2048:
                assert 0.07 < float((p == t).float().mean()) < 0.13


# ------------------------------------------------------------------------------------------------------------------ the rounded restatements
@pytest.mark.parametrize('dtype', R.DTYPES, ids=R.dtype_id)
def test_rounded_restatements_are_one_rounding_from_float64(dtype):
    u = 2.0 ** -24 if dtype == F32 else 2.0 ** -8 + 2.0 ** -24    # (bf16: the f32 add, then the rounding to 8 significant bits)
    for B, n, d in R.SHAPES:
        tok, cls, pos, _ = R.embed_inputs(B, n, d, dtype)
        ref = R.embed(tok, cls, pos, B, n, d)
        got = R.embed_rounded(tok, cls, pos, B, n, d, dtype)
        assert got.dtype == dtype and bool(((got.to(F64) - ref).abs() <= u * ref.abs()).all())
        tok, mt, pos, _ = R.embed_inputs(B, n, d, dtype, cls_row=False)
        for m in R.mask_counts(n):
            ref, mask = R.mask_embed(tok, mt, pos, R.mask_index(B, n, m), B, n, m, d)
            got = R.mask_embed_rounded(tok, mt, pos, mask, B, n, d, dtype)
            assert bool(((got.to(F64) - ref).abs() <= u * ref.abs()).all())


@pytest.mark.parametrize('dtype', R.DTYPES, ids=R.dtype_id)
def test_dpos_bound_holds_a_sequential_f32_sum_and_not_a_dropped_record(dtype):
    """the bound admits f32 sums in two different orders and rejects a sum that misses one record (B >= 2)"""
    for B, n, d in R.SHAPES:
        dX = R.embed_inputs(B, n, d, dtype)[3].reshape(B, n + 1, d)
        ref = R.embed_bwd(dX)[2]
        bound = R.dpos_bound(dX, ref)
        fwd, rev = torch.zeros(n + 1, d), torch.zeros(n + 1, d)
        for b in range(B):
            fwd += dX[b].float()
            rev += dX[B - 1 - b].float()
        assert R.worst_ratio(fwd, ref, bound) <= 1.0 and R.worst_ratio(rev, ref, bound) <= 1.0
        if B >= 2:
            assert R.worst_ratio(fwd - dX[B - 1].float(), ref, bound) > 1.0


def test_ulp32():
    x = torch.tensor([0.0, 1.0, -1.0, 1.5, 2.0, 0.75, 3e-5], dtype=F64)
    want = [0.0] + [float(torch.nextafter(v.abs().float(), torch.tensor(float('inf'))) - v.abs().float()) for v in x[1:]]
    assert R.ulp32(x).tolist() == want


# ------------------------------------------------------------------------------------------------------------------ memory
def test_every_case_fits_its_stated_memory():
    for dtype in R.DTYPES:
        for B, n, d in R.SHAPES:
            assert 5 * B * (n + 1) * d * ESIZE[dtype] <= R.SMALL_MB * R.MB
        for shapes, rows in ((R.embed_shapes(dtype), 1), (R.mask_shapes(dtype), 0)):
            B, n, d, fwd_only = shapes[-1]
            assert fwd_only and (B * n * d + B * (n + rows) * d) * ESIZE[dtype] < R.STRIDE_MB * R.MB
    for f in R.ROW_FORMS:
        B, n, m, width, ld_in, ld_out = f['form']
        for dtype in f['dtypes']:
            gather = B * n * ld_in + B * m * ld_out
            scatter = B * m * ld_in + B * n * ld_out
            assert max(gather, scatter) * ESIZE[dtype] <= f['mb'] * R.MB
    for c in R.L1_CASES:
        rows, width, ld = c['case']
        assert 3 * rows * ld * 4 <= c['mb'] * R.MB


# ------------------------------------------------------------------------------------------------------------------ every case reaches its edge
def test_shapes_reach_their_edges():
    assert R.SHAPES == [(1, 1, 8), (32, 7, 64), (33, 5, 72), (65, 3, 264)]
    B, n, d = R.SHAPES[0]
    assert (B, n) == (1, 1) and d // VN[BF16] == 1 and d // VN[F32] == 2
    B, n, d = R.SHAPES[1]
    assert all(R.batch_trips(B, lane) == 1 for lane in range(R.BATCH_LANES)) and d == 64
    B, n, d = R.SHAPES[2]
    assert R.batch_trips(B, 0) == 2 and all(R.batch_trips(B, lane) == 1 for lane in range(1, R.BATCH_LANES))
    assert (d // VN[F32], d // VN[BF16]) == (18, 9)
    assert R.column_groups(d, F32) == (3, 2) and R.column_groups(d, BF16) == (2, 1)
    B, n, d = R.SHAPES[3]
    assert R.batch_trips(B, 0) == 3 and all(R.batch_trips(B, lane) == 2 for lane in range(1, R.BATCH_LANES))
    assert (d // VN[F32], d // VN[BF16]) == (66, 33)
    assert R.column_groups(d, F32) == (9, 2) and R.column_groups(d, BF16) == (5, 1)
    for s in R.SHAPES:
        assert s[2] % 8 == 0 and all(R.stride_trips(s[0] * (s[1] + 1) * (s[2] // VN[dt])) == 1 for dt in R.DTYPES)
    for s in R.DROPOUT_SHAPES + [R.VARLEN_CROSS_SHAPE]:
        assert s in R.SHAPES and R.batch_trips(s[0]) >= 2 and R.column_groups(s[2], F32)[1] < R.GROUP
    assert R.VARLEN_CROSS_SHAPE == (33, 5, 72)


@pytest.mark.parametrize('dtype', R.DTYPES, ids=R.dtype_id)
def test_stride_shapes_take_a_second_trip_at_the_smallest_batch(dtype):
    for shapes, extra in ((R.embed_shapes(dtype), 1), (R.mask_shapes(dtype), 0)):
        assert [s[:3] for s in shapes[:-1]] == R.SHAPES and not any(s[3] for s in shapes[:-1])
        B, n, d, fwd_only = shapes[-1]
        assert (n, d) == (600, 776) and fwd_only and d % 8 == 0
        dv = d // VN[dtype]
        assert B * (n + extra) * dv > R.GRID_CAP * R.BLOCK >= (B - 1) * (n + extra) * dv
        assert R.stride_trips(B * (n + extra) * dv) == 2 and R.stride_trips((B - 1) * (n + extra) * dv) == 1
    assert R.embed_shapes(dtype)[-1][0] == {F32: 9, BF16: 18}[dtype] and R.mask_shapes(dtype)[-1][0] == {F32: 10, BF16: 19}[dtype]


def test_dropout_probabilities_are_accepted():
    assert R.DROPOUT_P[F32] == (0.1,) and R.DROPOUT_P[BF16][0] == 0.1 and len(R.DROPOUT_P[BF16]) == 2
    for p in R.DROPOUT_P[BF16]:                  # dropout_site_params: a 16-bit site takes round(256 p), which must not be 0
        assert 0 < int(p * 256.0 + 0.5) <= 255
    assert int(R.DROPOUT_P[BF16][0] * 256.0 + 0.5) < 128 <= int(R.DROPOUT_P[BF16][1] * 256.0 + 0.5)   # both branches of the byte compare


def test_row_forms_reach_their_edges():
    forms = [f['form'] for f in R.ROW_FORMS]
    assert forms == [(4, 25, 12, 64, 64, 64), (1, 1000, 37, 72, 72, 72), (37, 26, 1, 72, 72, 72), (5, 9, 9, 8, 8, 8), (6, 11, 4, 64, 80, 72),
                     (64, 300, 256, 520, 520, 520)]
    for f in R.ROW_FORMS:
        B, n, m, width, ld_in, ld_out = f['form']
        assert 1 <= m <= n and width % 8 == 0 and ld_in % 8 == 0 and ld_out % 8 == 0 and ld_in >= width and ld_out >= width
        idx = R.row_index(f['form'], f['idx'])
        assert idx.shape == (B, m) and idx.dtype == torch.int32 and int(idx.min()) >= 0 and int(idx.max()) < n
        assert all(len(set(r.tolist())) == m for r in idx)                       # distinct per record: a scatter has one writer per row
        for dtype in R.DTYPES:
            trips = R.stride_trips(B * m * (width // VN[dtype]))
            if dtype in f['dtypes']:
                assert (trips >= 2) if f is R.ROW_FORMS[-1] else (trips == 1)
    cls_gather, pruned, perm, pitched, big = R.ROW_FORMS[1:]
    idx = R.row_index(cls_gather['form'], cls_gather['idx'])
    assert cls_gather['form'][0] == 1 and bool((idx[0, 1:] > idx[0, :-1]).all())                      # (1, M, B): rising offsets
    assert pruned['form'][2] == 1 and not bool(R.row_index(pruned['form'], pruned['idx']).any())      # (B, N, 1): row 0 of every record
    assert perm['form'][1] == perm['form'][2] and perm['form'][3] // VN[BF16] == 1
    assert all(sorted(r.tolist()) == list(range(perm['form'][1])) for r in R.row_index(perm['form'], perm['idx']))
    assert pitched['form'][4] > pitched['form'][3] and pitched['form'][5] > pitched['form'][3] and pitched['form'][4] != pitched['form'][5]
    assert big['dtypes'] == (F32,)


def test_l1_cases_reach_their_edges():
    cases = [c['case'] for c in R.L1_CASES]
    assert cases == [(1, 1, 1), (3, 5, 7), (48, 240, 240), (8, 256, 256), (1, 2049, 2056), (4099, 520, 528)]
    want = {   # case -> (nb, per, trips of the thread loop, h)
        (1, 1, 1): (1, 1, 1, 1 + 10 + 7 + 3),
        (3, 5, 7): (1, 15, 1, 1 + 10 + 7 + 3),
        (48, 240, 240): (6, 1920, 8, 8 + 10 + 7 + 3),
        (8, 256, 256): (1, 2048, 8, 8 + 10 + 7 + 3),
        (1, 2049, 2056): (2, 1025, 5, 5 + 10 + 7 + 3),
        (4099, 520, 528): (1024, 2082, 9, 9 + 10 + 22 + 3),
    }
    for rows, width, ld in cases:
        total = rows * width
        nb, per = R.l1_blocks(total)
        assert ld >= width
        assert (nb, per, -(-per // R.BLOCK), R.l1_chain(total)) == want[(rows, width, ld)]
        assert nb * per >= total > (nb - 1) * per                                  # every block owns at least one element
    assert 8 * 256 == R.L1_PER_BLOCK                                               # the largest total of a single block
    assert 2049 - R.l1_blocks(2049)[1] == 1024                                     # the second block holds 1024 elements
    assert 4099 * 520 == 2131480 > R.L1_BLOCKS * R.L1_PER_BLOCK
    assert cases[1][2] % 2 == 1 and cases[1][2] > cases[1][1]                      # odd pitch, wider than the row
    assert cases[4][2] > cases[4][1] and cases[5][2] > cases[5][1]
