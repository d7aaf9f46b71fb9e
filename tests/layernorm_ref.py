"""
A plain torch restatement, in float64, of the LayerNorm contracts of include/ecgvit_hip.h (ecgvit_layernorm_fwd / _fwd_q8, ecgvit_layernorm_bwd /
_bwd_fused / _bwd_fused_rowpitch / _bwd_fused_q8), with the case lists and bounds that tests/test_layernorm_ref.py (CPU) and
tests/test_gpu_layernorm.py (MI355X) share.  Inputs are the exact f32 or bf16 values a kernel receives, widened to f64.  The backward takes `mean`
and `rstd` as INPUTS: its reference uses the f32 values handed to the kernel (`stats32`: computed in f64, rounded once to f32), widened, so a
backward figure says nothing about the forward.

Bounds.  u = 2^-24 (f32 unit roundoff), h = half an ulp of the element type relative to the value (f32: u, bf16: 2^-8).  Every bound is first
order, holds for f32 terms added in ANY order, is evaluated at the f64 reference, and is floored at one ulp of the output type (as
embed_ref.dpos_bound is), so none encodes a kernel's own order.  t = x - mean, var = sum t^2 / d, w = var + eps, xh = t rstd.

    mean    Dmean = (d - 1) u sum|x| / d
                    d - 1 additions of a sum in any order; the two roundings of the scaling by 1 / d ride inside d - 1 (they could exceed it only in
                    a strictly sequential sum, where just two of the d terms carry d - 1 roundings; every balanced order has depth log2 d)
    rstd    Dw    = 2 Dmean mean|t| + (d + 4) u var + u w
                    the shifted mean in every t (2 |t| Dmean each; their signed sum vanishes, the bound keeps the absolute one), 3 roundings in one
                    t^2 (the subtraction twice, the square), d - 1 of the sum, 2 of the scaling, 1 of the addition of eps
            Drstd = rstd (Dw / (2 w) + 4 u)
                    1 / sqrt propagates half the relative error of w; sqrtf and the division are each within one f32 ulp (2 u)
    y       |gamma| rstd Dmean + |t| |gamma| Drstd + 3 u |xh gamma| + u |y| + (bf16: 2^-8 |y|)
                    the subtraction and the two products of the affine form, the f32 addition of beta, the rounding to bf16
    dx      g = dy gamma, c1 = mean(g), c2 = mean(g xh), dx = rstd (g - c1 - xh c2) + dres
            Dc1 = (d + 2) u mean|g|         d - 1 of the sum, 1 in a term (the product dy gamma), 2 of the scaling
            Dc2 = (d + 5) u mean|g xh|      d - 1 of the sum, 4 in a term (g, the two of xh, their product), 2 of the scaling
            rstd (Dc1 + |xh| Dc2 + u (4 |g| + 3 |c1| + 5 |xh c2|)) + u |dx| + (bf16: 2^-8 |dx|)
                    |g| is rounded once itself and passes two subtractions and the product with rstd; c1 passes the same three; xh c2 carries the
                    two roundings of xh, its own product, one subtraction and the product with rstd; then the f32 addition of dres and the
                    rounding to bf16
    dgamma, dbeta, dcolsum      per column, `colsum_bound`: (rows + k) u sum_r |term|, k the roundings inside one term:
                    dgamma  term dy xh, k = 3 (the two of xh and the product);  dbeta  term dy, k = 0;
                    dcolsum term = the value AS STORED (the kernel's own dxm, or dx without dropout, widened to f64: the header says "as stored"), k = 0

What is a copy or a single rounding is compared by bits: dxm = T(f32(dx as stored) m), m in {0, inv_keep} (`dxm_rounded`, `inv_keep`); the e4m3 / e5m2
copies are torch's float8 cast of clamp(f32(v as stored) (1.0f / scale), +-max) (`q8_bytes`), zeros of either sign equal; a differing byte must be the
code adjacent to the wanted one (`q8_differences`) and their share stays under Q8_DIFFER_CAP, the figure tests/test_gpu_fp8.py already allows: the kernel
multiplies by its own f32 reciprocal of the scale, which may differ from torch's in the last place and then tips a value that lies at a rounding
boundary of the 8-bit format into the neighbouring code.

Launch geometry restated (csrc/rowops.hip), from which tests/test_layernorm_ref.py asserts with integer arithmetic that every case reaches the edge
it is listed for:

    one row per wave, 4 waves per block; forward grid min(ceil(rows / 4), 2048), backward grid = nparts = min(ceil(rows / 4), 1024)
    generic kernel: lane l holds vector i at columns (64 i + l) VN .. + VN, VN = 4 f32 / 8 bf16; WV = 64 VN = 256 / 512 columns per vector index;
                    MAXV = ceil(d / WV) rounded up to a power of two
    bf16, d = 64 E, E in {4, 8, 12, 16, 24, 32}: the exact lane mapping, E / 8 16-byte chunks + (E % 8 == 4) one 8-byte chunk per lane
    reducer: 64 columns x 16 slices; slice s walks partial rows s, s + 16, ...: four at a time while p + 48 < nparts (stride 64), then singly
"""
import torch

from embed_ref import F64, F32, BF16, VN, ESIZE, DTYPES, U32, ulp32, worst_ratio, dtype_id, _gen   # noqa: F401  (shared with the two test files)

EPS = 1e-5
UB16 = 2.0 ** -8                          # half an ulp of bf16, relative to the value
HALF_ULP = {F32: U32, BF16: UB16}
SIG_BITS = {F32: 24, BF16: 8}
WV = {F32: 256, BF16: 512}                # columns covered by one vector per lane
WAVES = 4                                 # rows per block and trip
FWD_CAP, BWD_CAP = 2048, 1024             # blocks
RED_SLICES, RED_STRIDE = 16, 64           # reduce_partials_kernel
FIT_E = (4, 8, 12, 16, 24, 32)            # exact-lane-mapping widths / 64
ROW_MAX_D = 2048

# ------------------------------------------------------------------------------------------------------------------ case lists
# widths, both types.  f32: MAXV = 1 (<= 256), 2 (264, 512), 4 (520 .. 1024), 8 (1032 .. 2048); a partly live last vector at 8, 72, 264, 520, 1032,
# 2040.  bf16: the six multiples of 256 take E = 4 (the 8-byte tail path alone), 8, 12 (16 B + tail), 16, 24, 32; the rest take the generic kernel at
# MAXV = 1 (8, 64, 72, 264), 2 (520), 4 (1032, 2040)
WIDTHS = [8, 64, 72, 256, 264, 512, 520, 768, 1024, 1032, 1536, 2040, 2048]
WIDTH_ROWS = (5, 65)                      # 5: fewer rows than two blocks' waves, the second block has one live wave; 65: 17 blocks, 17 partial rows
# row counts at one generic and one exact-mapping width: nparts = 1, 1, 16, 17, 49, 65 -- both sides of each reducer loop boundary
ROW_COUNTS = [1, 3, 61, 65, 193, 257]
ROW_WIDTHS = (72, 768)
# capped grids: 256 = bf16 exact mapping and f32 MAXV 1, 264 = generic with a partly live vector
CAPPED_WIDTHS = (256, 264)
CAPPED_BWD_ROWS = 4099                    # nparts = 1024, three waves take a second row
CAPPED_FWD_ROWS = 8195                    # 2048 blocks, three waves take a second row
# fused forms: one width of each kernel form
FUSED_WIDTHS = {BF16: (72, 256, 520, 768, 1536, 2040),      # generic MAXV 1, E = 4, MAXV 2, E = 12, E = 24, MAXV 4
                F32: (64, 264, 768, 2040)}                  # MAXV 1, 2, 4, 8
FUSED_P = {F32: (0.0, 0.1), BF16: (0.0, 0.1, 0.5)}           # bf16 applies round(256 p) / 256: 0.5 -> threshold 128, the other branch of quad_keepbits
FUSED_ROWS = (5, 65)
PITCH = 7                                 # ecgvit_layernorm_bwd_fused_rowpitch: row r draws the bits of row 7 r
Q8_WIDTHS = (256, 512, 768, 1024, 1536, 2048)
Q8_FWD_ROWS = (5, 65, CAPPED_FWD_ROWS)
Q8_BWD_ROWS = (5, 65)
Q8_DELAY = 1.5                            # a delayed scale: 1.5 x the tensor's own (tests/test_gpu_fp8.py)
Q8_DIFFER_CAP = 1e-4                      # share of bytes that may be the adjacent code (tests/test_gpu_fp8.py)
SEED = 0x5EED0BADC0FFEE
FAMILIES = ('randn', 'offset', 'constant', 'spike')
OFFSET, SPIKE, CONST = 64.0, 1e3, 0.75
ZERO_COL = 3                              # gamma[3] == 0 exactly; gamma[0] > 0 > gamma[1]
# refused: (rows, d)
REFUSED_SHAPES = [(5, 12), (5, 2056), (0, 64)]
REFUSED_Q8_D = 520
REFUSED_BF16_P = 0.001


def kernel_form(d, dtype):
    """('fit', E) for the exact lane mapping, else ('generic', MAXV)"""
    if dtype == BF16 and d % 256 == 0 and d // 64 in FIT_E:
        return 'fit', d // 64
    nv = -(-d // WV[dtype])
    return 'generic', 1 << (nv - 1).bit_length()


def last_vector_lanes(d, dtype):
    """live lanes of the last live vector index of the generic mapping (64: full)"""
    nvec = d // VN[dtype]
    return nvec - 64 * ((nvec - 1) // 64)


def grid(rows, cap):
    return min(-(-rows // WAVES), cap)


def second_trip_waves(rows, cap):
    """waves that take a second row (0 below the cap)"""
    nw = grid(rows, cap) * WAVES
    return max(0, min(rows - nw, nw))


def nparts(rows):
    return grid(rows, BWD_CAP)


def reducer_trips(n, s):
    """(trips of the unrolled-by-four loop, trips of the single loop) of slice s over n partial rows"""
    p, four, one = s, 0, 0
    while p + 3 * RED_SLICES < n:
        four, p = four + 1, p + RED_STRIDE
    while p < n:
        one, p = one + 1, p + RED_SLICES
    return four, one


def shape_id(rows, d):
    return f'{rows}x{d}'


# ------------------------------------------------------------------------------------------------------------------ inputs
def ln_inputs(rows, d, dtype, family='mixed'):
    """host tensors x, dy, dres [rows, d] (dtype), gamma, beta [d] f32.  Row r of x belongs to FAMILIES[r % 4] ('mixed') or to the one family named:
        randn     2 randn + 0.5
        offset    2 randn + 64: |mean| / std = 32, still varied after rounding to bf16 (ulp 0.5 at 64) -- what a one-pass variance gets wrong
        constant  0.75 in every column: variance 0, rstd = 1 / sqrt(eps)
        spike     randn with one element of 1e3
    gamma has both signs and gamma[ZERO_COL] == 0"""
    g = _gen(rows, d, ESIZE[dtype], 9 if family == 'mixed' else FAMILIES.index(family))
    n = max(rows, 1)
    base = torch.randn(n, d, generator=g)
    fam = torch.arange(n) % 4 if family == 'mixed' else torch.full((n,), FAMILIES.index(family))
    x = 2 * base + 0.5
    x = torch.where((fam == 1)[:, None], 2 * base + OFFSET, x)
    x = torch.where((fam == 2)[:, None], torch.full_like(x, CONST), x)
    spike = torch.where((fam == 3)[:, None], base, x)
    spike[torch.arange(n), (7 * torch.arange(n) + 3) % d] = SPIKE
    x = torch.where((fam == 3)[:, None], spike, x).to(dtype)
    gamma, beta = torch.randn(d, generator=g), torch.randn(d, generator=g)
    gamma[0], gamma[1], gamma[ZERO_COL] = gamma[0].abs() + 0.5, -gamma[1].abs() - 0.5, 0.0
    dy, dres = torch.randn(n, d, generator=g).to(dtype), torch.randn(n, d, generator=g).to(dtype)
    return dict(x=x, gamma=gamma, beta=beta, dy=dy, dres=dres)


# ------------------------------------------------------------------------------------------------------------------ float64 restatement
def fwd(x, gamma, beta, eps=EPS):
    """(mean [rows], rstd [rows], y [rows, d]) f64: biased variance, affine"""
    x = x.to(F64)
    mean = x.mean(1)
    t = x - mean[:, None]
    rstd = 1.0 / torch.sqrt((t * t).mean(1) + eps)
    return mean, rstd, t * rstd[:, None] * gamma.to(F64) + beta.to(F64)


def stats32(x, eps=EPS):
    """the (mean, rstd) a backward is handed: f64, rounded once to f32"""
    mean, rstd, _ = fwd(x, torch.ones(x.shape[1], dtype=F64, device=x.device), torch.zeros(x.shape[1], dtype=F64, device=x.device), eps)
    return mean.to(F32), rstd.to(F32)


def bwd(dy, x, gamma, mean32, rstd32, dres=None):
    """(dx [rows, d], dgamma [d], dbeta [d]) f64 from the f32 mean / rstd as given: dx = (dres ? dres : 0) + LN'(dy)"""
    dy, x, gamma = dy.to(F64), x.to(F64), gamma.to(F64)
    rs = rstd32.to(F64)[:, None]
    xh = (x - mean32.to(F64)[:, None]) * rs
    g = dy * gamma
    dx = rs * (g - g.mean(1, keepdim=True) - xh * (g * xh).mean(1, keepdim=True))
    if dres is not None:
        dx = dx + dres.to(F64)
    return dx, (dy * xh).sum(0), dy.sum(0)


def colsum(stored):
    """dcolsum [d] f64: the column sums of the values as stored (the kernel's own dxm, or dx without dropout)"""
    return stored.to(F64).sum(0)


# ---- what the kernels must return bit for bit
def inv_keep(p, dtype):
    """the f32 rescale of a kept element: bf16 256 / (256 - round(256 p)), f32 1.0f / (1.0f - p)"""
    one = torch.ones((), dtype=F32)
    if dtype == BF16:
        return torch.tensor(256.0, dtype=F32) / torch.tensor(256.0 - threshold8(p), dtype=F32)
    return one / (one - torch.tensor(p, dtype=F32))


def threshold8(p):
    return 0 if p <= 0 else min(255, int(p * 256.0 + 0.5))


def dxm_rounded(dx_stored, keep, p):
    """T(f32(dx as stored) m), m = keep ? inv_keep : 0 (keep: bool, the shape of dx)"""
    m = keep.to(F32) * inv_keep(p, dx_stored.dtype).to(dx_stored.device)
    return (dx_stored.float() * m).to(dx_stored.dtype)


FP8 = {'e4m3': (torch.float8_e4m3fn, 448.0), 'e5m2': (torch.float8_e5m2, 57344.0)}


def q8_bytes(stored, scale, fmt):
    """the bytes of clamp(f32(v as stored) (1.0f / scale), +-max) in `fmt`, by torch's float8 cast (scale: an f32 tensor of one element)"""
    dt, mx = FP8[fmt]
    inv = torch.ones((), dtype=F32, device=stored.device) / scale.to(F32).reshape(())
    return (stored.float() * inv).clamp(-mx, mx).to(dt).view(torch.uint8)


def q8_differences(got, want):
    """(bytes that differ, bytes that differ by more than one code) of two uint8 tensors of one 8-bit float format; +0 and -0 are one code"""
    def key(b):
        m = (b & 0x7F).to(torch.int16)
        return torch.where(b >= 128, -m, m)
    k = (key(got) - key(want)).abs()
    return int((k != 0).sum()), int((k > 1).sum())


# ------------------------------------------------------------------------------------------------------------------ bounds
def ulp_of(x, dtype):
    """one unit in the last place of |x| in `dtype` (f64 tensor; 0 at 0)"""
    _, e = torch.frexp(x.abs().to(F64))
    return torch.where(x == 0, torch.zeros_like(x, dtype=F64), torch.ldexp(torch.ones_like(x, dtype=F64), e - SIG_BITS[dtype]))


def fwd_held(x, gamma, beta, dtype, eps=EPS):
    """{name: (reference, bound)} for mean, rstd, y (module docstring)"""
    d = x.shape[1]
    x, gamma = x.to(F64), gamma.to(F64)
    mean, rstd, y = fwd(x, gamma, beta, eps)
    t = x - mean[:, None]
    var = (t * t).mean(1)
    w = var + eps
    dmean = torch.maximum((d - 1) * U32 * x.abs().sum(1) / d, ulp32(mean))
    dw = 2 * dmean * t.abs().mean(1) + (d + 4) * U32 * var + U32 * w
    drstd = torch.maximum(rstd * (dw / (2 * w) + 4 * U32), ulp32(rstd))
    ga = gamma.abs()
    by = (ga * rstd[:, None] * dmean[:, None] + t.abs() * ga * drstd[:, None] + 3 * U32 * (t * rstd[:, None] * gamma).abs() + U32 * y.abs())
    if dtype == BF16:
        by = by + UB16 * y.abs()
    return dict(mean=(mean, dmean), rstd=(rstd, drstd), y=(y, torch.maximum(by, ulp_of(y, dtype))))


def colsum_bound(terms, ref, k):
    """terms [rows, d] f64 (the exact terms), ref [d] their f64 sum: max((rows + k) u sum_r |term|, one f32 ulp of ref)"""
    return torch.maximum((terms.shape[0] + k) * U32 * terms.abs().sum(0), ulp32(ref))


def bwd_held(dy, x, gamma, mean32, rstd32, dres, dtype):
    """{name: (reference, bound)} for dx, dgamma, dbeta (module docstring)"""
    d = x.shape[1]
    dx, dgamma, dbeta = bwd(dy, x, gamma, mean32, rstd32, dres)
    dy, x, gamma = dy.to(F64), x.to(F64), gamma.to(F64)
    rs = rstd32.to(F64)[:, None]
    xh = (x - mean32.to(F64)[:, None]) * rs
    g = dy * gamma
    c1, c2 = g.mean(1, keepdim=True), (g * xh).mean(1, keepdim=True)
    dc1 = (d + 2) * U32 * g.abs().mean(1, keepdim=True)
    dc2 = (d + 5) * U32 * (g * xh).abs().mean(1, keepdim=True)
    bdx = rs * (dc1 + xh.abs() * dc2 + U32 * (4 * g.abs() + 3 * c1.abs() + 5 * (xh * c2).abs())) + U32 * dx.abs()
    if dtype == BF16:
        bdx = bdx + UB16 * dx.abs()
    return dict(dx=(dx, torch.maximum(bdx, ulp_of(dx, dtype))), dgamma=(dgamma, colsum_bound(dy * xh, dgamma, 3)), dbeta=(dbeta, colsum_bound(dy, dbeta, 0)))


def colsum_held(stored):
    ref = colsum(stored)
    return ref, colsum_bound(stored.to(F64), ref, 0)
