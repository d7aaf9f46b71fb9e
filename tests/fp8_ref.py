"""
The exact encoder of the two OCP 8-bit formats, the per-element criterion every emitter of 8-bit operand copies is held to, and the case lists
that tests/test_fp8_ref.py (CPU) and tests/test_gpu_fp8_ref.py (MI355X) share.  The contract is the one of include/ecgvit_hip.h, the same for
ecgvit_fp8_quantize, the two LayerNorm _q8 entry points, ecgvit_attention_fwd_q8 / _bwd_q8 and the ECGVIT_EPI_QUANT_OUT epilogues:

    byte = saturate(v as stored / *scale) in e4m3 or e5m2, round to nearest, ties to even;   *amax = max(*amax, max |v| as stored)

`encode(v32, fmt)` builds the 127 (e4m3: bytes 0x00 .. 0x7E, 0x7F is NaN) or 124 (e5m2: 0x00 .. 0x7B, 0x7C is inf) finite non-negative code values
in float64 from the format definition -- E exponent bits, M mantissa bits, bias 2^(E-1) - 1, subnormals m 2^(1 - bias - M) -- and takes the nearest
code of |v|.  A code's index in that table is its byte, so a tie goes to the even byte; the comparison is with the midpoint of the two
neighbouring codes, which is exact in float64 (no subtraction).  The sign is the sign bit; +-inf and everything beyond +-max give +-max.  Nothing
goes through a torch.float8 cast; tests/test_fp8_ref.py holds the table encoder against torch's CPU cast on every non-NaN bf16 pattern.

The criterion (`want_bytes`, `accepts`).  Every kernel multiplies by its own f32 reciprocal of the scale.  With r = f32(1) / scale correctly
rounded, a byte is right if it equals encode(clamp(f32(f32(v) r'), +-max)) for some r' in {r, nextafter(r, 0), nextafter(r, inf)}; +0 and -0 are one
code.  When the scale is a power of two, r and the product are exact and the accepted set is the single byte of r.  A scale that is not positive
gives r = 0 (the kernels' rule), so every byte is a zero code.  There is no share of bytes that may differ: `accepts(...).all()` is the assertion.
On all non-NaN bf16 patterns the three reciprocals disagree on 0 to 2 patterns at a scale that is no power of two, and at a power of two about
250 patterns are exact ties.

NaN is outside the contract: the kernels clamp with fmed3 and take the amax with fmaxf, neither of which propagates a NaN.  The sweeps replace
the NaN patterns by zero (`all_bf16`).

C of the ECGVIT_EPI_QUANT_OUT launches (tests/test_gpu_fp8_ref.py, `c_bound`) is held element by element to the float64 product of the dequantised
operands through the same epilogue.  The bound is derived: what the project's stored-GELU test grants for the rounding to bf16, 2^-8 |ref| (+ 1e-4,
the three-term erf's floor, on the GELU sets), plus g K 2^-23 (|A| |B|^T) |scale_a scale_b| for the f32 accumulation, with g what the epilogue
multiplies an error of the accumulator by: GELU_LIP = 1.13 >= max |gelu'| on the FFN-up sets, |aux| on the FFN-down input gradient, and 1 / (1 - p)
under dropout.  The products of 8-bit values are exact in f32; K - 1 additions in any order cost at most (K - 1) 2^-24 of the absolute sum, so
K 2^-23 also covers the two roundings of scale_a scale_b and the addition of the bias.  Under dropout (p = 0.25: keep threshold 64 / 256) an element
is exactly 0 where ecgvit_dropout_apply with the same seed gives 0, else within the bound of ref / (1 - p), the 1e-4 floor scaled likewise.
Largest |C - ref| / bound measured on the MI355X (MEASURED), by flag set and shape of GEMM_SHAPES; both runs of a case store the same C:

                  2051 x 136 x 384    2304 x 264 x 512    8200 x 2056 x 384
    UP|Q               0.9260              0.8915              0.9377
    UP|D|Q             0.9179              0.8761              0.9249
    UP|Q|A8            0.9260              0.8915              0.9377
    UP|D|Q|A8          0.9179              0.8761              0.9249
    DH|Q               0.9328              0.9189              0.9483
    DH|Q|A8            0.9328              0.9189              0.9483

The figures sit near 1 because the first term alone is attained: a value just above a power of two that rounds by half a bf16 ulp is off by
2^-8 of itself.  The accumulation term is a few 1e-5 of |ref| here and far from attained.  The NO_OUT sets write no C; their bytes, amax, saved
tensor and column sums are bit for bit those of their writing set.  AUX8 changes the saved tensor's format, not C.
"""
import math

import torch

F64, F32, BF16 = torch.float64, torch.float32, torch.bfloat16

E4M3, E5M2 = 'e4m3', 'e5m2'
FORMATS = (E4M3, E5M2)
_DEF = {E4M3: (4, 3, 0x7E), E5M2: (5, 2, 0x7B)}      # exponent bits, mantissa bits, the largest finite byte
FMAX = {E4M3: 448.0, E5M2: 57344.0}
NAN_BYTE = {E4M3: 0x7F, E5M2: 0x7F}                  # a byte no emitter produces: the sentinel of the output buffers
OVERFLOW_BYTE = {E4M3: 0x7F, E5M2: 0x7C}             # what a cast without saturation gives beyond max: NaN / inf
TORCH8 = {E4M3: torch.float8_e4m3fn, E5M2: torch.float8_e5m2}   # the independent check of tests/test_fp8_ref.py only


def fmt_of(code):
    """'e4m3' / 'e5m2' from the header's ECGVIT_FP8_E4M3 = 2 / ECGVIT_BF8_E5M2 = 3"""
    return {2: E4M3, 3: E5M2}[code]


FMT_CODE = {E4M3: 2, E5M2: 3}


def code_values(fmt):
    """the finite non-negative code values, float64, indexed by byte"""
    ebits, mbits, top = _DEF[fmt]
    bias = 2 ** (ebits - 1) - 1
    vals = []
    for b in range(top + 1):
        e, m = b >> mbits, b & (2 ** mbits - 1)
        vals.append(math.ldexp(m, 1 - bias - mbits) if e == 0 else math.ldexp(2 ** mbits + m, e - bias - mbits))
    assert vals[-1] == FMAX[fmt] and all(a < b for a, b in zip(vals, vals[1:]))
    return torch.tensor(vals, dtype=F64)


_TABLES = {}


def _table(fmt, device):
    key = (fmt, str(device))
    if key not in _TABLES:
        _TABLES[key] = code_values(fmt).to(device)
    return _TABLES[key]


def encode(v32, fmt):
    """uint8 bytes of the values `v32` (any float dtype; widened to float64 on its device): nearest code, ties to the even byte, sign from the
    sign bit, saturation at +-max"""
    t = _table(fmt, v32.device)
    v = v32.to(F64)
    a = v.abs().clamp(max=FMAX[fmt])
    hi = torch.searchsorted(t, a.contiguous()).clamp(max=t.numel() - 1)   # first code >= a
    lo = (hi - 1).clamp(min=0)
    mid = (t[lo] + t[hi]) * 0.5                                           # exact: two codes of at most 5 bits, one binade apart at most
    up = (a > mid) | ((a == mid) & ((lo & 1) == 1))
    b = torch.where(up, hi, lo)
    return (b + 128 * torch.signbit(v).to(b.dtype)).to(torch.uint8)


def canon(b):
    """+0 and -0 are one code"""
    return torch.where(b == 0x80, torch.zeros_like(b), b)


def reciprocals(scale32):
    """the f32 reciprocals a kernel may multiply by, as Python floats: [r] for a power of two (exact) or a scale that is not positive (0),
    else [r, nextafter(r, 0), nextafter(r, inf)] around the correctly rounded r = f32(1) / scale"""
    s = torch.as_tensor(scale32, dtype=F32).detach().reshape(()).cpu()
    if not float(s) > 0.0:
        return [0.0]
    r = torch.ones((), dtype=F32) / s                                     # IEEE division on the host: correctly rounded
    if math.frexp(float(s))[0] == 0.5 and math.isfinite(float(r)) and float(r) * float(s) == 1.0:
        return [float(r)]
    return [float(r), float(torch.nextafter(r, torch.zeros((), dtype=F32))), float(torch.nextafter(r, torch.full((), math.inf, dtype=F32)))]


def scaled(stored, r, fmt):
    """clamp(f32(f32(v) r), +-max): the f64 product of two f32 values is exact, its rounding to f32 is the f32 multiplication"""
    return (stored.to(F32).to(F64) * r).to(F32).clamp(-FMAX[fmt], FMAX[fmt])


def want_bytes(stored, scale32, fmt):
    """the accepted bytes, [1 or 3, *stored.shape] uint8 (module docstring)"""
    return torch.stack([encode(scaled(stored, r, fmt), fmt) for r in reciprocals(scale32)])


def accepts(got, stored, scale32, fmt):
    """bool, the shape of `got`: the byte is one of the accepted ones"""
    g = canon(got)
    ok = torch.zeros(got.shape, dtype=torch.bool, device=got.device)
    for r in reciprocals(scale32):
        ok |= g == canon(encode(scaled(stored, r, fmt), fmt))
    return ok


def describe_refused(got, stored, scale32, fmt, limit=5):
    """the first refused elements, for an assertion message: (flat index, value as stored, byte got, bytes accepted)"""
    bad = (~accepts(got, stored, scale32, fmt)).flatten().nonzero().flatten()
    idx = bad[:limit]
    w = want_bytes(stored.flatten()[idx], scale32, fmt)
    return int(bad.numel()), [(int(i), float(stored.flatten()[i]), int(got.flatten()[i]), w[:, k].tolist()) for k, i in enumerate(idx)]


def all_bf16(device='cpu'):
    """all 65 536 bf16 patterns in pattern order, the 254 NaN patterns replaced by zero; +-inf kept"""
    x = torch.arange(65536, dtype=torch.int32, device=device).to(torch.int16).view(BF16)
    return torch.where(torch.isnan(x), torch.zeros_like(x), x)


def ulp32(x):
    """one f32 ulp of |x| (f32 tensor of normal values)"""
    return torch.nextafter(x.abs(), torch.full_like(x, math.inf)) - x.abs()


# ------------------------------------------------------------------------------------------------------------------ case lists
SWEEP_SCALES = (1.0, 0.25, 0.0137, 3.1e-5, 17.3)      # tests/test_fp8_ref.py: the table encoder against torch's CPU cast
POW2_SCALES = (1.0, 2.0 ** -6, 2.0 ** 5)              # byte-exact: one accepted byte
# no power of two: an ordinary one; one at which a large share of the bf16 patterns saturates (everything above 448 x 3.1e-5 = 0.014, i.e.
# 52 % of the patterns in e4m3, above 57344 x 3.1e-5 = 1.8 in e5m2); and the largest kind an f32 scale with a normal reciprocal allows, at which
# everything below 2^-6 x 6e37 = 9.4e35 (e4m3) / 2^-14 x 6e37 = 3.7e33 (e5m2) lands in the 8-bit subnormals or rounds to zero: 97 % / 94 % of the
# patterns (no f32 scale puts the top bf16 binades there: it would have to exceed 64 x 3.4e38)
QUANT_NP2_SCALES = (0.0137, 3.1e-5, 6.0e37)
SATURATING_SCALE, SUBNORMAL_SCALE = 3.1e-5, 6.0e37
ZERO_CODE_SCALES = (0.0, -0.37)                       # r = 0: every byte a zero code (finite input)

# ecgvit_fp8_quantize / ecgvit_fp8_amax launch geometry restated (csrc/fp8.hip): 256 lanes x 16 elements per block and trip (the amax kernel: 8
# per lane on the same grid), grid = clamp(ceil(floor(count / 16) / 256), 1, nseg > 1 ? 256 : 4096) x nseg; a lane whose last 16 elements hold only
# 8 takes the 8-byte tail branch, which runs exactly when count % 16 == 8
LANE_ELEMS, BLOCK_LANES, GRID_CAP_ONE, GRID_CAP_SEG = 16, 256, 4096, 256
BLOCK_ELEMS = LANE_ELEMS * BLOCK_LANES                # 4096
# 8: the tail alone; 16: no tail; 24: one whole step + the tail in the next lane; 256 x 16 - 8: the block's last lane in the tail; 256 x 16 + 8
# (= 4096 + 8): still one block, lane 0's second trip is the tail; the last: 4096 blocks x 4096 elements + 24 -- the capped grid's second trip, a
# whole step for lane 0 of block 0 and the tail for lane 1
COUNTS = (8, 16, 24, BLOCK_ELEMS - 8, BLOCK_ELEMS + 8, GRID_CAP_ONE * BLOCK_ELEMS + 24)
# segment table (first element: a multiple of 16, count: a multiple of 8): unequal, gaps in front of, between and behind the segments, a segment
# of 8, tails in segments 0, 1 and 3, and segment 3 longer than 256 blocks x 4096 elements, so the capped grid of nseg > 1 walks it twice with a tail
SEG_LONG = GRID_CAP_SEG * BLOCK_ELEMS + 3 * BLOCK_ELEMS + 40
SEGMENTS = ((32, 24), (80, 8), (112, 4096), (4096 + 256, SEG_LONG), (4096 + 256 + SEG_LONG + 24 + 64, 4104))
SEG_TOTAL = SEGMENTS[-1][0] + SEGMENTS[-1][1] + 48
SEG_SCALES = (0.0137, 1.0, 0.25, 3.1e-3, 0.7)         # one per segment


def grid_blocks(count, nseg):
    return max(1, min((count // LANE_ELEMS + BLOCK_LANES - 1) // BLOCK_LANES, GRID_CAP_SEG if nseg > 1 else GRID_CAP_ONE))


def takes_tail(count):
    return count % LANE_ELEMS == 8


def second_trip(count, nseg):
    """elements left for a second trip of the grid-stride loop"""
    return max(0, count - grid_blocks(count, nseg) * BLOCK_ELEMS)


SCALE_UPDATE_N = 257                                  # two blocks of fp8_scale_update_kernel, the second with one live lane

# ECGVIT_EPI_QUANT_OUT on the 8-bit A . B^T kernel: the smallest shapes its router admits (M >= 2048, N >= 128, N % 8 == 0, K >= 384, K % 128 == 0)
GEMM_TILE = 256
GEMM_SHAPES = ((2051, 136, 384),      # a 3-row last tile, one narrow tile in N
               (2304, 264, 512),      # whole in M, an 8-column last tile
               (8200, 2056, 384))     # 33 x 9 = 297 tiles on 256 workgroups, ragged both ways: a workgroup walks several tiles (the amax carry)
EPI_BIAS, EPI_GELU, EPI_DROPOUT, EPI_COLSUM, EPI_GELU_GRAD_AUX, EPI_MUL_AUX, EPI_Q, EPI_NO, EPI_A8 = 1, 2, 32, 64, 128, 256, 512, 1024, 2048
UP = EPI_BIAS | EPI_GELU | EPI_GELU_GRAD_AUX
DH = EPI_MUL_AUX | EPI_COLSUM
# every Q-bearing set of epi_sets::E4m3 and epi_sets::E5m2 (csrc/gemm_plan.h): name -> (flags of the writing set, operand format of A, format of the copy)
Q_SETS = {'UP|Q': (UP | EPI_Q, E4M3), 'UP|D|Q': (UP | EPI_DROPOUT | EPI_Q, E4M3), 'UP|Q|A8': (UP | EPI_Q | EPI_A8, E4M3),
          'UP|D|Q|A8': (UP | EPI_DROPOUT | EPI_Q | EPI_A8, E4M3), 'DH|Q': (DH | EPI_Q, E5M2), 'DH|Q|A8': (DH | EPI_Q | EPI_A8, E5M2)}
# ... each with its |NO form, run by the same case: 12 sets
GEMM_P = 0.25                                         # bf16 outputs keep with threshold round(256 p) = 64: 1 / (1 - p) = 4 / 3 to one f32 ulp
GEMM_SEED = 99
GELU_LIP = 1.13                                       # max |gelu'(x)| = 1.1289 at x = sqrt(2)
LDQ_PAD, SLACK_ROWS = 24, 3                           # ldq8 = N + 24; three rows of sentinels behind row M - 1


def n_tiles(M, N):
    return -(-M // GEMM_TILE) * -(-N // GEMM_TILE)


def c_bound(ref, abs_prod, K, gain, gelu):
    """bound on |C - ref| (module docstring): ref, abs_prod = (|A| |B|^T) |scale_a scale_b| and gain are f64 tensors (or a float)"""
    return 2.0 ** -8 * ref.abs() + (1e-4 if gelu else 0.0) + gain * (K * 2.0 ** -23) * abs_prod


MEASURED = {'UP|Q': 0.9377, 'UP|D|Q': 0.9249, 'UP|Q|A8': 0.9377, 'UP|D|Q|A8': 0.9249, 'DH|Q': 0.9483, 'DH|Q|A8': 0.9483}   # worst over the shapes
