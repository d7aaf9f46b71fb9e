"""
A plain torch restatement, in float64, of the embedding and masked-objective contracts of include/ecgvit_hip.h (ecgvit_embed_finish / _bwd,
ecgvit_mask_embed_finish / _bwd, ecgvit_l1_loss_fwd_bwd; gather and scatter are torch indexing and need no function), with the case lists that
tests/test_embed_ref.py (CPU) and tests/test_gpu_embed_masked_ops.py (MI355X) share.  Inputs are the exact f32 or bf16 values a kernel receives,
widened to f64, so a bound below speaks of the kernel's own roundings only.

What a kernel is held to:

    forward X               bit-equal to `embed_rounded` / `mask_embed_rounded`: one f32 add, one rounding to the element type
    dtok, dmasked, dpred    bit-equal (copies, exact zeros, one constant)
    dpos, dcls              |got - ref| <= max((B - 1) 2^-24 sum_b |dX|, one f32 ulp of ref)      (`dpos_bound`)
                            a first-order bound of B f32 terms added in ANY order, so it does not encode the kernel's order
    loss                    |got - ref| <= h 2^-24 ref, h = `l1_chain(total)`

`l1_chain`: every term |pred - target| is non-negative, so each rounding on the way costs at most 2^-24 of the RESULT and the longest chain of
roundings bounds the relative error.  With nb = min(1024, ceil(total / 2048)) blocks of 256 threads, each owning per = ceil(total / nb)
consecutive elements:

    ceil(per / 256)     additions in a thread's loop
    10                  the block reduction (six butterfly steps inside a wave, four waves)
    ceil(nb / 64) + 6   the finish: one wave walks the partials, then its six butterfly steps
    3                   the f32 subtraction, the reciprocal of the count, the final multiply

Shapes (B, n, d) and the edge each is listed for (VN = 4 f32 / 8 bf16 elements per 16-B vector; the backward kernels run 32 batch lanes, b = lane,
lane + 32, ..., over groups of 8 column vectors; the element-wise kernels run at most 4096 blocks of 256 threads and stride from there):

    (1, 1, 8)       one record, one patch, one bf16 vector per row
    (32, 7, 64)     exactly one trip of the batch loop in every lane
    (33, 5, 72)     lane 0 takes a second trip; d / VN = 18 or 9: the last column group holds 2 or 1 live vectors
    (65, 3, 264)    lane 0 takes a third trip; d / VN = 66 or 33: nine or five groups, the last partly live
    (B*, 600, 776)  forward only: B* = the smallest B whose vector count passes 4096 * 256 (`stride_B`)

tests/test_embed_ref.py asserts each of these with integer arithmetic, so a case that stops reaching its edge fails there.
"""
import torch

F64, F32, BF16 = torch.float64, torch.float32, torch.bfloat16
VN = {F32: 4, BF16: 8}                  # elements per 16-B vector
ESIZE = {F32: 4, BF16: 2}
DTYPES = (F32, BF16)
U32 = 2.0 ** -24                        # unit roundoff of f32
GRID_CAP, BLOCK = 4096, 256             # element-wise launches: at most GRID_CAP blocks of BLOCK threads, one 16-B vector per thread and trip
BATCH_LANES, GROUP = 32, 8              # embed_bwd / mask_embed_bwd: 32 batch lanes x 8 column vectors per workgroup
L1_BLOCKS, L1_PER_BLOCK = 1024, 2048    # ecgvit_l1_loss_fwd_bwd: nb = min(L1_BLOCKS, ceil(total / L1_PER_BLOCK))
MB = 1e6

# ------------------------------------------------------------------------------------------------------------------ case lists
SHAPES = [(1, 1, 8), (32, 7, 64), (33, 5, 72), (65, 3, 264)]
STRIDE_N, STRIDE_D = 600, 776
STRIDE_MB = 40                          # tok + X of a stride-loop shape
SMALL_MB = 2                            # tok, X, dX, dtok and dmasked of a SHAPES case together
DROPOUT_SHAPES = [(33, 5, 72), (65, 3, 264)]
DROPOUT_P = {F32: (0.1,), BF16: (0.1, 0.5)}     # bf16 applies round(256 p) / 256: 0.5 -> threshold 128, the other branch of the byte compare
DROPOUT_SEED = 0x5EED0BADC0FFEE
VARLEN_CROSS_SHAPE = (33, 5, 72)

# (B, n, m, width, ld_in, ld_out), dtypes, index family, stated memory (MB) of in + out
ROW_FORMS = [
    dict(form=(4, 25, 12, 64, 64, 64), dtypes=DTYPES, idx='randperm', mb=1),          # the existing form
    dict(form=(1, 1000, 37, 72, 72, 72), dtypes=DTYPES, idx='rising', mb=1),          # the ragged CLS gather: rising offsets
    dict(form=(37, 26, 1, 72, 72, 72), dtypes=DTYPES, idx='zeros', mb=1),             # the pruned-block scatter: row 0 of every record
    dict(form=(5, 9, 9, 8, 8, 8), dtypes=DTYPES, idx='randperm', mb=1),               # m == n: a full permutation; one bf16 vector per row
    dict(form=(6, 11, 4, 64, 80, 72), dtypes=DTYPES, idx='randperm', mb=1),           # both pitches wider than the row
    dict(form=(64, 300, 256, 520, 520, 520), dtypes=(F32,), idx='randperm', mb=80),   # the vector count passes 4096 * 256: stride loop
]

# (rows, width, ld), stated memory (MB) of pred + target + dpred
L1_CASES = [
    dict(case=(1, 1, 1), mb=1),            # smallest
    dict(case=(3, 5, 7), mb=1),            # odd pitch
    dict(case=(48, 240, 240), mb=1),       # the engine's form, C * P = 240
    dict(case=(8, 256, 256), mb=1),        # total = 2048: nb = 1
    dict(case=(1, 2049, 2056), mb=1),      # nb = 2, the second block holds 1024 elements
    dict(case=(4099, 520, 528), mb=32),    # total = 2 131 480 > 1024 * 2048: per = 2082, nine trips of the thread loop
]
L1_GSCALAR = 2.5


def stride_B(rows_per_record, d, dtype):
    """the smallest B at which B * rows_per_record rows of d / VN vectors pass GRID_CAP * BLOCK: the stride loop takes a second trip"""
    return GRID_CAP * BLOCK // (rows_per_record * (d // VN[dtype])) + 1


def embed_shapes(dtype):
    """(B, n, d, forward_only) for ecgvit_embed_finish / _bwd: n + 1 rows per record"""
    return [s + (False,) for s in SHAPES] + [(stride_B(STRIDE_N + 1, STRIDE_D, dtype), STRIDE_N, STRIDE_D, True)]


def mask_shapes(dtype):
    """(B, n, d, forward_only) for ecgvit_mask_embed_finish / _bwd: n rows per record"""
    return [s + (False,) for s in SHAPES] + [(stride_B(STRIDE_N, STRIDE_D, dtype), STRIDE_N, STRIDE_D, True)]


def mask_counts(n):
    return sorted({0, 1, n // 2, n})


def shape_id(s):
    return 'x'.join(str(int(v)) for v in s)


def dtype_id(dt):
    return {F32: 'f32', BF16: 'bf16'}[dt]


# ---- the integer facts tests/test_embed_ref.py asserts
def batch_trips(B, lane=0):
    """trips of `for (b = lane; b < B; b += 32)`"""
    return max(0, -(-(B - lane) // BATCH_LANES))


def column_groups(d, dtype):
    """(groups of 8 column vectors, live vectors in the last group)"""
    dv = d // VN[dtype]
    g = -(-dv // GROUP)
    return g, dv - GROUP * (g - 1)


def stride_trips(vectors):
    """trips of the busiest thread of an element-wise launch over `vectors` 16-B vectors"""
    grid = max(1, min(-(-vectors // BLOCK), GRID_CAP))
    return -(-vectors // (grid * BLOCK))


def l1_blocks(total):
    """(nb, per): blocks of the first stage and the run of elements each owns"""
    nb = min(L1_BLOCKS, -(-total // L1_PER_BLOCK))
    return nb, -(-total // nb)


def l1_chain(total):
    """h, the longest chain of f32 roundings between an element and the loss (module docstring)"""
    nb, per = l1_blocks(total)
    return -(-per // BLOCK) + 10 + (-(-nb // 64) + 6) + 3


# ------------------------------------------------------------------------------------------------------------------ inputs
def _gen(*key):
    seed = 17
    for k in key:
        seed = (seed * 1000003 + int(k)) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(seed)


def embed_inputs(B, n, d, dtype, cls_row=True):
    """tok [B n, d] (dtype), cls or mask token [d] f32, pos [n + 1, d] f32, dX [B (n + 1 or n), d] (dtype); host tensors"""
    g = _gen(B, n, d, ESIZE[dtype], cls_row)
    rows = n + 1 if cls_row else n
    tok = torch.randn(B * n, d, generator=g).to(dtype)
    vec, pos = torch.randn(d, generator=g), torch.randn(n + 1, d, generator=g)
    dX = torch.randn(B * rows, d, generator=g).to(dtype)
    return tok, vec, pos, dX


def mask_index(B, n, m, seed=0):
    """int32 [B, m]: m distinct patches per record, by randperm (None when m == 0)"""
    if m == 0:
        return None
    g = _gen(B, n, m, seed, 77)
    return torch.stack([torch.randperm(n, generator=g)[:m] for _ in range(B)]).to(torch.int32)


def row_index(form, family):
    B, n, m = form[:3]
    g = _gen(*form)
    if family == 'zeros':
        return torch.zeros(B, m, dtype=torch.int32)
    if family == 'rising':
        return torch.stack([torch.randperm(n, generator=g)[:m].sort().values for _ in range(B)]).to(torch.int32)
    return torch.stack([torch.randperm(n, generator=g)[:m] for _ in range(B)]).to(torch.int32)


def l1_inputs(rows, width, ld, dtype):
    """pred, target [rows, ld] (dtype): standard normals, magnitudes under 2^-100 zeroed (no subnormal difference), about a tenth of the elements
    tied, NaN in the pitch gap"""
    g = _gen(rows, width, ld, ESIZE[dtype])
    pred, target = torch.randn(rows, ld, generator=g).to(dtype), torch.randn(rows, ld, generator=g).to(dtype)
    for t in (pred, target):
        t[t.float().abs() < 2.0 ** -100] = 0
    tie = torch.rand(rows, ld, generator=g) < 0.1
    target[tie] = pred[tie]
    pred[:, width:] = float('nan')
    target[:, width:] = float('nan')
    return pred, target


# ------------------------------------------------------------------------------------------------------------------ float64 restatement
def embed(tok, cls, pos, B, n, d):
    """X [B, n + 1, d] f64: row 0 = cls + pos[0], row 1 + p = tok[b n + p] + pos[1 + p]"""
    t = tok.to(F64).reshape(B, n, d)
    return torch.cat([cls.to(F64).reshape(1, 1, d).expand(B, 1, d), t], dim=1) + pos.to(F64).reshape(1, n + 1, d)


def embed_bwd(dX):
    """dX [B, n + 1, d] -> dtok [B, n, d], dcls [d], dpos [n + 1, d]"""
    dX = dX.to(F64)
    dpos = dX.sum(0)
    return dX[:, 1:], dpos[0].clone(), dpos       # dcls IS row 0 of dpos: the CLS row receives cls + pos[0]


def mask_of(idx, B, n, device=None):
    mask = torch.zeros(B, n, dtype=torch.bool, device=device if idx is None else idx.device)
    if idx is not None and idx.numel():
        mask.scatter_(1, idx.long(), True)
    return mask


def mask_embed(tok, mask_token, pos, idx, B, n, m, d):
    """(X [B, n, d] f64, mask [B, n] bool): X[b, p] = (p in idx[b] ? mask_token : tok[b n + p]) + pos[1 + p]; no CLS row"""
    assert (idx is None and m == 0) or tuple(idx.shape) == (B, m)
    mask = mask_of(idx, B, n, tok.device)
    src = torch.where(mask[..., None], mask_token.to(F64).reshape(1, 1, d), tok.to(F64).reshape(B, n, d))
    return src + pos.to(F64)[1:n + 1].reshape(1, n, d), mask


def mask_embed_bwd(dX, mask):
    """dX [B, n, d] -> dtok (dX off the mask, 0 on it), dmasked (dX on the mask, 0 off it; its sum over records and patches is the mask-token
    gradient), dpos [n + 1, d] with row 0 zero"""
    dX = dX.to(F64)
    zero = torch.zeros_like(dX)
    s = dX.sum(0)
    return torch.where(mask[..., None], zero, dX), torch.where(mask[..., None], dX, zero), torch.cat([torch.zeros_like(s[:1]), s], dim=0)


def l1(pred, target, rows, width, ld, gscalar=None):
    """(loss, dpred [rows, width]) f64: loss = mean |pred - target| over the first `width` columns of each pitch-`ld` row,
    dpred = gscalar sign(pred - target) / (rows width) (gscalar None: 1)"""
    diff = pred.reshape(rows, ld)[:, :width].to(F64) - target.reshape(rows, ld)[:, :width].to(F64)
    g = 1.0 if gscalar is None else float(gscalar)
    return diff.abs().mean(), g * torch.sign(diff) / (rows * width)


# ---- what the kernels must return bit for bit: the same expressions with the contract's one rounding
def embed_rounded(tok, cls, pos, B, n, d, dtype):
    t = tok.float().reshape(B, n, d)
    return (torch.cat([cls.float().reshape(1, 1, d).expand(B, 1, d), t], dim=1) + pos.float().reshape(1, n + 1, d)).to(dtype)


def mask_embed_rounded(tok, mask_token, pos, mask, B, n, d, dtype):
    src = torch.where(mask[..., None], mask_token.float().reshape(1, 1, d), tok.float().reshape(B, n, d))
    return (src + pos.float()[1:n + 1].reshape(1, n, d)).to(dtype)


def l1_dpred_rounded(pred, target, rows, width, ld, gscalar, dtype):
    """[rows, width] (dtype): (+-(g / (float)(rows width))) rounded once, exactly 0 at ties; the sign of an f32 difference of two normal values
    is exact"""
    diff = pred.reshape(rows, ld)[:, :width].float() - target.reshape(rows, ld)[:, :width].float()
    g = torch.tensor(1.0 if gscalar is None else float(gscalar), dtype=F32, device=diff.device)
    up = g / torch.tensor(float(rows * width), dtype=F32, device=diff.device)
    return (torch.sign(diff) * up).to(dtype)


# ------------------------------------------------------------------------------------------------------------------ bounds
def ulp32(x):
    """one f32 unit in the last place of |x| (f64 tensor; 0 at 0)"""
    _, e = torch.frexp(x.abs().to(F64))                         # |x| = m 2^e, m in [0.5, 1)
    return torch.where(x == 0, torch.zeros_like(x, dtype=F64), torch.ldexp(torch.ones_like(x, dtype=F64), e - 24))


def dpos_bound(dX, ref):
    """dX [B, rows, d] (the exact terms), ref [rows, d] = their f64 sum over B -> the bound of the module docstring"""
    B = dX.shape[0]
    return torch.maximum((B - 1) * U32 * dX.to(F64).abs().sum(0), ulp32(ref))


def worst_ratio(got, ref, bound):
    """max |got - ref| / bound, an exact result counting 0 whatever its bound"""
    err = (got.to(F64) - ref).abs()
    r = torch.where(err == 0, torch.zeros_like(err), err / bound)
    return float(r.max()) if r.numel() else 0.0
